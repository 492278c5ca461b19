// Host build (g++) of the pairing arithmetic in ark-blst_amd/csrc/pairing.cuh with the REAL 28-bit field, so the
// tower, the Miller loop and the final exponentiation can be checked against the oracle on a CPU-only box.
// Test helper only — not part of the shipped library.
#include <cstdint>
#include <cstring>
#include "../../ark-blst_amd/csrc/pairing.cuh"

using namespace fp28;
using T = pairing::Tower<pairing::PF2>;

static Fp load_fp(const uint8_t* p) {
    uint32_t w[12];
    memcpy(w, p, 48);
    return fp_from_blst(w);
}
static void store_fp(uint8_t* p, const Fp& a) {
    uint32_t w[12];
    fp_to_blst(w, a);
    memcpy(p, w, 48);
}
static ec::Fp2 load_fp2(const uint8_t* p) { return ec::Fp2{load_fp(p), load_fp(p + 48)}; }
static T::E12 load_fp12(const uint8_t* p) {   // member by member (no pointer walk across struct members)
    T::E12 r;
    ec::Fp2* c[6] = {&r.c0.c0, &r.c0.c1, &r.c0.c2, &r.c1.c0, &r.c1.c1, &r.c1.c2};
    for (int i = 0; i < 6; i++) *c[i] = load_fp2(p + 96 * i);
    return r;
}
static void store_fp12(uint8_t* p, const T::E12& a) {
    const ec::Fp2* c[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
    for (int i = 0; i < 6; i++) {
        store_fp(p + 96 * i, c[i]->c0);
        store_fp(p + 96 * i + 48, c[i]->c1);
    }
}
static Fp raw_fp(const uint32_t* p) {
    Fp r;
    memcpy(r.l, p, sizeof r.l);
    return r;
}
static ec::Fp2 raw_fp2(const uint32_t* p) { return ec::Fp2{raw_fp(p), raw_fp(p + 16)}; }
static void put_fp2(uint32_t* p, const ec::Fp2& a) {
    memset(p, 0, 32 * 4);
    memcpy(p, a.c0.l, sizeof a.c0.l);
    memcpy(p + 16, a.c1.l, sizeof a.c1.l);
}
static T::E12 raw_fp12(const uint32_t* p) {
    T::E12 r;
    ec::Fp2* c[6] = {&r.c0.c0, &r.c0.c1, &r.c0.c2, &r.c1.c0, &r.c1.c1, &r.c1.c2};
    for (int i = 0; i < 6; i++) *c[i] = raw_fp2(p + 32 * i);
    return r;
}
static void put_fp12(uint32_t* p, const T::E12& a) {
    const ec::Fp2* c[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
    for (int i = 0; i < 6; i++) put_fp2(p + 32 * i, *c[i]);
}

extern "C" {

void hp_fp12_mul(const uint8_t* a, const uint8_t* b, uint8_t* out) { store_fp12(out, T::mul12(load_fp12(a), load_fp12(b))); }
void hp_fp12_sqr(const uint8_t* a, uint8_t* out) { store_fp12(out, T::sqr12(load_fp12(a))); }
void hp_fp12_inv(const uint8_t* a, uint8_t* out) { store_fp12(out, T::inv12(load_fp12(a))); }
void hp_fp12_frob(const uint8_t* a, uint8_t* out) { store_fp12(out, T::frob12(load_fp12(a))); }
void hp_final_exp(const uint8_t* a, uint8_t* out) { store_fp12(out, T::final_exp(load_fp12(a))); }
// p: blst_p1_affine (96 B), q: blst_p2_affine (192 B), both not infinity
void hp_miller_loop(const uint8_t* p, const uint8_t* q, uint8_t* out) {
    T::G1Pt g{fp_neg<4>(load_fp(p)), load_fp(p + 48)};
    store_fp12(out, T::miller_loop(g, load_fp2(q), load_fp2(q + 96)));
}

// ---- raw device-form limbs in 16-word slots (no conversion), the operand layouts of mi_test_field_op's line ops and of
// mi_test_pairing_stage: the GENERIC tower on the vectors of tests/pairing_stage_util.py
void hp_line_op(int add, const uint32_t* in, size_t n, uint32_t* out) {
    const size_t nin = add ? 12 : 8;
    for (size_t e = 0; e < n; e++) {
        const uint32_t* p = in + e * nin * 16;
        T::PT t{raw_fp2(p), raw_fp2(p + 32), raw_fp2(p + 64)};
        const T::G1Pt g{raw_fp(p + 96), raw_fp(p + 112)};
        ec::Fp2 c0, c1, c4;
        if (add) T::line_add(t, raw_fp2(p + 128), raw_fp2(p + 160), g, c0, c1, c4);
        else T::line_dbl(t, g, c0, c1, c4);
        const ec::Fp2 r[6] = {c0, c1, c4, t.x, t.y, t.z};
        for (int k = 0; k < 6; k++) put_fp2(out + (e * 6 + k) * 32, r[k]);
    }
}
// k_miller_accumulate's job with the generic tower: f <- f^2 l_1 .. l_m per step over the production line buffer layout, conjugated
void hp_accumulate_raw(const uint32_t* lines, size_t n, unsigned m, uint32_t* out) {
    const size_t blk = 10 * (size_t)m, groups = (n + m - 1) / m;
    for (size_t g = 0; g < groups; g++) {
        T::E12 f = T::one12();
        int line = 0;
        auto mul_line = [&]() {
            for (size_t pair = g * m; pair < g * m + m && pair < n; pair++) {
                const uint32_t* lp = lines + ((pair / blk * 68 * blk + pair % blk) + (size_t)line * blk) * 96;
                f = T::mul_by_014(f, raw_fp2(lp), raw_fp2(lp + 32), raw_fp2(lp + 64));
            }
            line++;
        };
        for (int b = 62; b >= 0; b--) {
            f = T::sqr12(f);
            mul_line();
            if ((fp28c::Z_ABS >> b) & 1) mul_line();
        }
        put_fp12(out + g * 192, T::conj12(f));
    }
}
void hp_fp12_mul_raw(const uint32_t* a, const uint32_t* b, uint32_t* out) { put_fp12(out, T::mul12(raw_fp12(a), raw_fp12(b))); }

}  // extern "C"
