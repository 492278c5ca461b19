// Host build (g++) of the fixed-base walk (ark-blst_amd/csrc/fixed_base_kernels.cuh k_fb_walk) over a host-built table, from the SAME
// ec.cuh / fp28.cuh formulas the kernels use: XYZZ hot loop with the inlined multiplier, complete additions from the first exceptional pair on.
// The signed-digit recoding is RESTATED here (fb_digit / scalar_bits live in kernels_common.cuh, which needs the HIP headers); the scalar
// itself is loaded by the kernels' own fr::load_scalar (fr.cuh).  Test helper only — not part of the shipped library.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../ark-blst_amd/csrc/ec.cuh"
#include "../../ark-blst_amd/csrc/fr.cuh"
#include "../../ark-blst_amd/csrc/fixed_base_model.hpp"

using namespace fp28;
using F = ec::FpOps;
using FA = ec::FpOpsInline;
using Pj = ec::Proj<F>;

static Fp load_blst(const uint8_t* p) {
    uint32_t w[12];
    memcpy(w, p, 48);
    return fp_from_blst(w);
}
static void store_blst(uint8_t* p, const Fp& a) {
    uint32_t w[12];
    fp_to_blst(w, a);
    memcpy(p, w, 48);
}
static void store_proj_as_jac(uint8_t* out, const Pj& p) {
    uint8_t z[48];
    store_blst(z, p.z);
    bool any = false;
    for (int k = 0; k < 48; k++) any |= z[k] != 0;
    if (!any) { memset(out, 0, 144); return; }
    Fp zz = fp_mul(p.z, p.z);
    store_blst(out, fp_mul(p.x, p.z));
    store_blst(out + 48, fp_mul(p.y, zz));
    memcpy(out + 96, z, 48);
}
static Fp fp_inv(const Fp& a) {   // a^(p - 2); P[] are the 28-bit limbs of p, the low one is odd and > 2
    Fp r = fp_one();
    for (int k = NL - 1; k >= 0; k--) {
        const uint32_t limb = k == 0 ? P[0] - 2 : P[k];
        for (int b = 27; b >= 0; b--) {
            r = fp_mul(r, r);
            if ((limb >> b) & 1) r = fp_mul(r, a);
        }
    }
    return r;
}

struct Entry { Fp x, y; bool inf; };

static uint32_t scalar_bits(const uint32_t* s, uint32_t off, uint32_t c) {
    uint64_t v = 0;
    const uint32_t w = off >> 5, sh = off & 31;
    if (w < 8) v = s[w];
    if (w + 1 < 8) v |= (uint64_t)s[w + 1] << 32;
    return (uint32_t)(v >> sh) & ((1u << c) - 1u);
}
static const uint32_t NONE = 0xffffffffu;
static uint32_t digit(const uint32_t* s, uint32_t win, uint32_t c, uint32_t& carry) {
    const uint32_t raw = scalar_bits(s, win * c, c) + carry, half = 1u << (c - 1);
    const bool neg = raw > half;
    carry = neg ? 1u : 0u;
    const uint32_t mag = neg ? (1u << c) - raw : raw;
    return mag == 0 ? NONE : (((win << (c - 1)) + (mag - 1)) | (neg ? 0x80000000u : 0u));
}

extern "C" {

unsigned fbw_windows(unsigned w) { return mi::fbm::windows(w); }

// out[i] = scalars[i] * base as blst Jacobian bytes, cold[i] = the lane left the hot loop.  base: a finite point of the curve (any order).
int fbw_g1(const uint8_t* base, unsigned c, const uint8_t* scalars, size_t n, uint8_t* out, uint8_t* cold) {
    if (c < mi::fbm::W_MIN || c > mi::fbm::W_MAX) return -1;
    const uint32_t nwin = mi::fbm::windows(c), half = 1u << (c - 1);
    const size_t N = (size_t)nwin * half;
    // ---- table, as the build kernels make it: window bases by doublings, (2^k + u) B = u B + 2^k B level by level, one shared inversion
    std::vector<Pj> proj(N);
    Pj p = ec::proj_from_affine<F>(load_blst(base), load_blst(base + 48));
    for (uint32_t j = 0; j < nwin; j++) {
        proj[(size_t)j * half] = p;
        if (j + 1 < nwin)
            for (uint32_t k = 0; k < c; k++) ec::proj_dbl<F>(p);
    }
    for (uint32_t k = 0; k + 1 < c; k++)
        for (uint32_t j = 0; j < nwin; j++)
            for (uint32_t u = 0; u < (1u << k); u++) {
                Pj a = proj[(size_t)j * half + u];
                ec::proj_add<FA>(a, proj[(size_t)j * half + (1u << k) - 1]);
                proj[(size_t)j * half + (1u << k) + u] = a;
            }
    std::vector<Entry> tab(N);
    std::vector<Fp> pref(N);
    Fp run = fp_one();
    for (size_t i = 0; i < N; i++) {
        Fp z = fp_mul(proj[i].z, fp_one());
        tab[i].inf = fp_is_zero_2p(z);
        proj[i].z = tab[i].inf ? fp_one() : z;
        pref[i] = run;
        run = fp_mul(run, proj[i].z);
    }
    Fp I = fp_inv(run);
    for (size_t i = N; i-- > 0;) {
        const Fp zi = fp_mul(I, pref[i]);
        I = fp_mul(I, proj[i].z);
        tab[i].x = fp_mul(proj[i].x, zi);
        tab[i].y = fp_mul(proj[i].y, zi);
    }
    // ---- walk, the structure of k_fb_walk
    for (size_t i = 0; i < n; i++) {
        uint32_t raw[8], s[8];
        memcpy(raw, scalars + 32 * i, 32);
        fr::load_scalar(s, raw, 0, 0);   // canonical, no fold: as k_fb_walk loads it
        uint32_t win = 0, carry = 0, ent = NONE;
        bool have = false;
        while (win < nwin && !have) {
            ent = digit(s, win, c, carry);
            win++;
            have = ent != NONE && !tab[ent & 0x7fffffffu].inf;
        }
        ec::Xyzz<FA> acc;
        {
            const uint32_t e0 = have ? ent : 0u;
            Fp x = tab[e0 & 0x7fffffffu].x, y = tab[e0 & 0x7fffffffu].y;
            if (e0 >> 31) y = FA::neg_l<4>(y);
            acc.x = x; acc.y = FA::norm(y); acc.zz = fp_one(); acc.zzz = fp_one();
        }
        bool special = false;
        while (win < nwin) {
            ent = digit(s, win, c, carry);
            win++;
            if (ent == NONE || tab[ent & 0x7fffffffu].inf) continue;
            Fp x = tab[ent & 0x7fffffffu].x, y = tab[ent & 0x7fffffffu].y;
            if (ent >> 31) y = FA::neg_l<4>(y);
            if (ec::xyzz_madd<FA>(acc, x, y)) { special = true; break; }
        }
        cold[i] = special ? 1 : 0;
        Pj o = ec::proj_inf<F>();
        if (have) o = ec::xyzz_to_proj<F>(acc);
        while (special || win < nwin) {
            if (!special) {
                ent = digit(s, win, c, carry);
                win++;
            }
            special = false;
            if (ent == NONE || tab[ent & 0x7fffffffu].inf) continue;
            Fp x = tab[ent & 0x7fffffffu].x, y = tab[ent & 0x7fffffffu].y;
            if (ent >> 31) y = fp_neg<4>(y);
            const Pj q = ec::proj_from_affine<F>(x, y);
            ec::proj_add<F>(o, q);
        }
        if (carry) return -2;   // the window count must absorb every carry
        store_proj_as_jac(out + 144 * i, o);
    }
    return 0;
}
}
