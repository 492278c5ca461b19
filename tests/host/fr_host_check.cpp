// Host build (g++) of csrc/fr.cuh: the Fr arithmetic of the NTT on a CPU-only box, against Python integers (tests/test_fr_ntt_cpu.py).
// Stand-alone program, also built under AddressSanitizer + UBSan.   fr_host_check <in> <out>
//   in:  u64 count, then count pairs (a, b) of 32-byte words (any 256-bit values)
//   out: per pair ten 32-byte words: for fmt = canonical, Montgomery: store(load(a) * load(b)), store(.. + ..), store(.. - ..);
//        then to_mont(reduce(a)), from_mont(reduce(a)), load(a) as canonical, load(a) as Montgomery
// Before it reads anything the program checks fr::load_scalar by itself (check_load_scalar below) and exits with 1 on a mismatch.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../ark-blst_amd/csrc/fr.cuh"

// ---- fr::load_scalar (the MSM's and the fixed-base walk's scalar prologue) against arithmetic on plain 64-bit limbs, restated here:
// the value and the flip flag for 0, 1, r - 1, r, r + 1, 2r, 2^256 - 1, (r - 1) / 2, (r + 1) / 2, both formats, fold on and off.
namespace limbs {
struct U256 { uint64_t l[4]; };
static const U256 R = {{0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull}};
static U256 add(const U256& a, const U256& b) {   // callers keep the sum below 2^256
    U256 r;
    uint64_t c = 0;
    for (int k = 0; k < 4; k++) {
        const uint64_t s = a.l[k] + c, c1 = s < c;
        r.l[k] = s + b.l[k];
        c = c1 + (r.l[k] < s);
    }
    return r;
}
static U256 sub(const U256& a, const U256& b) {   // a >= b
    U256 r;
    uint64_t bw = 0;
    for (int k = 0; k < 4; k++) {
        const uint64_t d = a.l[k] - bw, b1 = a.l[k] < bw;
        r.l[k] = d - b.l[k];
        bw = b1 + (d < b.l[k]);
    }
    return r;
}
static bool less(const U256& a, const U256& b) {
    for (int k = 3; k >= 0; k--)
        if (a.l[k] != b.l[k]) return a.l[k] < b.l[k];
    return false;
}
static U256 half(const U256& a) {
    U256 r;
    for (int k = 0; k < 4; k++) r.l[k] = (a.l[k] >> 1) | (k < 3 ? a.l[k + 1] << 63 : 0);
    return r;
}
static U256 mod_r(U256 a) {
    while (!less(a, R)) a = sub(a, R);
    return a;
}
// a 2^-256 mod r by 256 halvings modulo r (an odd value becomes even by adding r; below r the sum fits 256 bits)
static U256 from_mont(const U256& a) {
    U256 x = mod_r(a);
    for (int k = 0; k < 256; k++) x = half((x.l[0] & 1) ? add(x, R) : x);
    return x;
}
}  // namespace limbs

static int check_load_scalar() {
    using namespace limbs;
    const U256 zero = {{0, 0, 0, 0}}, one = {{1, 0, 0, 0}}, ones = {{~0ull, ~0ull, ~0ull, ~0ull}};
    const U256 in[9] = {zero, one, sub(R, one), R, add(R, one), add(R, R), ones, half(sub(R, one)), half(add(R, one))};
    int bad = 0;
    for (int c = 0; c < 9; c++)
        for (unsigned fmt = 0; fmt < 4; fmt++) {   // bit 0: Montgomery, bit 1: fold
            alignas(16) uint32_t words[3][8];       // the case is element 1 of a vector
            memset(words, 0xa5, sizeof words);
            for (int k = 0; k < 8; k++) words[1][k] = (uint32_t)(in[c].l[k / 2] >> (32 * (k % 2)));
            U256 want = (fmt & 1u) ? from_mont(in[c]) : mod_r(in[c]);
            bool want_flip = false;
            if ((fmt & 2u) && less(zero, want) && less(sub(R, want), want)) { want = sub(R, want); want_flip = true; }
            uint32_t s[8];
            const bool flip = fr::load_scalar(s, &words[0][0], 1, fmt);
            bool same = flip == want_flip;
            for (int k = 0; k < 8; k++) same = same && s[k] == (uint32_t)(want.l[k / 2] >> (32 * (k % 2)));
            if (!same) {
                fprintf(stderr, "load_scalar: input %d, fmt %u: flip %d (want %d), value", c, fmt, (int)flip, (int)want_flip);
                for (int k = 7; k >= 0; k--) fprintf(stderr, " %08x", s[k]);
                fprintf(stderr, "\n");
                bad++;
            }
        }
    return bad;
}

int main(int argc, char** argv) {
    if (check_load_scalar() != 0) return 1;
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t count = 0;
    if (fread(&count, 8, 1, f) != 1) return 2;
    std::vector<uint32_t> in(count * 16), out(count * 80);
    if (count && fread(in.data(), 64, count, f) != count) return 2;
    fclose(f);
    for (uint64_t i = 0; i < count; i++) {
        const uint32_t *a = &in[i * 16], *b = a + 8;
        uint32_t* o = &out[i * 80];
        for (unsigned fmt = 0; fmt < 2; fmt++) {
            const fr::Fr x = fr::load(a, 0, fmt), y = fr::load(b, 0, fmt);
            fr::store(o, 3 * fmt + 0, fr::mul(x, y), fmt);
            fr::store(o, 3 * fmt + 1, fr::add(x, y), fmt);
            fr::store(o, 3 * fmt + 2, fr::sub(x, y), fmt);
        }
        const fr::Fr ra = fr::reduce(fr::load_words(a));
        fr::store_words(o + 48, fr::to_mont(ra));
        fr::store_words(o + 56, fr::from_mont(ra));
        fr::store_words(o + 64, fr::load(a, 0, fr::FMT_CANONICAL));
        fr::store_words(o + 72, fr::load(a, 0, fr::FMT_MONTGOMERY));
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (count && fwrite(out.data(), 320, count, f) != count) return 2;
    fclose(f);
    return 0;
}
