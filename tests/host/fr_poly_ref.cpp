// Plain C++ reference of mi_fr_poly_open for sizes Python does not reach: the serial Horner recurrence S_n = 0, S_i = p_i + z S_(i+1), q_i = S_(i+1),
// p(z) = S_0 on 4 x 64-bit limbs with Montgomery multiplication on unsigned __int128 (the arithmetic of fr_ntt_ref.cpp).  Shares no code with
// csrc/fr.cuh or poly_kernels.cuh; tests/test_fr_poly_cpu.py pins it against poly_util.  Also the CPU baseline of tools/bench_poly.py (the
// polynomials of a batch on `threads` threads).   fr_poly_ref <in> <out>
//   in:  u32 n, batch, n_points, fmt (0 canonical, 1 Montgomery), threads, evaluate_only; n_points x 32 bytes; batch x n x 32 bytes
//   out: batch x n x 32 bytes of quotients (element n - 1 zero; absent with evaluate_only), batch x 32 bytes of values, f64 seconds of the work alone
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

typedef unsigned __int128 u128;
struct F {
    uint64_t l[4];
};
static const F MOD = {{0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull}};
static uint64_t NINV;   // -r^-1 mod 2^64
static F R2;            // 2^512 mod r

static bool geq(const F& a, const F& b) {
    for (int k = 3; k >= 0; k--)
        if (a.l[k] != b.l[k]) return a.l[k] > b.l[k];
    return true;
}
static F sub_raw(const F& a, const F& b) {   // a - b mod 2^256
    F r;
    uint64_t borrow = 0;
    for (int k = 0; k < 4; k++) {
        const u128 x = (u128)a.l[k] - b.l[k] - borrow;
        r.l[k] = (uint64_t)x;
        borrow = (uint64_t)(x >> 64) & 1;
    }
    return r;
}
static F add(const F& a, const F& b) {   // a, b < r < 2^255: no carry out of 256 bits
    F r;
    u128 c = 0;
    for (int k = 0; k < 4; k++) {
        c += (u128)a.l[k] + b.l[k];
        r.l[k] = (uint64_t)c;
        c >>= 64;
    }
    return geq(r, MOD) ? sub_raw(r, MOD) : r;
}
static F mul(const F& a, const F& b) {   // a b 2^-256 mod r
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        u128 c = 0;
        for (int j = 0; j < 4; j++) {
            c += (u128)a.l[j] * b.l[i] + t[j];
            t[j] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[4] = (uint64_t)c;
        t[5] = (uint64_t)(c >> 64);
        const uint64_t m = t[0] * NINV;
        c = (u128)m * MOD.l[0] + t[0];
        c >>= 64;
        for (int j = 1; j < 4; j++) {
            c += (u128)m * MOD.l[j] + t[j];
            t[j - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = t[5] + (uint64_t)(c >> 64);
    }
    F r = {{t[0], t[1], t[2], t[3]}};
    return (t[4] || geq(r, MOD)) ? sub_raw(r, MOD) : r;
}
static F reduce(F a) {
    while (geq(a, MOD)) a = sub_raw(a, MOD);
    return a;
}
static void init() {
    uint64_t x = 1;   // Newton: r^-1 mod 2^64
    for (int k = 0; k < 6; k++) x *= 2 - MOD.l[0] * x;
    NINV = 0 - x;
    F r2 = reduce(sub_raw(F{{0, 0, 0, 0}}, MOD));   // 2^256 mod r, doubled 256 times: 2^512 mod r
    for (int k = 0; k < 256; k++) r2 = add(r2, r2);
    R2 = r2;
}
static F load(const F& w, unsigned fmt) {   // the stored word -> Montgomery form below r
    const F x = reduce(w);
    return fmt == 0 ? mul(x, R2) : x;
}
static F store(const F& a, unsigned fmt) { return fmt == 0 ? mul(a, F{{1, 0, 0, 0}}) : a; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    init();
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hd[6];
    if (fread(hd, sizeof hd, 1, f) != 1) return 2;
    const size_t n = hd[0], batch = hd[1], n_points = hd[2];
    const unsigned fmt = hd[3], threads = hd[4] ? hd[4] : 1;
    const bool evaluate_only = hd[5] != 0;
    if (n > ((size_t)1 << 26) || batch == 0 || (n_points != 1 && n_points != batch)) return 2;
    const size_t total = batch * n;
    std::vector<F> points(n_points), data(total), values(batch);
    if (fread(points.data(), 32, n_points, f) != n_points || (total != 0 && fread(data.data(), 32, total, f) != total)) return 2;
    fclose(f);
    const auto t0 = std::chrono::steady_clock::now();
    auto work = [&](size_t v0, size_t v1) {
        for (size_t v = v0; v < v1; v++) {
            const F z = load(points[n_points > 1 ? v : 0], fmt);
            F* a = data.data() + v * n;
            F s = {{0, 0, 0, 0}};   // S_(i+1)
            for (size_t i = n; i-- > 0;) {
                const F p = load(a[i], fmt);
                if (!evaluate_only) a[i] = store(s, fmt);
                s = add(p, mul(s, z));
            }
            values[v] = store(s, fmt);
        }
    };
    std::vector<std::thread> pool;
    const size_t T = std::min<size_t>(threads, batch);
    for (size_t t = 1; t < T; t++) pool.emplace_back(work, batch * t / T, batch * (t + 1) / T);
    work(0, batch / T);
    for (auto& th : pool) th.join();
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (!evaluate_only && total != 0 && fwrite(data.data(), 32, total, f) != total) return 2;
    if (fwrite(values.data(), 32, batch, f) != batch || fwrite(&secs, 8, 1, f) != 1) return 2;
    fclose(f);
    return 0;
}
