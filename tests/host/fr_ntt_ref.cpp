// Plain C++ reference of the radix-2 NTT over the BLS12-381 scalar field for sizes Python does not reach: 4 x 64-bit limbs, Montgomery
// multiplication on unsigned __int128, bit reversal + in-place decimation-in-time levels over a full table of n / 2 twiddles.  Shares no code
// with csrc/fr.cuh or ntt_kernels.cuh (its constants are computed here from r and 7); tests/test_fr_ntt_cpu.py pins it against ntt_util.
// Also the CPU baseline of tools/bench_ntt.py (the vectors of a batch on `threads` threads).   fr_ntt_ref <in> <out>
//   in:  u32 log_n, batch, inverse, has_offset, fmt (0 canonical, 1 Montgomery), threads; 32-byte offset in fmt; batch x 2^log_n x 32 bytes
//   out: batch x 2^log_n x 32 bytes in fmt, then f64 seconds of the transforms alone
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
static F ONE, R2;       // 2^256 mod r, 2^512 mod r

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
static F add_raw(const F& a, const F& b) {
    F r;
    u128 c = 0;
    for (int k = 0; k < 4; k++) {
        c += (u128)a.l[k] + b.l[k];
        r.l[k] = (uint64_t)c;
        c >>= 64;
    }
    return r;
}
static F add(const F& a, const F& b) {   // a, b < r < 2^255: no carry out of 256 bits
    const F r = add_raw(a, b);
    return geq(r, MOD) ? sub_raw(r, MOD) : r;
}
static F sub(const F& a, const F& b) { return geq(a, b) ? sub_raw(a, b) : add_raw(sub_raw(a, b), MOD); }
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
static F pow(F a, const uint64_t* e, int words) {
    F r = ONE;
    for (int bit = 64 * words - 1; bit >= 0; bit--) {
        r = mul(r, r);
        if ((e[bit >> 6] >> (bit & 63)) & 1) r = mul(r, a);
    }
    return r;
}
static F inv(const F& a) {
    const F e = sub_raw(MOD, F{{2, 0, 0, 0}});
    return pow(a, e.l, 4);
}
static void init() {
    uint64_t x = 1;   // Newton: r^-1 mod 2^64
    for (int k = 0; k < 6; k++) x *= 2 - MOD.l[0] * x;
    NINV = 0 - x;
    F one = reduce(sub_raw(F{{0, 0, 0, 0}}, MOD));   // 2^256 - r, reduced: 2^256 mod r
    ONE = one;
    F r2 = one;                                      // doubling 256 times: 2^512 mod r
    for (int k = 0; k < 256; k++) r2 = add(r2, r2);
    R2 = r2;
}

static void ntt(F* a, unsigned log_n, const F* tw) {   // tw[i] = w^i, i < n / 2
    const size_t n = (size_t)1 << log_n;
    for (size_t i = 0, j = 0; i < n; i++) {
        if (i < j) std::swap(a[i], a[j]);
        size_t bit = n >> 1;
        for (; bit && (j & bit); bit >>= 1) j ^= bit;
        j ^= bit;
    }
    for (unsigned s = 0; s < log_n; s++) {
        const size_t half = (size_t)1 << s, step = n >> (s + 1);
        for (size_t start = 0; start < n; start += 2 * half)
            for (size_t i = 0; i < half; i++) {
                const F x = a[start + i], y = mul(a[start + i + half], tw[i * step]);
                a[start + i] = add(x, y);
                a[start + i + half] = sub(x, y);
            }
    }
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    init();
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hd[6];
    F off;
    if (fread(hd, sizeof hd, 1, f) != 1 || fread(&off, 32, 1, f) != 1) return 2;
    const unsigned log_n = hd[0], fmt = hd[4], threads = hd[5] ? hd[5] : 1;
    const size_t batch = hd[1], n = (size_t)1 << log_n;
    const bool inverse = hd[2] != 0, has_offset = hd[3] != 0;
    if (log_n > 26) return 2;
    std::vector<F> data(batch * n);
    if (fread(data.data(), 32, batch * n, f) != batch * n) return 2;
    fclose(f);
    // w = (7^((r - 1) / 2^32))^(2^(32 - log_n)), inverted for the inverse direction
    F seven = ONE;
    for (int k = 0; k < 6; k++) seven = add(seven, ONE);
    const F e = sub_raw(MOD, F{{1, 0, 0, 0}});
    const uint64_t e32[4] = {(e.l[0] >> 32) | (e.l[1] << 32), (e.l[1] >> 32) | (e.l[2] << 32), (e.l[2] >> 32) | (e.l[3] << 32), e.l[3] >> 32};
    F w = pow(seven, e32, 4);
    for (unsigned k = log_n; k < 32; k++) w = mul(w, w);
    if (inverse) w = inv(w);
    std::vector<F> tw(n > 1 ? n / 2 : 1);
    tw[0] = ONE;
    for (size_t i = 1; i < tw.size(); i++) tw[i] = mul(tw[i - 1], w);
    F g = ONE;
    if (has_offset) {
        g = reduce(off);
        if (fmt == 0) g = mul(g, R2);
        if (inverse) g = inv(g);
    }
    F ninv = ONE;
    if (inverse) {
        F nn = ONE;
        for (unsigned k = 0; k < log_n; k++) nn = add(nn, nn);
        ninv = inv(nn);
    }
    const F plain_one = {{1, 0, 0, 0}};
    const auto t0 = std::chrono::steady_clock::now();
    auto work = [&](size_t v0, size_t v1) {
        for (size_t v = v0; v < v1; v++) {
            F* a = &data[v * n];
            for (size_t i = 0; i < n; i++) {
                a[i] = reduce(a[i]);
                if (fmt == 0) a[i] = mul(a[i], R2);
            }
            if (has_offset && !inverse) {
                F p = ONE;
                for (size_t i = 0; i < n; i++) { a[i] = mul(a[i], p); p = mul(p, g); }
            }
            ntt(a, log_n, tw.data());
            if (inverse) {
                F p = ninv;
                for (size_t i = 0; i < n; i++) { a[i] = mul(a[i], p); if (has_offset) p = mul(p, g); }
            }
            if (fmt == 0)
                for (size_t i = 0; i < n; i++) a[i] = mul(a[i], plain_one);
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
    if (fwrite(data.data(), 32, batch * n, f) != batch * n || fwrite(&secs, 8, 1, f) != 1) return 2;
    fclose(f);
    return 0;
}
