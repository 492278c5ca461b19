// Plain C++ reference of mi_fr_scan and mi_fr_batch_inverse for sizes Python does not reach: the running product / sum as the serial loop, the
// inversion as Montgomery's trick with zeros skipped and a^(r - 2), on 4 x 64-bit limbs with Montgomery multiplication on unsigned __int128 (the
// arithmetic of fr_ntt_ref.cpp).  Shares no code with csrc/fr.cuh or scan_kernels.cuh; tests/test_fr_scan_cpu.py pins it against scan_util.  Also
// the CPU baseline of tools/bench_scan.py: a vector is cut into `threads` chunks (scan: chunk totals, a serial pass over them, then the chunks'
// prefixes; inversion: one inversion per chunk).   fr_scan_ref <in> <out>
//   in:  u32 kind (0 scan, 1 inverse), n, batch, fmt (0 canonical, 1 Montgomery), threads, op (0 MUL, 1 ADD), exclusive, flags (bit 0: inverse with
//        numerators, bit 1: scan without the output vector); batch x n x 32 bytes; with numerators n x 32 bytes more
//   out: batch x n x 32 bytes (absent for a scan without output); scan: batch x 32 bytes of totals; inverse: u64 zeros; f64 seconds of the work alone
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

static bool is_zero(const F& a) { return (a.l[0] | a.l[1] | a.l[2] | a.l[3]) == 0; }
static F one() { return mul(R2, F{{1, 0, 0, 0}}); }   // 2^256 mod r
static F inverse(const F& a) {   // a^(r - 2)
    const F e = sub_raw(MOD, F{{2, 0, 0, 0}});
    F r = one();
    for (int bit = 254; bit >= 0; bit--) {
        r = mul(r, r);
        if ((e.l[bit >> 6] >> (bit & 63)) & 1) r = mul(r, a);
    }
    return r;
}
template <class Fn>
static void parallel(size_t threads, size_t n, Fn fn) {   // fn(chunk, lo, hi) over `threads` chunks of [0, n)
    std::vector<std::thread> pool;
    for (size_t t = 1; t < threads; t++) pool.emplace_back(fn, t, n * t / threads, n * (t + 1) / threads);
    fn(0, 0, n / threads);
    for (auto& th : pool) th.join();
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    init();
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hd[8];
    if (fread(hd, sizeof hd, 1, f) != 1) return 2;
    const bool invert = hd[0] == 1;
    const size_t n = hd[1], batch = hd[2];
    const unsigned fmt = hd[3], op = hd[5];
    const size_t threads = std::max<size_t>(1, std::min<size_t>(hd[4], n));
    const bool exclusive = hd[6] != 0, with_num = hd[7] & 1u, no_out = hd[7] & 2u;
    if (hd[0] > 1 || n > ((size_t)1 << 26) || batch == 0 || op > 1 || (invert && batch != 1)) return 2;
    const size_t total = batch * n;
    std::vector<F> data(total), num(with_num ? n : 0), totals(batch);
    if ((total != 0 && fread(data.data(), 32, total, f) != total) || (!num.empty() && fread(num.data(), 32, num.size(), f) != num.size())) return 2;
    fclose(f);
    uint64_t zeros = 0;
    const F id = op == 0 ? one() : F{{0, 0, 0, 0}};
    const auto t0 = std::chrono::steady_clock::now();
    if (invert) {
        std::vector<uint64_t> zc(threads, 0);
        std::vector<F> pre(n);   // the running product of the chunk's non-zero elements before each element
        parallel(threads, n, [&](size_t c, size_t lo, size_t hi) {
            F acc = one();
            for (size_t i = lo; i < hi; i++) {
                data[i] = load(data[i], fmt);
                pre[i] = acc;
                if (is_zero(data[i])) zc[c]++;
                else acc = mul(acc, data[i]);
            }
            F inv = inverse(acc);
            for (size_t i = hi; i-- > lo;) {
                F r = {{0, 0, 0, 0}};
                if (!is_zero(data[i])) {
                    r = mul(inv, pre[i]);
                    inv = mul(inv, data[i]);
                    if (with_num) r = mul(r, load(num[i], fmt));
                }
                data[i] = store(r, fmt);
            }
        });
        for (uint64_t z : zc) zeros += z;
    } else {
        auto comb = [&](const F& a, const F& b) { return op == 0 ? mul(a, b) : add(a, b); };
        std::vector<F> part(threads);
        for (size_t v = 0; v < batch; v++) {
            F* a = data.data() + v * n;
            parallel(threads, n, [&](size_t c, size_t lo, size_t hi) {
                F acc = id;
                for (size_t i = lo; i < hi; i++) acc = comb(acc, a[i] = load(a[i], fmt));
                part[c] = acc;
            });
            F acc = id;
            for (size_t c = 0; c < threads; c++) {
                const F t = part[c];
                part[c] = acc;
                acc = comb(acc, t);
            }
            totals[v] = store(n ? acc : id, fmt);
            if (no_out) continue;
            parallel(threads, n, [&](size_t c, size_t lo, size_t hi) {
                F y = part[c];
                for (size_t i = lo; i < hi; i++) {
                    const F next = comb(y, a[i]);
                    a[i] = store(exclusive ? y : next, fmt);
                    y = next;
                }
            });
        }
    }
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    if (!(no_out && !invert) && total != 0 && fwrite(data.data(), 32, total, f) != total) return 2;
    if (invert ? fwrite(&zeros, 8, 1, f) != 1 : fwrite(totals.data(), 32, batch, f) != batch) return 2;
    if (fwrite(&secs, 8, 1, f) != 1) return 2;
    fclose(f);
    return 0;
}
