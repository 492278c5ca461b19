// Radix-2 NTT over Fr (mi_fr_ntt): the pass plan, the index maps and butterflies of one pass, and the kernels.
//
// Convention (arkworks Radix2EvaluationDomain, natural order in and out): forward out[k] = sum_j a[j] w^(jk), w = ROOT^(2^(32 - log_n)).
// The log_n butterfly levels are decimation in frequency, grouped into passes over global memory.  A pass of b levels with s = 2^log_s
// (the product of the radices of the passes before it), R = 2^b and m = n / (s R) takes, for every column c = q + s p (q < s, p < m), the R
// elements in[c + (n / R) j], runs their R-point transform with the twiddles w^(s 2^l (p + m jj)) of level l, and writes result k to
// out[q + s (R p + k)] (the self-sorting Stockham index map: after the last pass the order is natural, no bit-reversal pass).  A workgroup holds
// a tile of 2^log_ct neighbouring columns in LDS — every global run is 2^log_ct x 32 contiguous bytes, the first pass writes its whole tile as one
// contiguous block — and does the levels in place there; the local bit reversal is undone by the index of the store.
// The scaling by 1 / n and the coset factors ride on the load of the first or the store of the last pass.
// Twiddles come from two tables of powers, w^i (i < 2^tw_h) and w^(2^tw_h i), joined by one multiplication when a level needs both halves of the
// exponent (levels with s 2^l >= 2^tw_h need only the second, the last level none).
// Everything but the kernels is plain C++: tests/host/fr_ntt_host.cpp runs the same functions as a serial loop over the lanes.
#pragma once
#include "fr.cuh"

namespace ntt {

constexpr unsigned MAX_LOG_N = 26;
constexpr unsigned TILE_BITS = 10;                      // elements of a workgroup's tile: 2^10 x 32 B = 32 KiB of LDS
constexpr unsigned COL_BITS = 3;                        // columns of a tile: 8 x 32 B = 256 contiguous bytes per global run
constexpr unsigned MAX_LEVELS = TILE_BITS - COL_BITS;   // butterfly levels of one pass
constexpr unsigned THREADS = 256;
constexpr unsigned TILE = 1u << TILE_BITS;

struct Plan {
    unsigned log_n = 0, passes = 1, widest = 0;
    unsigned levels[MAX_LOG_N + 1] = {};
};
// cap: most levels per pass (1 .. MAX_LEVELS).  even: the call is in place — the passes alternate between the caller's vector and the scratch
// vector, so three or more passes must be an even number (one pass holds a whole vector in its tile and may run in place).
inline Plan make_plan(unsigned log_n, unsigned cap, bool even) {
    Plan p;
    p.log_n = log_n;
    cap = cap < 1 ? 1 : cap > MAX_LEVELS ? MAX_LEVELS : cap;
    p.passes = log_n ? (log_n + cap - 1) / cap : 1;
    if (even && p.passes >= 3 && (p.passes & 1)) p.passes++;
    for (unsigned k = 0; k < p.passes; k++) {   // as even as it goes: the first passes take the remainder (a pass of 0 levels is a copy)
        p.levels[k] = log_n / p.passes + (k < log_n % p.passes ? 1u : 0u);
        if (p.levels[k] > p.widest) p.widest = p.levels[k];
    }
    return p;
}

enum { F_NONE = 0, F_CONST = 1, F_TABLE = 2 };
struct Pass {
    const uint32_t* src;
    uint32_t* dst;
    const uint32_t *tw_lo, *tw_hi;   // w^i, i < 2^tw_h; w^(2^tw_h i), i < 2^(tw_bits - tw_h)
    const uint32_t *f_lo, *f_hi;     // factor of element i: f_lo[i mod 2^f_h] f_hi[i >> f_h] (F_TABLE), or f_lo[0] (F_CONST)
    uint32_t log_n, log_s, b, log_ct;
    uint32_t tw_h, tw_bits;          // tw_bits = log2 of the number of twiddles = max(log_n - 1, 0)
    uint32_t f_h;
    uint32_t in_fmt, out_fmt;        // fr::FMT_*
    uint32_t pre, post;              // F_*: factor on the load (by input index) / on the store (by output index)
};
// workgroups of a pass per vector
inline uint64_t tiles_per_vector(const Pass& P) { return (uint64_t)1 << (P.log_n - P.b - P.log_ct); }

// A pair of power tables: lo[i] = scale base^i (i < n_lo = 2^h), hi[i] = hi_base^i (i < n_hi), hi_base = base^(2^h); lo[n_lo] = 1 / n for the
// inverse direction (the constant factor of a plain inverse transform), 1 otherwise.
struct TableSpec {
    fr::Fr base, hi_base, scale, ninv;
    unsigned h;
    uint32_t n_lo, n_hi;
};
// twiddles (coset = false: x is ignored) or the coset factors of the offset x (Montgomery form, non-zero)
inline TableSpec table_spec(bool coset, unsigned log_n, int inverse, const fr::Fr& x) {
    TableSpec t;
    t.ninv = fr::one();
    if (inverse) {
        const fr::Fr two = fr::add(fr::one(), fr::one());
        fr::Fr n = fr::one();
        for (unsigned k = 0; k < log_n; k++) n = fr::mul(n, two);
        t.ninv = fr::inverse(n);
    }
    unsigned bits;   // log2 of the number of powers the two tables span
    if (coset) {
        t.base = inverse ? fr::inverse(x) : x;
        t.scale = t.ninv;
        bits = log_n;
    } else {
        t.base = inverse ? FR_CONST(ROOT_INV) : FR_CONST(ROOT);
        for (unsigned k = log_n; k < (unsigned)frc::TWO_ADICITY; k++) t.base = fr::mul(t.base, t.base);
        t.scale = fr::one();
        bits = log_n ? log_n - 1 : 0;
    }
    t.h = (bits + 1) / 2;
    t.n_lo = 1u << t.h;
    t.n_hi = 1u << (bits - t.h);
    t.hi_base = t.base;
    for (unsigned k = 0; k < t.h; k++) t.hi_base = fr::mul(t.hi_base, t.hi_base);
    return t;
}
FR_HD fr::Fr power_entry(const fr::Fr& base, const fr::Fr& scale, uint32_t i) { return fr::mul(fr::pow_u32(base, i), scale); }

// Pass k of a call: the last pass writes `out`, the ones before it alternate backwards between `scratch` and `out`; the first reads `in`.
// cs_lo == nullptr: no coset.  tw_lo has the 1 / n entry behind its 2^tw_h powers.
inline Pass make_pass(const Plan& plan, unsigned k, unsigned fmt, int inverse, const uint32_t* tw_lo, const uint32_t* tw_hi, unsigned tw_h, const uint32_t* cs_lo,
                      const uint32_t* cs_hi, unsigned cs_h, const uint32_t* in, uint32_t* out, uint32_t* scratch) {
    const bool first = k == 0, last = k + 1 == plan.passes;
    auto dst_of = [&](unsigned q) { return ((plan.passes - 1 - q) & 1) ? scratch : out; };
    Pass P{};
    P.src = first ? in : dst_of(k - 1);
    P.dst = dst_of(k);
    P.tw_lo = tw_lo;
    P.tw_hi = tw_hi;
    P.tw_h = tw_h;
    P.tw_bits = plan.log_n ? plan.log_n - 1 : 0;
    P.log_n = plan.log_n;
    for (unsigned q = 0; q < k; q++) P.log_s += plan.levels[q];
    P.b = plan.levels[k];
    P.log_ct = plan.log_n - P.b < COL_BITS ? plan.log_n - P.b : COL_BITS;
    P.in_fmt = first ? fmt : fr::FMT_RAW;
    P.out_fmt = last ? fmt : fr::FMT_RAW;
    if (cs_lo) {
        P.f_lo = cs_lo;
        P.f_hi = cs_hi;
        P.f_h = cs_h;
        P.pre = first && !inverse ? F_TABLE : F_NONE;
        P.post = last && inverse ? F_TABLE : F_NONE;
    } else if (inverse) {
        P.f_lo = tw_lo + ((size_t)8 << tw_h);
        P.post = last ? F_CONST : F_NONE;
    }
    return P;
}

FR_HD uint32_t bitrev(uint32_t x, uint32_t bits) {
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
    x = (x >> 16) | (x << 16);
    return bits ? x >> (32 - bits) : 0u;
}

// the tile in LDS: eight planes of TILE words (lanes that touch neighbouring elements touch neighbouring banks)
FR_HD fr::Fr tile_get(const uint32_t* lds, uint32_t pos) {
    fr::Fr r;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 8; k++) r.v[k] = lds[k * TILE + pos];
    return r;
}
FR_HD void tile_put(uint32_t* lds, uint32_t pos, const fr::Fr& a) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 8; k++) lds[k * TILE + pos] = a.v[k];
}

FR_HD fr::Fr factor(const Pass& P, uint32_t mode, uint32_t idx) {
    if (mode == F_CONST) return fr::load_words(P.f_lo);
    const fr::Fr lo = fr::load_words(P.f_lo + (size_t)(idx & ((1u << P.f_h) - 1u)) * 8);
    if (P.log_n <= P.f_h) return lo;
    return fr::mul(lo, fr::load_words(P.f_hi + (size_t)(idx >> P.f_h) * 8));
}
// w^e for a level whose exponents are multiples of 2^sh
FR_HD fr::Fr twiddle(const Pass& P, uint32_t e, uint32_t sh) {
    if (sh >= P.tw_h) return fr::load_words(P.tw_hi + (size_t)(e >> P.tw_h) * 8);
    const fr::Fr lo = fr::load_words(P.tw_lo + (size_t)(e & ((1u << P.tw_h) - 1u)) * 8);
    if (P.tw_bits <= P.tw_h) return lo;
    return fr::mul(lo, fr::load_words(P.tw_hi + (size_t)(e >> P.tw_h) * 8));
}

struct TileAt {
    size_t base;     // first element of the tile's vector
    uint32_t col0;   // first column of the tile
};
FR_HD TileAt tile_at(const Pass& P, uint64_t block) {
    const uint32_t tpv = P.log_n - P.b - P.log_ct;
    TileAt t;
    t.base = (size_t)(block >> tpv) << P.log_n;
    t.col0 = (uint32_t)(block & (((uint64_t)1 << tpv) - 1u)) << P.log_ct;
    return t;
}

// global -> tile: local position cc + 2^log_ct j holds in[c + (n / R) j]
FR_HD void pass_load(const Pass& P, uint64_t block, uint32_t tid, uint32_t nthr, uint32_t* lds) {
    const TileAt t = tile_at(P, block);
    const uint32_t log_nc = P.log_n - P.b, cmask = (1u << P.log_ct) - 1u;
    for (uint32_t i = tid; i < (1u << (P.b + P.log_ct)); i += nthr) {
        const uint32_t idx = t.col0 + (i & cmask) + ((i >> P.log_ct) << log_nc);
        fr::Fr x = fr::load(P.src, t.base + idx, P.in_fmt);
        if (P.pre != F_NONE) x = fr::mul(x, factor(P, P.pre, idx));
        tile_put(lds, i, x);
    }
}
// level l of the pass, in place: (a, b) at distance R / 2^(l + 1) -> (a + b, (a - b) w^e)
FR_HD void pass_level(const Pass& P, uint64_t block, uint32_t l, uint32_t tid, uint32_t nthr, uint32_t* lds) {
    const TileAt t = tile_at(P, block);
    const uint32_t half_log = P.b - 1u - l, cmask = (1u << P.log_ct) - 1u;
    const uint32_t log_m = P.log_n - P.log_s - P.b, sh = P.log_s + l;
    const bool last = sh + 1u == P.log_n;   // the last level of the transform: every twiddle is 1
    for (uint32_t i = tid; i < (1u << (P.b - 1u + P.log_ct)); i += nthr) {
        const uint32_t cc = i & cmask, tp = i >> P.log_ct;
        const uint32_t jj = tp & ((1u << half_log) - 1u), j0 = ((tp >> half_log) << (half_log + 1u)) + jj;
        const uint32_t pos0 = cc + (j0 << P.log_ct), pos1 = pos0 + (1u << (half_log + P.log_ct));
        const fr::Fr a = tile_get(lds, pos0), b = tile_get(lds, pos1);
        tile_put(lds, pos0, fr::add(a, b));
        fr::Fr d = fr::sub(a, b);
        if (!last) {
            const uint32_t p = (t.col0 + cc) >> P.log_s;
            d = fr::mul(d, twiddle(P, (p + (jj << log_m)) << sh, sh));
        }
        tile_put(lds, pos1, d);
    }
}
// tile -> global: result k of column c = q + s p sits at the bit-reversed local row and goes to out[q + s (R p + k)]
FR_HD void pass_store(const Pass& P, uint64_t block, uint32_t tid, uint32_t nthr, const uint32_t* lds) {
    const TileAt t = tile_at(P, block);
    const uint32_t cmask = (1u << P.log_ct) - 1u;
    for (uint32_t i = tid; i < (1u << (P.b + P.log_ct)); i += nthr) {
        uint32_t cc, k;
        if (P.log_s == 0) {   // first pass: the tile's results are one contiguous block, k runs fastest
            k = i & ((1u << P.b) - 1u);
            cc = i >> P.b;
        } else {
            cc = i & cmask;
            k = i >> P.log_ct;
        }
        const uint32_t c = t.col0 + cc, q = c & ((1u << P.log_s) - 1u), p = c >> P.log_s;
        const uint32_t out = q + (((p << P.b) + k) << P.log_s);
        fr::Fr x = tile_get(lds, cc + (bitrev(k, P.b) << P.log_ct));
        if (P.post != F_NONE) x = fr::mul(x, factor(P, P.post, out));
        fr::store(P.dst, t.base + out, x, P.out_fmt);
    }
}

enum { OP_MUL = 0, OP_ADD = 1, OP_SUB = 2 };   // MI_FR_MUL / MI_FR_ADD / MI_FR_SUB
FR_HD fr::Fr vec_op(int op, const fr::Fr& a, const fr::Fr& b) { return op == OP_MUL ? fr::mul(a, b) : op == OP_ADD ? fr::add(a, b) : fr::sub(a, b); }

#if defined(__HIPCC__) && !defined(MI_NTT_PLAN_ONLY)   // MI_NTT_PLAN_ONLY: a second translation unit takes the plan, the maps and the tables (g1_ntt.hip)
// one workgroup per tile; block0 + blockIdx.x = vector * tiles per vector + tile (the batch is one more dimension of the same launch)
__global__ __launch_bounds__(THREADS) void k_ntt_pass(const Pass P, const uint64_t block0) {
    __shared__ uint32_t lds[8 * TILE];
    const uint64_t block = block0 + blockIdx.x;
    pass_load(P, block, threadIdx.x, THREADS, lds);
    __syncthreads();
    for (uint32_t l = 0; l < P.b; l++) {
        pass_level(P, block, l, threadIdx.x, THREADS, lds);
        __syncthreads();
    }
    pass_store(P, block, threadIdx.x, THREADS, lds);
}

// out[i] = scale base^i, i < count: the tables of powers (twiddles, coset factors)
__global__ __launch_bounds__(THREADS) void k_fr_powers(uint32_t* out, const fr::Fr base, const fr::Fr scale, const uint32_t count) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= count) return;
    fr::store_words(out + (size_t)i * 8, power_entry(base, scale, i));
}

// out[i] = a[i] op b[i]; out may be a or b (every lane reads its elements before it writes them)
__global__ __launch_bounds__(THREADS) void k_fr_vec_op(const uint32_t* a, const uint32_t* b, uint32_t* out, const size_t n, const int op, const unsigned fmt) {
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * THREADS)
        fr::store(out, i, vec_op(op, fr::load(a, i, fmt), fr::load(b, i, fmt)), fmt);
}
#endif

}  // namespace ntt
