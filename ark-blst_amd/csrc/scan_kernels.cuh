// Running products / sums and batched inversion over Fr (mi_fr_scan, mi_fr_batch_inverse): the level plan, the index maps, the per-lane steps and
// the kernels.  The tile plan is the one of poly_kernels.cuh: a workgroup of 256 lanes owns a tile of T = 2^tile_bits consecutive elements, k = 4
// per lane; level l holds ceil(n / T^l) elements per vector, the levels above the data live in a scratch vector of the context, and the plan stops
// at the first level one tile holds.  A partial last tile is padded with the identity.
//
// Scan (op = MUL or ADD, a template parameter; the multiplier is the data itself):
//   up sweep of level l     reads the level, writes the tile totals = the elements of level l + 1
//   down sweep of level l   reads the level and the EXCLUSIVE prefixes of level l + 1 (the tiles' carry-ins), writes the inclusive or exclusive
//                           prefixes in the place of the level (levels above the data: always exclusive); the top level also writes the total
// A scan is the up sweeps of all levels but the top and the down sweeps from the top: two reads and one write of the data.  A reduction alone is
// the up sweeps of all levels: one read.  Inside a tile: a serial pass over the lane's k elements, a log-step scan over the lanes' totals through
// LDS (step d: x_l = x_(l - d) op x_l) and a second serial pass from the previous lane's prefix; the up sweep, which wants the total alone, halves
// the lanes' totals instead (step h = 128 .. 1: x_l = x_l op x_(l + h) for l < h), so that whole waves drop out after the first two steps.
//
// Inversion (Montgomery's trick as a tree).  Level 0 is `a` with every zero replaced by one; level l + 1 holds the tile products of level l.
//   up sweep of level l     the scan's up sweep with op = MUL (level 0: zeros read as one); the data itself stays as it is
//   down sweep of level l   gets, per tile, the inverse I_t of the tile's product — element t of the already inverted level l + 1; the top level
//                           inverts its own product, one lane (scan::inverse), broadcast through LDS — and writes 1 / e_i = I_t x (product of the other
//                           elements of the tile) in the place of e_i: lane products x_l, an inclusive prefix scan P and an inclusive suffix
//                           scan S over the lanes in the same barrier steps, 1 / x_l = I_t P_(l-1) S_(l+1), then Montgomery's trick over the
//                           lane's k elements.  Level 0 writes zero for a zero, multiplies num[i] in, converts to the caller's format and counts
//                           the zeros (one atomic addition per workgroup).
// There is no host round trip between the launches of a call.
// Everything but the kernels is plain C++: tests/host/fr_scan_host.cpp runs the same functions as a serial loop over the lanes.
#pragma once
#include "poly_kernels.cuh"   // the tile plan (poly::Plan, make_plan, lane_bits) and the LDS planes (scan_get / scan_put)

namespace scan {

using fr::Fr;
using poly::LANE_BITS;
using poly::LANE_ELEMS;
using poly::MAX_N;
using poly::MIN_TILE_BITS;
using poly::Plan;
using poly::scan_get;
using poly::scan_put;
using poly::THREADS;
using poly::TILE_BITS;

constexpr int OP_MUL = 0, OP_ADD = 1;   // MI_FR_MUL / MI_FR_ADD

template <int OP>
FR_HD Fr identity() {
    if (OP == OP_MUL) return fr::one();
    return fr::zero();
}
template <int OP>
FR_HD Fr combine(const Fr& a, const Fr& b) {
    if (OP == OP_MUL) return fr::mul(a, b);
    return fr::add(a, b);
}

struct Level {
    const uint32_t* src;     // the level: one vector of m elements per vector of the batch
    const uint32_t* num;     // inversion, down sweep of level 0: the numerators, in the shape of src (nullptr: none)
    uint32_t* dst;           // up: the tile totals, `tiles` per vector; down: the results, in the shape of src (may be src, or num)
    const uint32_t* carry;   // down: the level above after its own down sweep, `tiles` per vector (nullptr: the top level)
    uint32_t* vals;          // scan, down sweep of the top level: the total per vector (nullptr: not wanted)
    unsigned long long* zeros;   // inversion, down sweep of level 0: the count of zeros
    uint64_t m, tiles;
    uint32_t tile_bits;
    uint32_t in_fmt, out_fmt, val_fmt;   // fr::FMT_*
    uint32_t exclusive;      // scan, down: element i of the output leaves i itself out
    uint32_t zero_as_one;    // inversion, level 0: a zero is read as one
};

inline Level make_level(const Plan& pl, unsigned l, unsigned fmt, const uint32_t* in, uint32_t* scratch) {
    Level P{};
    P.src = l ? scratch + pl.off[l] * 8 : in;
    P.m = pl.m[l];
    P.tiles = pl.m[l + 1];
    P.tile_bits = pl.tile_bits;
    P.in_fmt = l ? fr::FMT_RAW : fmt;
    P.out_fmt = fr::FMT_RAW;
    P.val_fmt = fmt;
    return P;
}
// vals != nullptr: a reduction alone, whose top level writes the vectors' totals there.  invert: the up sweep of an inversion.
inline Level make_up(const Plan& pl, unsigned l, unsigned fmt, const uint32_t* in, uint32_t* scratch, uint32_t* vals, bool invert) {
    Level P = make_level(pl, l, fmt, in, scratch);
    const bool to_vals = vals && l + 1 == pl.levels;
    P.dst = to_vals ? vals : scratch + pl.off[l + 1] * 8;
    P.out_fmt = to_vals ? fmt : fr::FMT_RAW;
    P.zero_as_one = invert && l == 0;
    return P;
}
inline Level make_scan_down(const Plan& pl, unsigned l, unsigned fmt, const uint32_t* in, uint32_t* out, uint32_t* scratch, uint32_t* vals, bool exclusive) {
    Level P = make_level(pl, l, fmt, in, scratch);
    const bool top = l + 1 == pl.levels;
    P.dst = l ? scratch + pl.off[l] * 8 : out;
    P.out_fmt = l ? fr::FMT_RAW : fmt;
    P.carry = top ? nullptr : scratch + pl.off[l + 1] * 8;
    P.vals = top ? vals : nullptr;
    P.exclusive = l ? 1u : (exclusive ? 1u : 0u);
    return P;
}
inline Level make_inv_down(const Plan& pl, unsigned l, unsigned fmt, const uint32_t* a, const uint32_t* num, uint32_t* out, uint32_t* scratch,
                           unsigned long long* zeros) {
    Level P = make_level(pl, l, fmt, a, scratch);
    const bool top = l + 1 == pl.levels;
    P.dst = l ? scratch + pl.off[l] * 8 : out;
    P.out_fmt = l ? fr::FMT_RAW : fmt;
    P.carry = top ? nullptr : scratch + pl.off[l + 1] * 8;
    P.num = l ? nullptr : num;
    P.zeros = l ? nullptr : zeros;
    P.zero_as_one = l == 0;
    return P;
}
inline uint64_t blocks_of(const Level& P, uint64_t batch) { return batch * P.tiles; }

struct TileAt {
    uint64_t vec, block;
    uint64_t base;    // first element of the vector
    uint64_t first;   // first element of the tile in that vector
};
FR_HD TileAt tile_at(const Level& P, uint64_t block) {
    TileAt t;
    t.block = block;
    t.vec = block / P.tiles;
    t.base = t.vec * P.m;
    t.first = (block - t.vec * P.tiles) << P.tile_bits;
    return t;
}
template <int OP>
FR_HD Fr carry_in(const Level& P, const TileAt& t) { return P.carry ? fr::load_words(P.carry + (size_t)t.block * 8) : identity<OP>(); }

// first pass: the lane's K elements (the identity behind the vector's end; a zero as one where the level says so, remembered in zmask) and
// their total
template <int OP, unsigned K>
FR_HD Fr lane_total(const Level& P, const TileAt& t, uint32_t lane, Fr (&p)[K], uint32_t& zmask) {
    const uint64_t i0 = t.first + (uint64_t)lane * K;
    zmask = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (unsigned j = 0; j < K; j++) {
        p[j] = i0 + j < P.m ? fr::load(P.src, (size_t)(t.base + i0 + j), P.in_fmt) : identity<OP>();
        if (P.zero_as_one && fr::is_zero(p[j])) {
            zmask |= 1u << j;
            p[j] = fr::one();
        }
    }
    Fr acc = p[0];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (unsigned j = 1; j < K; j++) acc = combine<OP>(acc, p[j]);
    return acc;
}
// one step of the inclusive prefix scan over the lanes, x_l = x_(l - d) op x_l, and of the suffix scan, x_l = x_l op x_(l + d); st holds every
// lane's x of the step before
template <int OP>
FR_HD Fr prefix_step(const uint32_t* st, uint32_t lane, uint32_t d, const Fr& x) { return lane >= d ? combine<OP>(scan_get(st, lane - d), x) : x; }
template <int OP>
FR_HD Fr suffix_step(const uint32_t* st, uint32_t lane, uint32_t lanes, uint32_t d, const Fr& x) {
    return lane + d < lanes ? combine<OP>(x, scan_get(st, lane + d)) : x;
}
// one step of the tile's reduction: lane l < h takes lane l + h in (readers and writers of a step touch different halves: one copy suffices)
template <int OP>
FR_HD Fr reduce_step(const uint32_t* st, uint32_t lane, uint32_t h, const Fr& x) { return combine<OP>(x, scan_get(st, lane + h)); }
// what enters the lane from below: the tile's carry-in and the previous lane's inclusive prefix
template <int OP>
FR_HD Fr lane_carry(const uint32_t* st, uint32_t lane, const Fr& cin) { return lane ? combine<OP>(cin, scan_get(st, lane - 1)) : cin; }
// second pass of the scan: y = the prefix of everything before the lane's first element
template <int OP, unsigned K>
FR_HD void lane_finish(const Level& P, const TileAt& t, uint32_t lane, const Fr (&p)[K], Fr y) {
    const uint64_t i0 = t.first + (uint64_t)lane * K;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (unsigned j = 0; j < K; j++) {
        Fr next = y;
        if (j + 1 < K || !P.exclusive) next = combine<OP>(y, p[j]);
        if (i0 + j < P.m) fr::store(P.dst, (size_t)(t.base + i0 + j), P.exclusive ? y : next, P.out_fmt);
        y = next;
    }
}
// lane 0 after the reduction holds the tile's total
FR_HD void put_total(const Level& P, const TileAt& t, const Fr& x) { fr::store(P.dst, (size_t)t.block, x, P.out_fmt); }
FR_HD void put_value(const Level& P, const TileAt& t, const Fr& x) {
    if (P.vals) fr::store(P.vals, (size_t)t.vec, x, P.val_fmt);
}

// 256-bit helpers of the inversion below (plain integers, no reduction)
FR_HD Fr modulus() {
    return Fr{{fp28c::FR_MOD[0], fp28c::FR_MOD[1], fp28c::FR_MOD[2], fp28c::FR_MOD[3], fp28c::FR_MOD[4], fp28c::FR_MOD[5], fp28c::FR_MOD[6], fp28c::FR_MOD[7]}};
}
FR_HD Fr shr1(const Fr& a) {
    Fr r;
    for (int k = 0; k < 7; k++) r.v[k] = (a.v[k] >> 1) | (a.v[k + 1] << 31);
    r.v[7] = a.v[7] >> 1;
    return r;
}
FR_HD Fr shl1(const Fr& a) {   // a < 2^255
    Fr r;
    for (int k = 7; k > 0; k--) r.v[k] = (a.v[k] << 1) | (a.v[k - 1] >> 31);
    r.v[0] = a.v[0] << 1;
    return r;
}
FR_HD Fr add_raw(const Fr& a, const Fr& b) {   // a + b < 2^256
    Fr r;
    uint64_t c = 0;
    for (int k = 0; k < 8; k++) {
        c += (uint64_t)a.v[k] + b.v[k];
        r.v[k] = (uint32_t)c;
        c >>= 32;
    }
    return r;
}
FR_HD Fr sub_raw(const Fr& a, const Fr& b) {   // a >= b
    Fr r;
    uint64_t borrow = 0;
    for (int k = 0; k < 8; k++) {
        const uint64_t x = (uint64_t)a.v[k] - b.v[k] - borrow;
        r.v[k] = (uint32_t)x;
        borrow = (x >> 32) & 1;
    }
    return r;
}
// 1 / a for a Montgomery value a != 0 below r: the one inversion of a call, on one lane of the top level's workgroup.  Kaliski's almost inverse
// (binary Euclid: u x_s + v x_r = r throughout, x_r and x_s below 2r < 2^256) gives x = a^-1 2^k mod r with 255 <= k <= 510 in k steps of
// shifts and subtractions; a = A R stands for A, and A^-1 R = a^-1 R^2 = x 2^(512 - k): that many doublings modulo r.  About 400 short
// steps where a^(r - 2) takes 380 multiplications one after the other on the one lane (measured: 0.57 ms per call).
FR_HD Fr inverse(const Fr& a) {
    Fr u = modulus(), v = a, xr = fr::zero(), xs = fr::zero();
    xs.v[0] = 1;
    uint32_t k = 0;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (; !fr::is_zero(v) && k < 512; k++) {
        if ((u.v[0] & 1u) == 0) {
            u = shr1(u);
            xs = shl1(xs);
        } else if ((v.v[0] & 1u) == 0) {
            v = shr1(v);
            xr = shl1(xr);
        } else if (fr::less(v, u)) {
            u = shr1(sub_raw(u, v));
            xr = add_raw(xr, xs);
            xs = shl1(xs);
        } else {
            v = shr1(sub_raw(v, u));
            xs = add_raw(xs, xr);
            xr = shl1(xr);
        }
    }
    if (!fr::less(xr, modulus())) xr = sub_raw(xr, modulus());
    Fr x = sub_raw(modulus(), xr);   // a^-1 2^k mod r (xr != 0 for a != 0)
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (; k < 512; k++) x = fr::add(x, x);
    return x;
}

// the inversion's second pass.  inv = 1 / (the tile's product); stp / sts hold every lane's inclusive prefix and suffix product; e the lane's
// elements as lane_total left them.  1 / x_l = inv P_(l-1) S_(l+1), then from the back: 1 / e_j = (1 / (e_0 .. e_j)) (e_0 .. e_(j-1)).
template <unsigned K>
FR_HD void lane_invert(const Level& P, const TileAt& t, uint32_t lane, uint32_t lanes, const Fr (&e)[K], uint32_t zmask, const Fr& inv, const uint32_t* stp,
                       const uint32_t* sts) {
    const uint64_t i0 = t.first + (uint64_t)lane * K;
    Fr ix = inv;
    if (lane) ix = fr::mul(ix, scan_get(stp, lane - 1));
    if (lane + 1 < lanes) ix = fr::mul(ix, scan_get(sts, lane + 1));
    Fr q[K];   // q[j] = e_0 .. e_j
    q[0] = e[0];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (unsigned j = 1; j + 1 < K; j++) q[j] = fr::mul(q[j - 1], e[j]);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (unsigned j = K; j-- > 0;) {
        Fr v = j ? fr::mul(ix, q[j - 1]) : ix;
        if (j) ix = fr::mul(ix, e[j]);
        if (i0 + j < P.m) {
            if ((zmask >> j) & 1u) v = fr::zero();
            if (P.num) v = fr::mul(v, fr::load(P.num, (size_t)(t.base + i0 + j), P.in_fmt));
            fr::store(P.dst, (size_t)(t.base + i0 + j), v, P.out_fmt);
        }
    }
}
FR_HD uint32_t zeros_of(uint32_t zmask) {
    uint32_t c = 0;
    for (; zmask; zmask &= zmask - 1) c++;
    return c;
}

#if defined(__HIPCC__)
// The first two phases of a tile in the scan's down sweep: totals, scan, and what is left in LDS for lane_carry.  Lanes behind `lanes` (a
// reduced tile) only keep the barriers company.  Returns the lane's inclusive prefix; *st is the storage that holds every lane's.
template <int OP, unsigned K>
__device__ __forceinline__ Fr tile_scan(const Level& P, const TileAt& t, const uint32_t lane, const uint32_t lanes, Fr (&p)[K], uint32_t (&lds)[2][8 * THREADS],
                                        const uint32_t** st) {
    Fr x = identity<OP>();
    uint32_t zmask;
    if (lane < lanes) {
        x = lane_total<OP, K>(P, t, lane, p, zmask);
        scan_put(lds[0], lane, x);
    }
    __syncthreads();
    uint32_t buf = 0;
    for (uint32_t d = 1; d < lanes; d <<= 1) {
        if (lane < lanes) {
            x = prefix_step<OP>(lds[buf], lane, d, x);
            scan_put(lds[buf ^ 1u], lane, x);
        }
        buf ^= 1u;
        __syncthreads();
    }
    *st = lds[buf];
    return x;
}

// one workgroup per tile; block0 + blockIdx.x = vector * tiles + tile (the batch is one more dimension of the same launch)
// The up sweep wants the tile's total alone: a reduction through one copy of the planes, in which whole waves drop out after the first steps.
template <int OP, unsigned K>
__global__ __launch_bounds__(THREADS) void k_scan_up(const Level P, const uint64_t block0) {
    __shared__ uint32_t lds[8 * THREADS];
    const TileAt t = tile_at(P, block0 + blockIdx.x);
    const uint32_t lane = threadIdx.x, lanes = 1u << (P.tile_bits - (K == 1 ? 0 : LANE_BITS));
    Fr p[K];
    Fr x = identity<OP>();
    uint32_t zmask;
    if (lane < lanes) {
        x = lane_total<OP, K>(P, t, lane, p, zmask);
        scan_put(lds, lane, x);
    }
    __syncthreads();
    for (uint32_t h = lanes >> 1; h; h >>= 1) {
        if (lane < h) {
            x = reduce_step<OP>(lds, lane, h, x);
            scan_put(lds, lane, x);
        }
        __syncthreads();
    }
    if (lane == 0) put_total(P, t, x);
}
template <int OP, unsigned K>
__global__ __launch_bounds__(THREADS) void k_scan_down(const Level P, const uint64_t block0) {
    __shared__ uint32_t lds[2][8 * THREADS];
    const TileAt t = tile_at(P, block0 + blockIdx.x);
    const uint32_t lanes = 1u << (P.tile_bits - (K == 1 ? 0 : LANE_BITS));
    Fr p[K];
    const uint32_t* st;
    const Fr x = tile_scan<OP, K>(P, t, threadIdx.x, lanes, p, lds, &st);
    if (threadIdx.x >= lanes) return;
    if (threadIdx.x + 1 == lanes) put_value(P, t, x);   // the top level: one tile per vector, no carry-in
    lane_finish<OP, K>(P, t, threadIdx.x, p, lane_carry<OP>(st, threadIdx.x, carry_in<OP>(P, t)));
}
// TOP: the level one tile holds; its product is inverted here
template <unsigned K, bool TOP>
__global__ __launch_bounds__(THREADS) void k_inv_down(const Level P, const uint64_t block0) {
    __shared__ uint32_t lds[2][2][8 * THREADS];   // [buffer][prefix, suffix]
    const TileAt t = tile_at(P, block0 + blockIdx.x);
    const uint32_t lane = threadIdx.x, lanes = 1u << (P.tile_bits - (K == 1 ? 0 : LANE_BITS));
    Fr e[K];
    Fr pre = fr::one(), suf = pre;
    uint32_t zmask = 0;
    if (lane < lanes) {
        pre = suf = lane_total<OP_MUL, K>(P, t, lane, e, zmask);
        scan_put(lds[0][0], lane, pre);
        scan_put(lds[0][1], lane, pre);
    }
    __syncthreads();
    uint32_t buf = 0;
    for (uint32_t d = 1; d < lanes; d <<= 1) {
        if (lane < lanes) {
            pre = prefix_step<OP_MUL>(lds[buf][0], lane, d, pre);
            suf = suffix_step<OP_MUL>(lds[buf][1], lane, lanes, d, suf);
            scan_put(lds[buf ^ 1u][0], lane, pre);
            scan_put(lds[buf ^ 1u][1], lane, suf);
        }
        buf ^= 1u;
        __syncthreads();
    }
    // lds[buf] holds every lane's prefix and suffix; the other buffer is free: the broadcast of the inverse, the waves' zero counts
    uint32_t* spare = lds[buf ^ 1u][0];
    Fr inv;
    if (TOP) {
        if (lane + 1 == lanes) scan_put(spare, 0, inverse(pre));
    } else {
        inv = fr::load_words(P.carry + (size_t)t.block * 8);
    }
    if (P.zeros) {   // each wave counts its zeros, lane 0 adds the workgroup's count to the call's counter
        uint32_t c = zeros_of(zmask);
        for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
        if ((lane & 63u) == 0) spare[8 * THREADS - 4 + (lane >> 6)] = c;
    }
    if (TOP || P.zeros) __syncthreads();
    if (TOP) inv = scan_get(spare, 0);
    if (P.zeros && lane == 0) {
        const uint32_t c = spare[8 * THREADS - 4] + spare[8 * THREADS - 3] + spare[8 * THREADS - 2] + spare[8 * THREADS - 1];
        if (c) atomicAdd(P.zeros, (unsigned long long)c);
    }
    if (lane >= lanes) return;
    lane_invert<K>(P, t, lane, lanes, e, zmask, inv, lds[buf][0], lds[buf][1]);
}
#endif

}  // namespace scan
