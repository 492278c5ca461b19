// Opening a polynomial over Fr at a point (mi_fr_poly_open): the value p(z) and the quotient (p(X) - p(z)) / (X - z), as a multi-level suffix
// scan.  The level plan, the index maps, the per-lane steps and the kernels.
//
// The serial recurrence (ark-poly's division by a linear factor, DensePolynomial::evaluate): S_n = 0, S_i = p_i + z S_(i+1); q_i = S_(i+1),
// p(z) = S_0.  S_i = sum_(j >= i) p_j z^(j - i) is a suffix sum whose multiplier over a segment of length L is the constant z^L, so it is a scan:
// a tile of T = 2^tile_bits consecutive coefficients belongs to one workgroup, tile t has the local suffixes L_i = sum_(i <= j < end) p_j z^(j - i),
// its total A_t = L_(tT) and its carry C_t = S_(tT), with C_t = A_t + z^T C_(t+1) and S_i = L_i + z^((t + 1) T - i) C_(t+1).  The carries are the
// same problem on the vector A at the point z^T: level l holds ceil(n / T^l) elements per polynomial and is opened at z^(T^l); the plan stops at
// the first level one tile holds.  Every level stores the EXCLUSIVE suffixes E_i = S_(i+1) in the place of its elements: for level 0 that is the
// quotient (element n - 1 = S_n = 0), for a level above it E_t is the carry-in C_(t+1) of tile t of the level below.
//   up sweep of level l     reads the level, writes the tile totals = the elements of level l + 1
//   down sweep of level l   reads the level and E of level l + 1, writes E of level l (the top level also S_0 = p(z))
// An opening is the up sweeps of all levels but the top and the down sweeps from the top: two reads and one write of the data.  An evaluation
// alone is the up sweeps of all levels: one read.
// Inside a tile a lane owns k = 2^lane_bits consecutive elements: a serial Horner pass over them (the last lane takes the tile's carry-in in as
// z^k C), a log-step scan over the lanes' totals through LDS (step d: x_l += z^(k d) x_(l + d), a multiplier every lane shares), and for the down
// sweep a second serial pass from the next lane's suffix.  Every multiplier is z^(2^s) for some s: one small table per point.
// Everything but the kernels is plain C++: tests/host/fr_poly_host.cpp runs the same functions as a serial loop over the lanes.
#pragma once
#include "fr.cuh"

namespace poly {

constexpr unsigned MAX_LOG_N = 26;
constexpr uint64_t MAX_N = (uint64_t)1 << MAX_LOG_N;
constexpr unsigned THREADS = 256;
constexpr unsigned TILE_BITS = 10;        // elements of a workgroup's tile: 2^10, four per lane
constexpr unsigned LANE_BITS = 2;
constexpr unsigned LANE_ELEMS = 1u << LANE_BITS;
constexpr unsigned MIN_TILE_BITS = 2;     // the test build's switch goes down to tiles of four elements
constexpr unsigned MAX_LEVELS = 13;       // tile_bits = 2 at 2^26 elements
constexpr unsigned POW_SLOTS = 40;        // z^(2^s), s < tile_bits x levels <= 26 + tile_bits

// elements per lane: 2^LANE_BITS at a tile of more than THREADS elements, one below it (reduced tiles of the test build)
inline unsigned lane_bits(unsigned tile_bits) { return tile_bits > 8 ? LANE_BITS : 0; }

struct Plan {
    unsigned tile_bits = TILE_BITS, levels = 1;
    uint64_t m[MAX_LEVELS + 1] = {};     // elements of one polynomial at level l; m[l + 1] = tiles of level l; m[levels] = 1, the polynomial's total
    uint64_t off[MAX_LEVELS + 1] = {};   // first element of level l >= 1 in the scratch vector (the polynomials of a level back to back)
    uint64_t scratch = 0;                // elements of the scratch vector
};
// n >= 1 coefficients per polynomial
inline Plan make_plan(uint64_t n, uint64_t batch, unsigned tile_bits) {
    Plan p;
    p.tile_bits = tile_bits < MIN_TILE_BITS ? MIN_TILE_BITS : tile_bits > TILE_BITS ? TILE_BITS : tile_bits;
    const uint64_t T = (uint64_t)1 << p.tile_bits;
    p.m[0] = n;
    while (p.m[p.levels - 1] > T) {
        p.m[p.levels] = (p.m[p.levels - 1] + T - 1) >> p.tile_bits;
        p.levels++;
    }
    p.m[p.levels] = 1;
    for (unsigned l = 1; l <= p.levels; l++) {
        p.off[l] = p.scratch;
        p.scratch += batch * p.m[l];
    }
    return p;
}

struct Level {
    const uint32_t* src;     // the level: one vector of m elements per polynomial
    uint32_t* dst;           // up: the tile totals, `tiles` per polynomial; down: the exclusive suffixes, in the shape of src (may be src)
    const uint32_t* carry;   // down: the exclusive suffixes of the level above, `tiles` per polynomial (nullptr: the top level)
    uint32_t* vals;          // down, top level: S_0 = p(z) per polynomial (nullptr: not wanted)
    const uint32_t* pows;    // z^(2^s), s < POW_SLOTS, of the point (or of every polynomial's point)
    uint64_t m, tiles;
    uint32_t tile_bits, s0;  // the level's point is z^(2^s0)
    uint32_t pow_stride;     // words between the tables of two polynomials (0: one point for all)
    uint32_t in_fmt, out_fmt, val_fmt;   // fr::FMT_*
};

inline Level make_level(const Plan& pl, unsigned l, unsigned fmt, const uint32_t* in, uint32_t* scratch, const uint32_t* pows, bool per_poly) {
    Level P{};
    P.src = l ? scratch + pl.off[l] * 8 : in;
    P.pows = pows;
    P.m = pl.m[l];
    P.tiles = pl.m[l + 1];
    P.tile_bits = pl.tile_bits;
    P.s0 = pl.tile_bits * l;
    P.pow_stride = per_poly ? POW_SLOTS * 8 : 0;
    P.in_fmt = l ? fr::FMT_RAW : fmt;
    P.out_fmt = fr::FMT_RAW;
    P.val_fmt = fmt;
    return P;
}
// vals != nullptr: an evaluation alone, whose top level writes the polynomials' totals as the values
inline Level make_up(const Plan& pl, unsigned l, unsigned fmt, const uint32_t* in, uint32_t* scratch, const uint32_t* pows, bool per_poly, uint32_t* vals) {
    Level P = make_level(pl, l, fmt, in, scratch, pows, per_poly);
    const bool to_vals = vals && l + 1 == pl.levels;
    P.dst = to_vals ? vals : scratch + pl.off[l + 1] * 8;
    P.out_fmt = to_vals ? fmt : fr::FMT_RAW;
    return P;
}
inline Level make_down(const Plan& pl, unsigned l, unsigned fmt, const uint32_t* in, uint32_t* out, uint32_t* scratch, const uint32_t* pows, bool per_poly,
                       uint32_t* vals) {
    Level P = make_level(pl, l, fmt, in, scratch, pows, per_poly);
    const bool top = l + 1 == pl.levels;
    P.dst = l ? scratch + pl.off[l] * 8 : out;
    P.out_fmt = l ? fr::FMT_RAW : fmt;
    P.carry = top ? nullptr : scratch + pl.off[l + 1] * 8;
    P.vals = top ? vals : nullptr;
    return P;
}
// the table of one point: out[s] = z^(2^s) for s < tile_bits x levels, what the plan's levels and their scan steps multiply by; zero behind
inline void point_powers(uint32_t* out, const Plan& pl, fr::Fr z) {
    const unsigned slots = pl.tile_bits * pl.levels;
    for (unsigned s = 0; s < POW_SLOTS; s++) {
        fr::store_words(out + (size_t)s * 8, s < slots ? z : fr::zero());
        if (s + 1 < slots) z = fr::mul(z, z);
    }
}
inline uint64_t blocks_of(const Level& P, uint64_t batch) { return batch * P.tiles; }

struct TileAt {
    uint64_t poly, block;
    uint64_t base;         // first element of the polynomial's vector
    uint64_t first;        // first element of the tile in that vector
    const uint32_t* pw;    // the table of the polynomial's point
};
FR_HD TileAt tile_at(const Level& P, uint64_t block) {
    TileAt t;
    t.block = block;
    t.poly = block / P.tiles;
    t.base = t.poly * P.m;
    t.first = (block - t.poly * P.tiles) << P.tile_bits;
    t.pw = P.pows + (size_t)t.poly * P.pow_stride;
    return t;
}
FR_HD fr::Fr power(const TileAt& t, uint32_t s) { return fr::load_words(t.pw + (size_t)s * 8); }
FR_HD fr::Fr carry_in(const Level& P, const TileAt& t) { return P.carry ? fr::load_words(P.carry + (size_t)t.block * 8) : fr::zero(); }

// the scan's storage: eight planes of THREADS words (lanes that touch neighbouring elements touch neighbouring banks)
FR_HD fr::Fr scan_get(const uint32_t* st, uint32_t lane) {
    fr::Fr r;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 8; k++) r.v[k] = st[k * THREADS + lane];
    return r;
}
FR_HD void scan_put(uint32_t* st, uint32_t lane, const fr::Fr& a) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 8; k++) st[k * THREADS + lane] = a.v[k];
}

// first pass: the lane's K elements (zero behind the vector's end) and their Horner total sum_j p_j z^j; cin: the tile's carry-in, which the last
// lane takes in as z^K C (zk = z^K), or nullptr (up sweep)
template <unsigned K>
FR_HD fr::Fr lane_total(const Level& P, const TileAt& t, uint32_t lane, uint32_t lanes, fr::Fr (&p)[K], const fr::Fr& z, const fr::Fr& zk, const fr::Fr* cin) {
    const uint64_t i0 = t.first + (uint64_t)lane * K;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (unsigned j = 0; j < K; j++) p[j] = i0 + j < P.m ? fr::load(P.src, (size_t)(t.base + i0 + j), P.in_fmt) : fr::zero();
    fr::Fr acc = p[K - 1];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (unsigned j = K - 1; j-- > 0;) acc = fr::add(fr::mul(acc, z), p[j]);
    if (cin && lane + 1 == lanes) acc = fr::add(acc, fr::mul(zk, *cin));
    return acc;
}
// one step of the scan over the lanes: x_l += mult x_(l + d), mult = z^(K d); st holds every lane's x of the step before
FR_HD fr::Fr scan_step(const uint32_t* st, uint32_t lane, uint32_t lanes, uint32_t d, const fr::Fr& mult, const fr::Fr& x) {
    return lane + d < lanes ? fr::add(x, fr::mul(mult, scan_get(st, lane + d))) : x;
}
// what enters the lane from above, S at the next lane's first element: its x after the last step, or the tile's carry-in
FR_HD fr::Fr lane_carry(const uint32_t* st, uint32_t lane, uint32_t lanes, const fr::Fr& cin) { return lane + 1 < lanes ? scan_get(st, lane + 1) : cin; }
// second pass: element i of the output is S_(i+1); y = S at the element behind the lane's last
template <unsigned K>
FR_HD void lane_finish(const Level& P, const TileAt& t, uint32_t lane, const fr::Fr (&p)[K], const fr::Fr& z, fr::Fr y) {
    const uint64_t i0 = t.first + (uint64_t)lane * K;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (unsigned j = K; j-- > 0;) {
        if (i0 + j < P.m) fr::store(P.dst, (size_t)(t.base + i0 + j), y, P.out_fmt);
        if (j) y = fr::add(fr::mul(y, z), p[j]);
    }
}
// lane 0 after the scan holds the tile's total (up) or S at the tile's first element (down: p(z) at the top level)
FR_HD void put_total(const Level& P, const TileAt& t, const fr::Fr& x) { fr::store(P.dst, (size_t)t.block, x, P.out_fmt); }
FR_HD void put_value(const Level& P, const TileAt& t, const fr::Fr& x) {
    if (P.vals) fr::store(P.vals, (size_t)t.poly, x, P.val_fmt);
}

#if defined(__HIPCC__)
// The three phases of a tile, shared by the two sweeps: totals, scan, and what is left in LDS for lane_carry.  Lanes behind `lanes` (a reduced
// tile) only keep the barriers company.  Returns the lane's x; *st is the storage that holds every lane's.
template <unsigned K>
__device__ __forceinline__ fr::Fr tile_scan(const Level& P, const TileAt& t, const uint32_t lane, const uint32_t lanes, fr::Fr (&p)[K], const fr::Fr& z,
                                            const fr::Fr* cin, uint32_t (&lds)[2][8 * THREADS], const uint32_t** st) {
    const uint32_t kb = K == 1 ? 0 : LANE_BITS;
    fr::Fr x = fr::zero();
    if (lane < lanes) {
        x = lane_total<K>(P, t, lane, lanes, p, z, power(t, P.s0 + kb), cin);
        scan_put(lds[0], lane, x);
    }
    __syncthreads();
    uint32_t buf = 0;
    for (uint32_t j = 0; (1u << j) < lanes; j++) {
        if (lane < lanes) {
            x = scan_step(lds[buf], lane, lanes, 1u << j, power(t, P.s0 + kb + j), x);
            scan_put(lds[buf ^ 1u], lane, x);
        }
        buf ^= 1u;
        __syncthreads();
    }
    *st = lds[buf];
    return x;
}

// one workgroup per tile; block0 + blockIdx.x = polynomial * tiles + tile (the batch is one more dimension of the same launch)
template <unsigned K>
__global__ __launch_bounds__(THREADS) void k_poly_up(const Level P, const uint64_t block0) {
    __shared__ uint32_t lds[2][8 * THREADS];
    const TileAt t = tile_at(P, block0 + blockIdx.x);
    const uint32_t lanes = 1u << (P.tile_bits - (K == 1 ? 0 : LANE_BITS));
    const fr::Fr z = power(t, P.s0);
    fr::Fr p[K];
    const uint32_t* st;
    const fr::Fr x = tile_scan<K>(P, t, threadIdx.x, lanes, p, z, nullptr, lds, &st);
    if (threadIdx.x == 0) put_total(P, t, x);
}
template <unsigned K>
__global__ __launch_bounds__(THREADS) void k_poly_down(const Level P, const uint64_t block0) {
    __shared__ uint32_t lds[2][8 * THREADS];
    const TileAt t = tile_at(P, block0 + blockIdx.x);
    const uint32_t lanes = 1u << (P.tile_bits - (K == 1 ? 0 : LANE_BITS));
    const fr::Fr z = power(t, P.s0), cin = carry_in(P, t);
    fr::Fr p[K];
    const uint32_t* st;
    const fr::Fr x = tile_scan<K>(P, t, threadIdx.x, lanes, p, z, &cin, lds, &st);
    if (threadIdx.x >= lanes) return;
    if (threadIdx.x == 0) put_value(P, t, x);
    lane_finish<K>(P, t, threadIdx.x, p, z, lane_carry(st, threadIdx.x, lanes, cin));
}
#endif

}  // namespace poly
