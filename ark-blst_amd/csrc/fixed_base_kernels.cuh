// Kernels of the fixed-base batch multiplication out[i] = s_i P (mi_g{1,2}_batch_mul; ark_ec FixedBase::msm + normalize_batch over the
// reference's groups, src/g1.rs:593-600, src/g2.rs:573-580).  Not the Pippenger pipeline: no sort, no buckets, no reduction.
//
//   table   T[j][m - 1] = m 2^(w j) P, j < W = fbm::windows(w), 1 <= m <= 2^(w-1), affine in the device form k_accumulate gathers from
//           (an entry at infinity — a base of small order has many — carries the per-point infinity flag in the last word of its y slot):
//     k_fb_bases   one lane: the window bases 2^(w j) P by w doublings each, projective
//     k_fb_level   level k = 0 .. w - 2: (2^k + u) B = u B + 2^k B for 1 <= u <= 2^k — ONE complete addition per entry, W 2^k lanes
//     k_fb_vals    Z of every entry for the shared inversion (an entry at infinity is kept out of it and flagged)
//     (the product tree k_norm_up / k_norm_down of normalize_batch, then k_table_affine)
//   walk    k_fb_walk (G1: one lane per scalar) / k_fb_walk_g2_coop (G2: a lane pair per scalar, CoopF2A as in k_accumulate_g2_coop): the
//           lane recodes its scalar into signed w-bit digits and adds the entry of every non-zero digit, XYZZ mixed additions; a lane that
//           meets an exceptional pair finishes its remaining windows with complete additions.  The sum leaves as a Jacobian point in the
//           reference's form, which normalize_batch's kernels turn into affine points with ONE inversion per pass.
// Launch-bounds rule of curve_kernels.cuh: every kernel here contains calls and is built for two waves per SIMD.
#pragma once
#include "curve_kernels.cuh"

namespace msmk {

constexpr uint32_t FB_NONE = 0xffffffffu;

// One step of the signed recoding of for_each_digit (kernels_common.cuh), resumable: the digit of window `win` of the integer s as
// (table entry | sign << 31), entry = win 2^(c-1) + |d| - 1, or FB_NONE for a zero digit.  `carry` travels from window to window.
__device__ __forceinline__ uint32_t fb_digit(const uint32_t (&s)[8], uint32_t win, uint32_t c, uint32_t& carry) {
    const uint32_t raw = scalar_bits(s, win * c, c) + carry, half = 1u << (c - 1);
    const bool neg = raw > half;
    carry = neg ? 1u : 0u;
    const uint32_t mag = neg ? (1u << c) - raw : raw;
    return mag == 0 ? FB_NONE : (((win << (c - 1)) + (mag - 1)) | (neg ? 0x80000000u : 0u));
}
// infinity flag of a table entry (word 31 of a G1 point, word 63 of a G2 point)
template <class C>
__device__ __forceinline__ bool fb_entry_inf(const uint32_t* __restrict__ table, uint32_t ent) {
    return table[(size_t)(ent & 0x7fffffffu) * Geo<C>::PT_WORDS + (Geo<C>::PT_WORDS - 1)] != 0;
}

// ---------------------------------------------------------------------------------------------- table build
template <class C>
__global__ void __launch_bounds__(64, 2) k_fb_bases(const uint32_t* __restrict__ base, uint32_t c, uint32_t nwin, uint32_t* __restrict__ proj) {
    using F = typename C::F;
    using E = typename F::E;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    E x, y;
    load_xy<OneLane<C>>(x, y, base, 0);
    ec::Proj<F> p = ec::proj_from_affine<F>(x, y);
    for (uint32_t j = 0; j < nwin; j++) {
        store_bucket<C>(proj + ((size_t)j << (c - 1)) * Geo<C>::BK_WORDS, p);
        if (j + 1 < nwin) {
#pragma unroll 1
            for (uint32_t k = 0; k < c; k++) ec::proj_dbl<F>(p);
        }
    }
}

template <class C>
__global__ void __launch_bounds__(256, 2) k_fb_level(uint32_t* __restrict__ proj, uint32_t c, uint32_t nwin, uint32_t k) {
    using F = typename C::F;
    constexpr int BK = Geo<C>::BK_WORDS;
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= (nwin << k)) return;
    const uint32_t j = t >> k, u = t & ((1u << k) - 1u);
    uint32_t* win = proj + ((size_t)j << (c - 1)) * BK;
    ec::Proj<F> a = load_bucket<C>(win + (size_t)u * BK);                               // (u + 1) B
    const ec::Proj<F> b = load_bucket<C>(win + (size_t)((1u << k) - 1u) * BK);          // 2^k B
    add_inplace(a, b);
    store_bucket<C>(win + (size_t)((1u << k) + u) * BK, a);                             // (2^k + u + 1) B
}

template <class C>
__global__ void __launch_bounds__(256, 2) k_fb_vals(const uint32_t* __restrict__ proj, uint32_t n, uint32_t* __restrict__ vals, uint8_t* __restrict__ inf_flags) {
    using F = typename C::F;
    using E = typename F::E;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    E z;
    ElemIO<E>::load(z, proj + (size_t)i * Geo<C>::BK_WORDS + 2 * Geo<C>::SLOT);
    z = F::mul(z, F::one());                      // below 2p, where the zero test is exact
    const bool inf = F::is_zero_2p(z);
    ElemIO<E>::store(vals + (size_t)i * Geo<C>::SLOT, F::select(inf, z, F::one()));
    inf_flags[i] = inf ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------- walk
// The state of a walk that its tail takes over, as COPIES (accumulate_item, curve_kernels.cuh, says why): nothing of the hot loop is address-taken.
struct FbTail {
    uint32_t s[8];
    uint32_t win, carry, ent;
    bool special, have;
};
// Everything after the hot loop: XYZZ -> projective, the cold path (the exceptional entry and the remaining windows on the complete
// formulas) and the store as a Jacobian point in the reference's form.
template <class V>
__device__ __forceinline__ void fb_tail(const uint32_t* __restrict__ table, FbTail st, uint32_t c, uint32_t nwin, const ec::Xyzz<typename V::F>& acc,
                                        uint32_t* __restrict__ o) {
    using F = typename V::F;
    ec::Proj<F> out = ec::proj_inf<F>();
    if (st.have) out = ec::xyzz_to_proj<F>(acc);
    while (st.special || st.win < nwin) {
        if (!st.special) {
            st.ent = fb_digit(st.s, st.win, c, st.carry);
            st.win++;
        }
        st.special = false;
        if (st.ent == FB_NONE || fb_entry_inf<typename V::C>(table, st.ent)) continue;
        typename V::E x, y;
        load_xy<V>(x, y, table, st.ent);
        y = F::select((st.ent >> 31) != 0, y, F::template neg<4>(y));
        const ec::Proj<F> q = ec::proj_from_affine<F>(x, y);
        V::cold_add(out, q);
    }
    store_jac_raw<V>(o, out);
}
template <class V>
static __device__ __noinline__ void fb_tail_call(const uint32_t* __restrict__ table, FbTail st, uint32_t c, uint32_t nwin, const ec::Xyzz<typename V::F>& acc,
                                                 uint32_t* __restrict__ o) {
    fb_tail<V>(table, st, c, nwin, acc, o);
}

// One unit of V per scalar (every lane of a unit recodes the same scalar: every decision below is unit-wide); workgroups of one wave
// (k_accumulate's A/B).  fmt: MI_SCALAR_* (bit 0 = Montgomery), never the sign fold.  The shape is accumulate_item's: first usable entry
// peeled, one xyzz_madd site, the tail on copies and out of line where V asks for it.
template <class V>
__device__ __forceinline__ void fb_walk_unit(const uint32_t* __restrict__ table, const uint32_t* __restrict__ scalars, uint32_t n, uint32_t fmt, uint32_t c,
                                             uint32_t nwin, uint32_t* __restrict__ jac_out) {
    using C = typename V::C;
    using F = typename V::F;
    using FA = typename V::FA;
    using E = typename V::E;
    const uint32_t i = V::unit(blockIdx.x * 64 + threadIdx.x);
    if (i >= n) return;
    uint32_t s[8];
    load_scalar(s, scalars, i, fmt & 1u);
    uint32_t win = 0, carry = 0, ent = FB_NONE;
    // the first usable entry only initialises the running sum
    bool have = false;
    while (win < nwin && !have) {
        ent = fb_digit(s, win, c, carry);
        win++;
        have = ent != FB_NONE && !fb_entry_inf<C>(table, ent);
    }
    ec::Xyzz<FA> acc;
    {
        const uint32_t e0 = have ? ent : 0u;   // entry 0 = P always exists
        E x, y;
        load_xy<V>(x, y, table, e0);
        y = F::select((e0 >> 31) != 0, y, FA::template neg_l<4>(y));
        acc.x = x; acc.y = FA::norm(y); acc.zz = F::one(); acc.zzz = F::one();
    }
    bool special = false;
    while (win < nwin) {
        ent = fb_digit(s, win, c, carry);
        win++;
        if (ent == FB_NONE || fb_entry_inf<C>(table, ent)) continue;
        E x, y;
        load_xy<V>(x, y, table, ent);
        y = F::select((ent >> 31) != 0, y, FA::template neg_l<4>(y));
        if (ec::xyzz_madd<FA>(acc, x, y)) { special = true; break; }   // exceptional pair: acc untouched, `ent` is added by the tail
    }
    FbTail st;
#pragma unroll
    for (int k = 0; k < 8; k++) st.s[k] = s[k];
    st.win = win; st.carry = carry; st.ent = ent; st.special = special; st.have = have;
    ec::Xyzz<F> fin;
    fin.x = acc.x; fin.y = acc.y; fin.zz = acc.zz; fin.zzz = acc.zzz;
    if constexpr (V::TAIL_OUT_OF_LINE) fb_tail_call<V>(table, st, c, nwin, fin, jac_out + (size_t)i * Geo<C>::RAW_JAC);
    else fb_tail<V>(table, st, c, nwin, fin, jac_out + (size_t)i * Geo<C>::RAW_JAC);
}

template <class C>
__global__ void __launch_bounds__(64, C::OCC) k_fb_walk(const uint32_t* __restrict__ table, const uint32_t* __restrict__ scalars, uint32_t n,
                                                         uint32_t fmt, uint32_t c, uint32_t nwin, uint32_t* __restrict__ jac_out) {
    fb_walk_unit<OneLane<C>>(table, scalars, n, fmt, c, nwin, jac_out);
}
template <class C>   // C = G2C (a template so that only a translation unit that uses it instantiates it)
__global__ void __launch_bounds__(64, 2) k_fb_walk_g2_coop(const uint32_t* __restrict__ table, const uint32_t* __restrict__ scalars, uint32_t n,
                                                            uint32_t fmt, uint32_t c, uint32_t nwin, uint32_t* __restrict__ jac_out) {
    fb_walk_unit<LanePairG2>(table, scalars, n, fmt, c, nwin, jac_out);
}

}  // namespace msmk

