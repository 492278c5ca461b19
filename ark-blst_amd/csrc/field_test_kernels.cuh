// Device side of the raw-limb field test entry (field_test_ops.cuh; test builds only).  One kernel template per family, one
// instantiation per operation, so every operation is compiled in a kernel of its own as the production kernels compile it:
//   k_field_lane   one lane per element; may call the out-of-line multiplier bodies: two waves per SIMD, no AGPRs
//   k_field_pair   the lane-pair Fp2 of coop_fp2.cuh: even lane c0, odd lane c1 (the shape of k_miller_lines2)
//   k_field_kara   the column-set accumulators of pairing_kernels.cuh: one wave per SIMD and no call (the shape of
//                  k_miller_accumulate / k_fp12_prod)
//   k_field_line   one coop_line_dbl / coop_line_add step on an injected T, P, Q: the shape of k_miller_lines2 (two lanes per pair,
//                  the loop invariants in LDS, the coefficients stored through a LineSink)
#pragma once
#if defined(MI_TEST_HOOKS)
#include "field_test_ops.cuh"
#include "pairing_kernels.cuh"

namespace msmk {

template <int OP, int NIN, int NOUT>
__global__ void __launch_bounds__(64, 2) k_field_lane(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t* p = in + (size_t)i * NIN * 16;
    Fp a[NIN], r[NOUT];
#pragma unroll
    for (int k = 0; k < NIN; k++) load_fp16(a[k], p + 16 * k);
#pragma unroll
    for (int k = 0; k < NOUT; k++) r[k] = fp28::fp_zero();
    const uint32_t flag = fieldtest::lane_op<OP>(a, p[15], r);
    uint32_t* q = out + (size_t)i * NOUT * 16;
#pragma unroll
    for (int k = 0; k < NOUT; k++) store_fp16(q + 16 * k, r[k], 0, flag);
}

// in[k]: this lane's component of the Fp2 operand k
template <int OP>
__device__ __forceinline__ uint32_t pair_op(const Fp* in, Fp* out) {
    using namespace fieldtest;
    if constexpr (OP == OP_coop_mul) out[0] = CoopF2::mul(in[0], in[1]);
    else if constexpr (OP == OP_coop_sqr) out[0] = CoopF2::sqr(in[0]);
    else if constexpr (OP == OP_coop_sqr_sub12sqr) out[0] = CoopF2::sqr_sub12sqr(in[0], in[1]);
    else if constexpr (OP == OP_coop_mul2add) out[0] = CoopF2::mul2add(in[0], in[1], in[2], in[3]);
    else if constexpr (OP == OP_coop_mul_b3) out[0] = CoopF2::mul_b3(in[0]);
    else if constexpr (OP == OP_coop_one) out[0] = CoopF2::one();
    else if constexpr (OP == OP_coopa_mul2add) out[0] = CoopF2A::mul2add(in[0], in[1], in[2], in[3]);
    else if constexpr (OP == OP_coopa_is_zero_2p) return CoopF2A::is_zero_2p(in[0]) ? 1u : 0u;
    else if constexpr (OP == OP_coopa_limbs_all_zero) return CoopF2A::limbs_all_zero(in[0]) ? 1u : 0u;
    else if constexpr (OP == OP_madd_g2) {   // one step of the G2 accumulate hot loop from an injected state
        ec::Xyzz<CoopF2A> acc;
        acc.x = in[0]; acc.y = in[1]; acc.zz = in[2]; acc.zzz = in[3];
        const bool special = ec::xyzz_madd<CoopF2A>(acc, in[4], in[5]);
        out[0] = acc.x; out[1] = acc.y; out[2] = acc.zz; out[3] = acc.zzz;
        return special ? 1u : 0u;
    }
    return 0;
}

// NIN / NOUT in Fp2 values; both lanes of a pair always run (a pair beyond n shadows the last element and stores nothing)
template <int OP, int NIN, int NOUT>
__global__ void __launch_bounds__(64, 2) k_field_pair(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t lane = blockIdx.x * 64 + threadIdx.x, h = lane & 1u;
    const bool valid = (lane >> 1) < n;
    const uint32_t e = valid ? lane >> 1 : n - 1;
    const uint32_t* p = in + (size_t)e * NIN * 32;
    Fp a[NIN], r[NOUT];
#pragma unroll
    for (int k = 0; k < NIN; k++) load_fp16(a[k], p + 32 * k + 16 * h);
#pragma unroll
    for (int k = 0; k < NOUT; k++) r[k] = fp28::fp_zero();
    const uint32_t flag = pair_op<OP>(a, r);
    if (!valid) return;
    uint32_t* q = out + (size_t)e * NOUT * 32;
#pragma unroll
    for (int k = 0; k < NOUT; k++) store_fp16(q + 32 * k + 16 * h, r[k], 0, flag);
}

template <int OP, int NIN>
__global__ void __launch_bounds__(64, 1) k_field_kara(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    using namespace fieldtest;
    __shared__ uint32_t recs[64 * ACC_COEFF_WORDS];   // kara_pre: the five-value record of the term's coefficient, one per lane
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const uint32_t* p = in + (size_t)i * NIN * 16;
    const uint32_t terms = p[15] & 0xffu, wrapped = p[15] >> 8;
    ec::Fp2 r;
    if constexpr (OP == OP_acc4) {
        uint64_t c0[2 * fp28::NL], c1[2 * fp28::NL];
#pragma unroll
        for (int t = 0; t < 2 * fp28::NL; t++) { c0[t] = 0; c1[t] = 0; }
#pragma unroll 1
        for (uint32_t t = 0; t < NIN / 4; t++) {
            if (t >= terms) break;
            fp2_acc_term4(c0, c1, lds_load_fp2(p + 64 * t), ((wrapped >> t) & 1u) != 0, lds_load_fp2(p + 64 * t + 32));
        }
        r = ec::Fp2{fp28::fp_mont_reduce(c0), fp28::fp_mont_reduce(c1)};
    } else {
        uint32_t* rec = recs + threadIdx.x * ACC_COEFF_WORDS;
        KaraCols cols;
        cols.clear();
#pragma unroll 1
        for (uint32_t t = 0; t < NIN / 4; t++) {
            if (t >= terms) break;
            const ec::Fp2 a = lds_load_fp2(p + 64 * t), g = lds_load_fp2(p + 64 * t + 32);
            const bool w = ((wrapped >> t) & 1u) != 0;
            if constexpr (OP == OP_kara) {
                fp2_acc_term(cols, a, w, g);
            } else {
                lds_store_variants(rec, a);
                fp2_acc_term_pre(cols, rec, w, g);
            }
        }
        r = fp2_kara_reduce(cols);
    }
    store_fp16(out + (size_t)i * 32, r.c0);
    store_fp16(out + (size_t)i * 32 + 16, r.c1);
}

// T, (-xP | yP) and (xQ, yQ) as the caller chose them; both lanes of a pair always run (a pair beyond n shadows the last element and
// stores nothing: the sink is not `valid`)
template <int OP, int NIN>
__global__ void __launch_bounds__(64, 2) k_field_line(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    __shared__ uint32_t cst[LINES_LDS_WORDS];
    const uint32_t lane = threadIdx.x, h = lane & 1u;
    const uint32_t pair = (blockIdx.x * 64 + lane) >> 1;
    const bool valid = pair < n;
    const uint32_t e = valid ? pair : n - 1;
    const uint32_t* p = in + (size_t)e * NIN * 32;
    uint32_t* lds_q = cst + lane * 32;                       // this lane's component of xQ | yQ
    uint32_t* lds_p = cst + 64 * 32 + (lane >> 1) * 32;      // -xP | yP of the pair (both lanes write the same values)
    ec::Proj<CoopF2> T;
    load_fp16(T.x, p + 16 * h);
    load_fp16(T.y, p + 32 + 16 * h);
    load_fp16(T.z, p + 64 + 16 * h);
    {
        Fp nx, yp;
        load_fp16(nx, p + 96);
        load_fp16(yp, p + 112);
        store_fp16(lds_p, nx);
        store_fp16(lds_p + 16, yp);
    }
    if constexpr (OP == fieldtest::OP_line_add) {
        Fp xq, yq;
        load_fp16(xq, p + 128 + 16 * h);
        load_fp16(yq, p + 160 + 16 * h);
        store_fp16(lds_q, xq);
        store_fp16(lds_q + 16, yq);
    }
    __syncthreads();
    uint32_t* q = out + (size_t)e * 6 * 32 + 16 * h;
    const LineSink sink{q, valid, (p[15] & 1u) != 0, h};
    if constexpr (OP == fieldtest::OP_line_add) coop_line_add(T, lds_q, lds_p, sink);
    else coop_line_dbl(T, lds_p, sink);
    if (!valid) return;
    store_fp16(q + 96, T.x);
    store_fp16(q + 128, T.y);
    store_fp16(q + 160, T.z);
}

inline void launch_field_op(int op, const uint32_t* in, uint32_t n, uint32_t* out, hipStream_t s) {
    using namespace fieldtest;
    const dim3 one((n + 63) / 64), two((2 * n + 63) / 64), blk(64);
    switch (op) {
#define X(name, nin, nout) case OP_##name: hipLaunchKernelGGL((k_field_lane<OP_##name, nin, nout>), one, blk, 0, s, in, n, out); break;
        FIELD_OPS_LANE(X)
#undef X
#define X(name, nin, nout) case OP_##name: hipLaunchKernelGGL((k_field_pair<OP_##name, nin, nout>), two, blk, 0, s, in, n, out); break;
        FIELD_OPS_PAIR(X)
#undef X
#define X(name, nin, nout) case OP_##name: hipLaunchKernelGGL((k_field_kara<OP_##name, nin>), one, blk, 0, s, in, n, out); break;
        FIELD_OPS_KARA(X)
#undef X
#define X(name, nin, nout) case OP_##name: hipLaunchKernelGGL((k_field_line<OP_##name, nin>), two, blk, 0, s, in, n, out); break;
        FIELD_OPS_LINE(X)
#undef X
        default: break;
    }
}

}  // namespace msmk
#endif
