// Raw-limb test entry of the field arithmetic (test builds only: everything here sits under MI_TEST_HOOKS).
//
// One table of operations, each a call of the PRODUCTION function on operands whose every limb the caller chose: no conversion
// through fp_from_blst / fp_to_blst, so a test can hand a function the extremes its own comment permits (maximal N-form limbs,
// the top of a K p value contract, both representations of zero, lazy 2^29 limbs) and read back the raw limbs of the result.
// Operands and results travel in the 16-word slot layout of load_fp16 / store_fp16; word 15 of an element's first operand slot
// carries an op-specific argument (`aux`), word 15 of every result slot carries the op's verdict (predicates, xyzz_madd).
//
// The one-lane operations compile on the host as well (tests/host/fp28_host_check.cpp runs the same table with g++), the
// lane-pair, line-step and Karatsuba ones exist on the device only (field_test_kernels.cuh).
#pragma once
#if defined(MI_TEST_HOOKS)
#include "ec.cuh"

namespace fieldtest {

using fp28::Fp;

// X(name, operand slots, result slots).  One lane per element.
#define FIELD_OPS_SUBK(X, K) X(fp_sub##K, 2, 1) X(fp_sub_lazy##K, 2, 1) X(fp_neg##K, 1, 1)
#define FIELD_OPS_FP2(X, V) \
    X(V##_mul, 4, 2) X(V##_sqr, 2, 2) X(V##_mul2add, 8, 2) X(V##_sqr_sub12sqr, 4, 2) X(V##_mul_b3, 2, 2) X(V##_is_zero_2p, 2, 1)
#define FIELD_OPS_LANE(X) \
    X(fp_mul, 2, 1) X(fp_mul_os, 2, 1) X(fp_mul_call, 2, 1) X(fp_sqr, 1, 1) X(fp_sqr_os, 1, 1) X(fp_sqr_call, 1, 1) \
    X(fp_mul2add, 4, 1) X(fp_mul2add_os, 4, 1) X(fp_mul2add_call, 4, 1) X(fp_mul4add, 8, 1) \
    X(fp_add, 2, 1) X(fp_add_lazy, 2, 1) X(fp_norm, 1, 1) \
    FIELD_OPS_SUBK(X, 2) FIELD_OPS_SUBK(X, 4) FIELD_OPS_SUBK(X, 8) FIELD_OPS_SUBK(X, 16) FIELD_OPS_SUBK(X, 32) FIELD_OPS_SUBK(X, 64) \
    X(fp_sub8_lazy_wide, 2, 1) X(fp_mul_small2, 1, 1) X(fp_mul_small3, 1, 1) X(fp_mul_small12, 1, 1) X(fp_mul_small15, 1, 1) \
    X(fp_reduce_small, 1, 1) X(fp_carry_exact, 1, 1) X(fp_canon_2p, 1, 1) \
    X(fp_is_zero_2p, 1, 1) X(fp_is_zero_2p_exact, 1, 1) X(fp_is_zero_any, 1, 1) \
    FIELD_OPS_FP2(X, fp2c) FIELD_OPS_FP2(X, fp2i) \
    X(madd_g1, 6, 4) X(madd_g2_lane, 12, 8) X(fp_from_blst, 1, 1) X(fp_to_blst, 1, 1)
// Two lanes per element (even lane c0, odd lane c1): operands and results counted in Fp2 values of two slots each.
#define FIELD_OPS_PAIR(X) \
    X(coop_mul, 2, 1) X(coop_sqr, 1, 1) X(coop_sqr_sub12sqr, 2, 1) X(coop_mul2add, 4, 1) X(coop_mul_b3, 1, 1) X(coop_one, 1, 1) \
    X(coopa_mul2add, 4, 1) X(coopa_is_zero_2p, 1, 1) X(coopa_limbs_all_zero, 1, 1) X(madd_g2, 6, 4)
// Column-set accumulators of the pairing kernels, one lane per element: terms of four slots (a.c0, a.c1, g.c0, g.c1);
// aux = number of terms | wrapped flags << 8.
#define FIELD_OPS_KARA(X) X(kara, 16, 2) X(kara_pre, 16, 2) X(acc4, 24, 2)
// One step of the G2 point walk of k_miller_lines2 (coop_line_dbl / coop_line_add), two lanes per element in a kernel of that kernel's
// shape.  Operands in Fp2 values of two slots: T = (X, Y, Z), then (-xP | yP) as the two slots of one value, then (xQ, yQ) for the
// addition; results c0, c1, c4 (written by the LineSink) and the new T.  aux bit 0 = the sink's `inf`.
#define FIELD_OPS_LINE(X) X(line_dbl, 4, 6) X(line_add, 6, 6)

enum Op : int {
#define X(name, nin, nout) OP_##name,
    FIELD_OPS_LANE(X) FIELD_OPS_PAIR(X) FIELD_OPS_KARA(X) FIELD_OPS_LINE(X)
#undef X
    OP_COUNT
};
enum Kind : int { KIND_LANE = 0, KIND_PAIR = 1, KIND_KARA = 2, KIND_LINE = 3 };

// name, slots per element in and out (a lane-pair element has two slots per Fp2 value), kind; nullptr for an unknown op
inline const char* op_info(int op, int* in_slots, int* out_slots, int* kind) {
    switch (op) {
#define X(name, nin, nout) case OP_##name: *in_slots = nin; *out_slots = nout; *kind = KIND_LANE; return #name;
        FIELD_OPS_LANE(X)
#undef X
#define X(name, nin, nout) case OP_##name: *in_slots = 2 * nin; *out_slots = 2 * nout; *kind = KIND_PAIR; return #name;
        FIELD_OPS_PAIR(X)
#undef X
#define X(name, nin, nout) case OP_##name: *in_slots = nin; *out_slots = nout; *kind = KIND_KARA; return #name;
        FIELD_OPS_KARA(X)
#undef X
#define X(name, nin, nout) case OP_##name: *in_slots = 2 * nin; *out_slots = 2 * nout; *kind = KIND_LINE; return #name;
        FIELD_OPS_LINE(X)
#undef X
        default: return nullptr;
    }
}

template <class F2, int WHICH>
FP_HD uint32_t fp2_op(const Fp* in, Fp* out) {
    using E = ec::Fp2;
    const E a{in[0], in[1]};
    E r = F2::zero();
    uint32_t flag = 0;
    if constexpr (WHICH == 0) r = F2::mul(a, E{in[2], in[3]});
    else if constexpr (WHICH == 1) r = F2::sqr(a);
    else if constexpr (WHICH == 2) r = F2::mul2add(a, E{in[2], in[3]}, E{in[4], in[5]}, E{in[6], in[7]});
    else if constexpr (WHICH == 3) r = F2::sqr_sub12sqr(a, E{in[2], in[3]});
    else if constexpr (WHICH == 4) r = F2::mul_b3(a);
    else flag = F2::is_zero_2p(a) ? 1u : 0u;
    out[0] = r.c0;
    if constexpr (WHICH < 5) out[1] = r.c1;
    return flag;
}

// the operation OP on in[0 .. operand slots), results to out[0 .. result slots); returns the verdict
template <int OP>
FP_HD uint32_t lane_op(const Fp* in, uint32_t aux, Fp* out) {
    using namespace fp28;
    (void)aux;
#define SUBK(K) \
    else if constexpr (OP == OP_fp_sub##K) out[0] = fp_sub<K>(in[0], in[1]); \
    else if constexpr (OP == OP_fp_sub_lazy##K) out[0] = fp_sub_lazy<K>(in[0], in[1]); \
    else if constexpr (OP == OP_fp_neg##K) out[0] = fp_neg<K>(in[0]);
#define FP2V(V, F2) \
    else if constexpr (OP == OP_##V##_mul) return fp2_op<F2, 0>(in, out); \
    else if constexpr (OP == OP_##V##_sqr) return fp2_op<F2, 1>(in, out); \
    else if constexpr (OP == OP_##V##_mul2add) return fp2_op<F2, 2>(in, out); \
    else if constexpr (OP == OP_##V##_sqr_sub12sqr) return fp2_op<F2, 3>(in, out); \
    else if constexpr (OP == OP_##V##_mul_b3) return fp2_op<F2, 4>(in, out); \
    else if constexpr (OP == OP_##V##_is_zero_2p) return fp2_op<F2, 5>(in, out);
    if constexpr (OP == OP_fp_mul) out[0] = fp_mul(in[0], in[1]);
    else if constexpr (OP == OP_fp_mul_os) out[0] = fp_mul_os(in[0], in[1]);
    else if constexpr (OP == OP_fp_mul_call) out[0] = fp_mul_call(in[0], in[1]);
    else if constexpr (OP == OP_fp_sqr) out[0] = fp_sqr(in[0]);
    else if constexpr (OP == OP_fp_sqr_os) out[0] = fp_sqr_os(in[0]);
    else if constexpr (OP == OP_fp_sqr_call) out[0] = fp_sqr_call(in[0]);
    else if constexpr (OP == OP_fp_mul2add) out[0] = fp_mul2add(in[0], in[1], in[2], in[3]);
    else if constexpr (OP == OP_fp_mul2add_os) out[0] = fp_mul2add_os(in[0], in[1], in[2], in[3]);
    else if constexpr (OP == OP_fp_mul2add_call) out[0] = fp_mul2add_call(in[0], in[1], in[2], in[3]);
    else if constexpr (OP == OP_fp_mul4add) out[0] = fp_mul4add(in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7]);
    else if constexpr (OP == OP_fp_add) out[0] = fp_add(in[0], in[1]);
    else if constexpr (OP == OP_fp_add_lazy) out[0] = fp_add_lazy(in[0], in[1]);
    else if constexpr (OP == OP_fp_norm) out[0] = fp_norm(in[0]);
    SUBK(2) SUBK(4) SUBK(8) SUBK(16) SUBK(32) SUBK(64)
    else if constexpr (OP == OP_fp_sub8_lazy_wide) out[0] = fp_sub8_lazy_wide(in[0], in[1]);
    else if constexpr (OP == OP_fp_mul_small2) out[0] = fp_mul_small<2>(in[0]);
    else if constexpr (OP == OP_fp_mul_small3) out[0] = fp_mul_small<3>(in[0]);
    else if constexpr (OP == OP_fp_mul_small12) out[0] = fp_mul_small<12>(in[0]);
    else if constexpr (OP == OP_fp_mul_small15) out[0] = fp_mul_small<15>(in[0]);
    else if constexpr (OP == OP_fp_reduce_small) out[0] = fp_reduce_small(in[0]);
    else if constexpr (OP == OP_fp_carry_exact) { out[0] = in[0]; fp_carry_exact(out[0]); }
    else if constexpr (OP == OP_fp_canon_2p) out[0] = fp_canon_2p(in[0]);
    else if constexpr (OP == OP_fp_is_zero_2p) return fp_is_zero_2p(in[0]) ? 1u : 0u;
    else if constexpr (OP == OP_fp_is_zero_2p_exact) return fp_is_zero_2p_exact(in[0]) ? 1u : 0u;
    else if constexpr (OP == OP_fp_is_zero_any) return fp_is_zero_any(in[0]) ? 1u : 0u;
    FP2V(fp2c, ec::Fp2Ops) FP2V(fp2i, ec::Fp2OpsInline)
    else if constexpr (OP == OP_madd_g1) {   // one step of the G1 accumulate hot loop from an injected state
        ec::Xyzz<ec::FpOpsInline> acc;
        acc.x = in[0]; acc.y = in[1]; acc.zz = in[2]; acc.zzz = in[3];
        const bool special = ec::xyzz_madd<ec::FpOpsInline>(acc, in[4], in[5]);
        out[0] = acc.x; out[1] = acc.y; out[2] = acc.zz; out[3] = acc.zzz;
        return special ? 1u : 0u;
    }
    else if constexpr (OP == OP_madd_g2_lane) {   // the same step over Fp2 with one lane per value (the field of k_accumulate<G2C>)
        using F2 = ec::Fp2OpsInline;
        ec::Xyzz<F2> acc;
        acc.x = ec::Fp2{in[0], in[1]}; acc.y = ec::Fp2{in[2], in[3]}; acc.zz = ec::Fp2{in[4], in[5]}; acc.zzz = ec::Fp2{in[6], in[7]};
        const bool special = ec::xyzz_madd<F2>(acc, ec::Fp2{in[8], in[9]}, ec::Fp2{in[10], in[11]});
        out[0] = acc.x.c0; out[1] = acc.x.c1; out[2] = acc.y.c0; out[3] = acc.y.c1;
        out[4] = acc.zz.c0; out[5] = acc.zz.c1; out[6] = acc.zzz.c0; out[7] = acc.zzz.c1;
        return special ? 1u : 0u;
    }
    // the conversions to / from the reference's words: the 12 words travel in limbs 0..11 of the slot (limbs 12, 13 zero)
    else if constexpr (OP == OP_fp_from_blst) {
        uint32_t w[12];
        for (int k = 0; k < 12; k++) w[k] = in[0].l[k];
        out[0] = fp_from_blst(w);
    }
    else if constexpr (OP == OP_fp_to_blst) {
        uint32_t w[12];
        fp_to_blst(w, in[0]);
        for (int k = 0; k < 12; k++) out[0].l[k] = w[k];
    }
#undef SUBK
#undef FP2V
    return 0;
}

}  // namespace fieldtest
#endif
