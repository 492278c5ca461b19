/* Test-only entry points of libarkblst_amd_test.so (built with -DMI_TEST_HOOKS; the product library exports none of them
 * and compiles none of the code behind them).  Used by tests/ to pin the device field arithmetic against the oracle, to
 * force the pairing kernels through every sharing / batching shape at small sizes, to exercise the multi-pass split of very
 * long inputs at small sizes, and to inject allocation failures. */
#ifndef ARKBLST_AMD_TEST_HOOKS_H
#define ARKBLST_AMD_TEST_HOOKS_H
#include "../../include/arkblst_amd.h"
#ifdef __cplusplus
extern "C" {
#endif
/* batch Montgomery multiply / square / add / sub on the device representation, I/O in blst_fp form. op: 0 mul, 1 sqr(a), 2 add, 3 sub */
int mi_test_fp_op(mi_ctx *ctx, int op, const mi_fp *a, const mi_fp *b, mi_fp *out, size_t n);
/* one field primitive on raw device-form limbs (field_test_ops.cuh): n <= 4096 elements, operands and results in 16-word slots (14 limbs,
 * word 15 of an element's first operand slot = op argument, word 15 of a result slot = the op's verdict); no conversion on the way */
int mi_test_field_op(mi_ctx *ctx, int op, const uint32_t *in, size_t n, uint32_t *out);
/* name of op (NULL beyond the last one), its operand / result slots per element and kind: 0 one lane, 1 lane pair, 2 column-set accumulator,
 * 3 one step of the pairing line kernel (coop_line_dbl / coop_line_add) */
const char *mi_test_field_op_info(int op, int *in_slots, int *out_slots, int *kind);
/* one production kernel of the pairing row on device-form limbs (16-word slots, an Fp12 = 12 slots in blst_fp12 order), n <= 4096:
 * stage 0 k_miller_accumulate: `in` = a complete line buffer in the production layout ([block of 10 m pairs][68 lines][pair][c0, c1, c4 as Fp2],
 *   the last block whole: in_words = ceil(n / 10m) * 10m * 68 * 96), n pairs, m <= 16 pairs per accumulator; out = ceil(n / m) Fp12 values as stored;
 * stage 1 k_fp12_prod: one tree level over n Fp12 values (in_words = 192 n), out = ceil(n / 2) values; m ignored;
 * stage 2 k_fp12_to_raw: n <= 64 values (in_words = 192 n), out = 144 raw words (a blst_fp12) each; m ignored */
int mi_test_pairing_stage(mi_ctx *ctx, int stage, const uint32_t *in, size_t in_words, size_t n, unsigned m, uint32_t *out);
/* pairing: pairs per accumulator (0 = heuristic), pairs per line batch (0 = 2^17), the one-lane-per-pair first version */
int mi_test_set_pairing(mi_ctx *ctx, unsigned share, unsigned batch, int single_lane);
/* points per pass of the MSM pipeline (0 = built-in 2^26): longer calls are split and the parts added */
int mi_test_set_max_part(mi_ctx *ctx, size_t points);
/* the next `count` growing device allocations of the process fail (as hipErrorOutOfMemory would) */
void mi_test_fail_allocs(int count);
/* treat every device slot as remote from the scalar vector's device: device-resident scalars of a multi-device context are then
 * staged by peer copies even on one GPU (the path every slot but the owner's takes on a real multi-GPU node) */
int mi_test_set_no_peer(mi_ctx *ctx, int no_peer);
/* the window-size plan of an n-point call (host only, no device): out[13] = c, windows, bucket sets, buckets per logical lane of the cooperative
 * reduce (coop_L), buckets per reduce chunk, logT, lo_bits, serial reduce, chunks per window, buckets (hi, lo), chunks, buckets per lane of the
 * serial reduce.  group 0 = G1, 1 = G2; shared bit 0 = precomputed tables, bit 1 = sign fold (a validated resident set); c = 0 in out[0]: no usable plan.
 * The plan — this one and every call's — reads three switches from the environment (msm_sort.hip reduce_geometry, test build only):
 * MI_TEST_COOP_L pins the cooperative reduce's buckets per logical lane (clamped to 1 .. min(64, buckets per window / logical lanes)),
 * MI_TEST_SERIAL_MIN_BUCKETS the bucket count from which the serial reduce runs, MI_TEST_SERIAL_L its buckets per lane (1 .. 64) */
int mi_test_plan(size_t n, unsigned forced_c, int group, int shared, size_t stride, uint32_t *out);
#ifdef __cplusplus
}
#endif
#endif
