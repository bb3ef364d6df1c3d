/* libscat_hip — C ABI of on-device evaluation (second public header of the one library; the conventions are those of
 * scat_hip.h: device pointers owned by the caller, explicit sizes, caller-provided workspace, hipStream_t as void* last,
 * stream-ordered, never synchronises, never allocates, retains no pointer, returns 0 or a negative SCAT_E_* code).
 *
 * Stands in for the scoring half of the reference's eval loop (eval.py:788-1053, reference checkout tomguluson92/SCAT):
 *   eval.py:817-823    blank padding frames dropped                      scat_eval_frame_mask
 *   eval.py:467-475    orthographic projection * 112 + 112               scat_eval_accumulate (2-D error)
 *   eval.py:110-161    similarity (Procrustes) alignment, applied :953   scat_eval_accumulate
 *   eval.py:300-316    PCK counts per threshold                          scat_eval_accumulate
 *   eval.py:1026       MPJPE                                             scat_eval_accumulate
 * The per-batch PCK average of eval.py:998,1028 and the AUC of eval.py:328-340 are host arithmetic on the record rows
 * (scat_amd/evaluator.py finalize).
 */
#ifndef SCAT_EVAL_H
#define SCAT_EVAL_H
#include <stdint.h>

#include "scat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- blank-frame rule: eval.py:817-823 ----
 * x[B,n] fp32 (n = 3*224*224 for the network's input; any n >= 1, any 4-byte-aligned x), keep[B] bytes:
 *   keep[b] = 1 if b == 0 or | |sum x[b]| - blank_sum | > tol, else 0.
 * b == 0 is the reference's quirk, kept: its filter keeps the samples whose index survives `idxs * arange(B)`, and a
 * dropped sample's product is 0, which is sample 0's own index — sample 0 can never be dropped.
 * The sum is fp64 in an order fixed by n and the address of the row alone (8192-float chunks of the 16-byte-aligned
 * body, then ascending over chunks): the same call gives the same bits whatever the device does.
 * ws: 8-byte aligned, scat_eval_frame_mask_ws(B, n) bytes. */
int scat_eval_frame_mask(const float* x, uint8_t* keep, int B, int64_t n, float blank_sum, float tol, void* ws,
                         int64_t ws_bytes, void* stream);
int64_t scat_eval_frame_mask_ws(int B, int64_t n);

/* ---- per-batch scores: eval.py:110-161, :300-316, :467-475, :953, :1026 ----
 * out[B,66] = camera (s, tx, ty) then 21 x 3 joints; gt3d[B,63] / gt2d[B,42] with row stride ld_gt floats (as
 * scat_loss_fwd_bwd takes them); keep[B] bytes or null (all kept); thresholds_mm[T] fp32, 1 <= T <= 64.  All arithmetic
 * is fp64 on the fp32 inputs.  Per kept sample, p = predicted joints, g = gt3d (metres):
 *   mpjpe     1000 mean_j |p_j - g_j|
 *   alignment both centred, K = X1 X2^T, R the proper rotation maximising tr(R K) (Horn's quaternion form of the
 *             reference's V diag(1,1,sign det(U V^T)) U^T), scale = tr(R K) / sum |X1|^2, t = mu2 - scale R mu1
 *   pa_mpjpe  1000 mean_j |scale R p_j + t - g_j|
 *   err2d     mean_j |(s (p_j.xy + (tx, ty))) 112 + 112 - gt2d_j|   pixels, un-aligned joints
 *   counts    for each threshold, how many of the 21 distances (mm) are <= it: raw and aligned
 * A sample is degenerate when any of its inputs is not finite or sum |X1|^2 == 0 (the reference yields NaN there), or if
 * a score came out non-finite; it is counted and left out of every sum.  keep[b] == 0: counted as skipped, nothing read.
 *
 * record[8 + 2T] doubles, 8-byte aligned:
 *   n_in, n_kept, n_skipped, n_degenerate, sum mpjpe, sum pa_mpjpe, sum err2d, 0, cnt_raw[T], cnt_pa[T]
 * counts are exact integers; the sums run over the kept samples in ascending sample order, so the row is bit-identical
 * from run to run.  Optional (nullable) outputs: per_sample[B,4] doubles = mpjpe, pa_mpjpe, err2d, flag (0 kept,
 * 1 skipped, 2 degenerate; zeros beside a non-zero flag), 8-byte aligned; aligned[B,63] fp32, the aligned joints (zeros
 * for a sample that is not kept).
 * Two launches: one wavefront per sample, then one workgroup that folds the per-sample rows in order (time linear in
 * B).  ws: 8-byte aligned, scat_eval_accumulate_ws(B, T) bytes. */
int scat_eval_accumulate(const float* out, const float* gt3d, const float* gt2d, int ld_gt, const uint8_t* keep,
                         const float* thresholds_mm, int T, double* record, double* per_sample, float* aligned, int B,
                         void* ws, int64_t ws_bytes, void* stream);
int64_t scat_eval_accumulate_ws(int B, int T);

#ifdef __cplusplus
}
#endif
#endif
