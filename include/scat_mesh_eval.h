/* libscat_hip — C ABI of on-device mesh scoring (a public header of the one library; the conventions are those of
 * scat_hip.h and scat_eval.h: device pointers owned by the caller, explicit sizes, hipStream_t as void* last,
 * stream-ordered, never synchronises, never allocates, retains no pointer, returns 0 or a negative SCAT_E_* code).
 *
 * scat_eval.h scores the 21 joints; this header scores a whole mesh whose vertices correspond to the ground truth's
 * (ManoLayer's 778, or any V <= 1024): mean per-vertex error raw and after the similarity alignment of scat_eval.h, the
 * vertex PCK counts, and the F-score of point-cloud reconstruction at a few thresholds, from exact brute-force
 * nearest-neighbour distances in both directions.  The F-score rule is stated below; tests/_mesh_eval_oracle.py is its
 * authority, no parity with an outside script is claimed.
 */
#ifndef SCAT_MESH_EVAL_H
#define SCAT_MESH_EVAL_H
#include <stdint.h>

#include "scat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define SCAT_MESH_EVAL_MAX_V 1024
#define SCAT_MESH_EVAL_MAX_T 128
#define SCAT_MESH_EVAL_MAX_F 8

/* ---- per-batch mesh scores ----
 * pred[B,V,3], gt[B,V,3] fp32, metres, vertex i of one corresponds to vertex i of the other; 1 <= V <= 1024, B >= 1.
 * keep[B] bytes or null (all kept); thresholds_mm[T] fp32, 1 <= T <= 128 (the vertex PCK curve); f_thresholds_mm[F] fp32,
 * 1 <= F <= 8 (the F-score thresholds).  All arithmetic is fp64 on the fp32 inputs.  Per kept sample, p = pred, g = gt:
 *   mpvpe     1000 mean_i |p_i - g_i|
 *   alignment scat_eval_accumulate's over V points: both centred, K = X1 X2^T, R the proper rotation maximising tr(R K)
 *             (Horn's quaternion form), scale = tr(R K) / sum |X1|^2, t = mu2 - scale R mu1, a_i = scale R p_i + t
 *   pa_mpvpe  1000 mean_i |a_i - g_i|
 *   counts    for each thresholds_mm[t], how many of the V corresponding distances (mm) are <= it: raw and aligned
 *   F-score   for each f_thresholds_mm[k], raw (q = p) and aligned (q = a, the fp64 points, not the fp32 output):
 *               n_pred = #{i : 1000 min_j |q_i - g_j| < th}      n_gt = #{j : 1000 min_i |g_j - q_i| < th}
 *               F = 2 n_pred n_gt / (V (n_pred + n_gt)), 0 when both counts are 0
 *             (strict <, on millimetres; the harmonic mean of precision n_pred / V and recall n_gt / V).  The search is
 *             exact: the minimum over all V candidates of the squared distance, one sqrt after the minimum.
 * A sample is degenerate when any of its inputs is not finite, when sum |X1|^2 == 0, or if a score came out non-finite:
 * it is counted and left out of every sum.  keep[b] == 0: counted as skipped, none of its data is read.
 *
 * per_sample[B, 4 + 2T + 6F] doubles, 8-byte aligned, REQUIRED (it is also the hand-over between the two launches):
 *   flag (0 kept, 1 skipped, 2 degenerate), mpvpe, pa_mpvpe, 0, cnt_raw[T], cnt_pa[T],
 *   then for raw and then for aligned, per F threshold: n_pred, n_gt, F        (zeros beside a non-zero flag)
 * record[8 + 2T + 2F] doubles, 8-byte aligned:
 *   n_in, n_kept, n_skipped, n_degenerate, sum mpvpe, sum pa_mpvpe, V, 0, cnt_raw[T], cnt_pa[T], sum F_raw[F], sum F_pa[F]
 * counts are exact integers; the sums run over the kept samples in ascending sample order, and every sum over vertices
 * runs in an order fixed by V alone, so the same call gives the same bits whatever B, the grid or the timing.
 * aligned[B,V,3] fp32 or null: the aligned vertices rounded to fp32 (zeros for a sample that is not kept).
 * Two launches: one workgroup per sample, then one workgroup that folds the per_sample rows in sample order (time linear
 * in B).  No workspace. */
int scat_mesh_eval_accumulate(const float* pred, const float* gt, int V, const uint8_t* keep,
                              const float* thresholds_mm, int T, const float* f_thresholds_mm, int F,
                              double* record, double* per_sample, float* aligned, int B, void* stream);

#ifdef __cplusplus
}
#endif
#endif
