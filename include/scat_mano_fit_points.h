/* libscat_hip — C ABI of the on-device MANO fit to an unordered point cloud: nearest-vertex correspondences and the
 * ICP loop around scat_mano_fit_verts (public header of the one library; the conventions are those of
 * scat_mano_fit_verts.h: device pointers owned by the caller, explicit sizes, hipStream_t as void* last, stream-ordered,
 * never synchronises, never allocates, retains no pointer, returns 0 or a negative SCAT_E_* code, every check before any
 * HIP call).  The model arrays, V, parents and the 62 unknowns p[62] = rots[3] ++ poses[45] ++ betas[10] ++ trans[3] ++
 * log_scale[1] are scat_mano_fit_verts.h's, and so are the model points
 *     model_v = exp(log_scale) verts(rots, poses, betas)[v] + trans,          v = 0..V-1.
 * Every fp32 and int32 operand may sit at any 4-byte-aligned address; stats holds doubles and is 8-byte aligned, the
 * workspace 16-byte aligned.
 *
 * UNITS: points, model points, max_dist and dist are in one unit (metres for MANO), the data cost in that unit squared;
 * rots and poses are axis-angles in radians.
 *
 * THE ASSIGNMENT.  Point n of a hand, q_n with weight w_n (null weights: all ones), goes to its nearest model point:
 *     d2(n, v) = (dx dx + dy dy) + dz dz,   dx, dy, dz = q_n - model_v,
 * in IEEE fp64 on the fp32 numbers, each product and sum rounded once (no fused multiply-add), v ascending with a
 * strict <: the lowest index wins an exact tie.  idx[n] is that vertex and dist[n] = (float)sqrt(min d2).  A point of
 * weight 0 takes no part: idx[n] = -1, dist[n] = 0, whatever its finite coordinates.  A point is MATCHED iff w_n > 0 and
 * min d2 <= (double)max_dist * max_dist; max_dist > 0, +inf (no trim) allowed.  A point that is not matched keeps its idx
 * and dist and counts nowhere else.
 *
 * THE REDUCTION.  For fixed correspondences c(n),
 *     sum_n w_n |model_c(n) - q_n|^2 = sum_v W_v |model_v - qbar_v|^2 + const,
 *     W_v = sum_{c(n) = v} w_n,   qbar_v = (sum_{c(n) = v} w_n q_n) / W_v,
 * so the per-vertex weights and centroids are scat_mano_fit_verts' weights and targets, with the same Gauss-Newton
 * system and the same accept / reject as the per-point problem.  vw[v] = (float)W_v and vtarget[v] = (float)(S_v / W_v)
 * (0 where W_v = 0), W_v and S_v = sum w q summed in fp64 over the matched points of v with n ascending.  There is no
 * floating-point atomic.  stats[b] = {flag, matched weight, matched count, data cost}: flag 0 ok, 2 unusable; the data
 * cost is sum w_n d2 over the matched points and carries NO priors.  The three sums of stats run vertex by vertex (the
 * points of a vertex with n ascending), then over the vertices in an order fixed by V alone.  So points that are not
 * matched (trimmed, or of weight 0) change no bit of vw, vtarget or stats wherever they stand in the cloud, and the same
 * call gives the same bits.
 *
 * UNUSABLE.  A hand with a point or weight that is not finite, a negative weight, a model point that is not finite or
 * (parameter form) an entry of p that is not finite: flag 2, idx = -1, dist = 0, data cost +inf, vtarget = 0, and its vw
 * row is NaN (model_pts, when asked for, holds zeros if p was not finite).  A usable hand with NOTHING MATCHED also gets
 * a NaN vw row, with flag 0, matched 0 and data cost 0.  The NaN row is the hand-over to the fit: scat_mano_fit_verts
 * with init = 0 leaves such a hand's p untouched bit for bit and reports accepted = 0, so the priors never pull a hand
 * that has no data.  The hands beside it are not affected.
 */
#ifndef SCAT_MANO_FIT_POINTS_H
#define SCAT_MANO_FIT_POINTS_H
#include <stdint.h>

#include "scat_mano_fit_verts.h"
#ifdef __cplusplus
extern "C" {
#endif

#define SCAT_FIT_POINTS_MAX_N 8192
#define SCAT_FIT_POINTS_MAX_ROUNDS 64
#define SCAT_FIT_POINTS_MAX_STEPS 256 /* rounds * iters */

/* The caller's vertices: verts[B,V,3], points[B,N,3], weights[B,N] (null: all ones) -> idx[B,N] int32, dist[B,N],
 * vw[B,V], vtarget[B,V,3], stats[B,4] doubles.  One launch, one workgroup of 256 threads per hand: the vertices in LDS,
 * every thread walks all of them for its points.  1 <= N <= SCAT_FIT_POINTS_MAX_N, 1 <= V <= SCAT_MANO_MAX_V. */
int scat_cloud_assign(const float* verts, const float* points, const float* weights, float max_dist, int* idx, float* dist,
                      float* vw, float* vtarget, double* stats, int B, int N, int V, void* stream);

/* The same with the model points of p[B,62], posed inside the launch (scat_mano_fwd's order of sums) and rounded to
 * fp32 before the search; model_pts[B,V,3] (null: not wanted) receives them, and every other output has the bits of
 * scat_cloud_assign on those model_pts. */
int scat_mano_cloud_assign(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                           const float* hands_mean, const float* p, const float* points, const float* weights, float max_dist,
                           float* model_pts, int* idx, float* dist, float* vw, float* vtarget, double* stats, int B, int N,
                           int V, uint64_t parents, void* stream);

/* Bytes of workspace scat_mano_fit_points needs; 0 for sizes the launch refuses.  It holds stats, vtarget, vw, the
 * per-round cost and accepted count, and idx and dist (used when the caller passes none), each rounded up to 16 bytes.
 * After the call its first 4 B doubles are the last assignment's stats[B,4]; the rest holds nothing of use. */
int64_t scat_mano_fit_points_ws(int B, int N, int V);

/* Nearest-vertex ICP.  points[B,N,3], weights[B,N] (null: all ones), p[B,62] read and written: the start is the
 * caller's (ICP is a local method and no start is invented).  `rounds` (1..SCAT_FIT_POINTS_MAX_ROUNDS) times
 * { scat_mano_cloud_assign at p; scat_mano_fit_verts(init = 0, iters) on the workspace's (vtarget, vw) }, then one more
 * assignment so that the outputs describe the returned p: 2 rounds + 1 launches on the caller's stream, no
 * data-dependent exit, rounds * iters <= SCAT_FIT_POINTS_MAX_STEPS.  iters, lambda0 (every round starts from it), w_pose,
 * w_beta and free_mask are scat_mano_fit_verts'.
 *   data_cost[B]   the last assignment's data cost (no priors) rounded to fp32; +inf for an unusable hand, whose p is
 *                  untouched.
 *   accepted[B]    the accepted steps summed over the rounds (the next assignment folds each round's count).
 *   idx, dist      [B,N], the last assignment's; null: not wanted.
 *   ws             16-byte aligned, at least scat_mano_fit_points_ws(B, N, V) bytes; otherwise SCAT_E_WORKSPACE. */
int scat_mano_fit_points(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                         const float* hands_mean, const float* points, const float* weights, float* p, float* data_cost,
                         int* accepted, int* idx, float* dist, void* ws, int64_t ws_bytes, int B, int N, int V, uint64_t parents,
                         int rounds, int iters, float max_dist, float lambda0, float w_pose, float w_beta, uint64_t free_mask,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif
