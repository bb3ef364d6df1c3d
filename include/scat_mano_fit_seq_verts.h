/* libscat_hip — C ABI of the on-device MANO fit to a track of meshes and to a track of point clouds (public header of
 * the one library; the conventions are those of scat_mano_fit_seq.h and scat_mano_fit_points.h: device pointers owned by
 * the caller, explicit sizes, hipStream_t as void* last, stream-ordered, never synchronises, never allocates, retains no
 * pointer, returns 0 or a negative SCAT_E_* code, every check before any HIP call).  The model arrays, V, parents and the
 * 62 unknowns of one frame, p[62] = rots[3] ++ poses[45] ++ betas[10] ++ trans[3] ++ log_scale[1], are
 * scat_mano_fit_verts.h's; the per-vertex data term and the plane metric M_v, rho_v are scat_mano_fit_plane.h's; the
 * smoothness between consecutive frames, the block-tridiagonal solve and the accept rule are scat_mano_fit_seq.h's.
 * Every fp32 and int32 operand may sit at any 4-byte-aligned address; the workspace is 16-byte aligned.
 *
 * THE PROBLEM.  S sequences of T frames.  With model_tv = exp(log_scale_t) verts(p_t)[v] + trans_t, targets X_tv, weights
 * w_tv and, where normals are given, rho_tv of scat_mano_fit_plane.h (|r|^2 without normals), the cost of sequence s is
 *     cost_s = sum_t ( sum_v w_tv rho_tv(model_tv - X_tv) + w_pose |poses_t|^2 + w_beta |betas_t|^2 )
 *            + sum_{t >= 1} sum_i d_i (p_t,i - p_t-1,i)^2,
 * d_i the smoothness weight of unknown i's group: s_rots, s_poses, s_betas, s_trans, s_scale.  All five zero decouples the
 * frames: every frame is then scat_mano_fit_verts' problem, under one shared lambda and one accept / reject.
 *
 * UNITS.  The data term is in the targets' (the points') unit squared, summed over V vertices (over the matched points
 * of a cloud): it is V / 21 times a joints track's at the same residual.  A smoothness weight multiplies a squared
 * difference in the unknown's OWN unit: radians squared for s_rots and s_poses (the penalty is on the axis-angle numbers,
 * not on the rotations), the shape coefficients' unit squared for s_betas, the targets' unit squared for s_trans, the
 * square of a log-ratio for s_scale.  For a mesh in metres with unit weights, s_trans = V counts a step of the
 * translation like a residual of the same size at every vertex.
 *
 * THE SOLVE.  One Levenberg-Marquardt per sequence: one lambda, one accept / reject, one accepted count.  What is
 * independent per frame runs as a launch over S T workgroups (the frame kernel: scat_mano_fit_verts' tiles and
 * accumulation at a given point, no solver; it leaves the frame's undamped A_t, g_t and cost in the workspace), and only
 * the elimination along the frames runs one workgroup per sequence (the track kernel: it holds no model).  Per call the
 * track kernel decides on the previous trial (the T frame costs added in frame order, then the smoothness terms, t
 * ascending, i ascending; accepted only if every pivot of every frame was positive and finite, every trial unknown of
 * every frame is finite and cost_s drops; then lambda /= 10, otherwise lambda *= 10 within 1e-12..1e12), and then solves
 * from the current point: to A_t it adds c_t d_i on the diagonal (c_t the number of neighbours of frame t) and
 * d_i ((p_t - p_t-1) + (p_t - p_t+1))_i to g_t, sets the unit rows of frozen unknowns, multiplies the full diagonal by
 * 1 + lambda, and factors the block-tridiagonal system by scat_mano_fit_seq.h's recurrences, forward and backward.  A_t
 * and g_t are kept undamped for the current and for the trial point, so a rejected step costs no second assembly.  The
 * cost of a point is computed once, by the frame kernel's accumulation, and carried: an accepted trial's cost becomes
 * the current cost with the same bits.
 *
 * LAUNCHES.  With init = 0: the frame kernel at the start, `iters` times { track kernel, frame kernel at the trial }, and
 * a last track call that decides and writes the results: 2 iters + 2 launches.  init = 1 puts two more in front: the
 * frame kernel in its start form (Procrustes per frame) and the track kernel in its scan form.  No host synchronisation,
 * no data-dependent exit, no atomic; every sum runs in an order fixed by the sizes.  The same call gives the same bits,
 * and the bits of a sequence depend neither on S nor on its index.
 *
 * WORKSPACE, per frame: L_t with y_t (63 x 62 floats), M_t^T (62 x 62) and two copies of the 62 unknowns, as in
 * scat_mano_fit_seq.h (31,496 bytes); A_t with g_t as its 63rd row for the current and the trial point (2 x 63 x 62
 * floats, 31,248 bytes); the frame's cost and its state (8 bytes): 62,752 bytes.  Per sequence: 32 bytes of state
 * (lambda, cost, which buffer is current, accepted, failed pivot, refused).  Each of the five parts is rounded up to 16
 * bytes.  It holds nothing of use after the call.
 *
 * WHAT REFUSES A SEQUENCE: a target, weight or normal that is not finite, a negative weight, or (init = 0) a start that
 * is not finite, in any frame.  Then cost = +inf, accepted = 0 and p is the start (init = 0: the caller's, untouched;
 * init = 1: zeros).  The other sequences are not affected.
 * WHAT IS BRIDGED: a frame whose weights are all zero is legal whatever its finite targets.  It has no data term (A_t is
 * the priors, the data part of g_t is zero), is held by its neighbours through the smoothness, and its targets do not
 * reach the result.  This is also how a short clip is padded.
 */
#ifndef SCAT_MANO_FIT_SEQ_VERTS_H
#define SCAT_MANO_FIT_SEQ_VERTS_H
#include <stdint.h>

#include "scat_mano_fit_plane.h"
#include "scat_mano_fit_seq.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace scat_mano_fit_seq_verts needs; 0 for S < 1, T outside 1..SCAT_FIT_SEQ_MAX_T, V outside
 * 1..SCAT_MANO_MAX_V or more than 2^31 - 1 frames in all (S T is a grid size), which the launch refuses.  The size does not
 * depend on V. */
int64_t scat_mano_fit_seq_verts_ws(int S, int T, int V);

/* targets[S,T,V,3], weights[S,T,V] (null: all ones), normals[S,T,V,3] (null: the Euclidean cost; otherwise the plane
 * metric with 0 <= w_tangent <= 1, and init must be 0) -> p[S,T,62], cost[S], accepted[S].
 *   init = 0     p is read: the caller's start.  p is written only after an accepted step.
 *   init = 1     p is written only: scat_mano_fit_verts' Procrustes start over the vertices frame by frame, then
 *                scat_mano_fit_seq's scan: rots_t takes the equivalent axis-angle closer to rots_t-1, a frame of total
 *                weight zero takes the start of the frame before it, frame 0 that of the first frame that has weight.
 * ws: 16-byte aligned, at least scat_mano_fit_seq_verts_ws(S, T, V) bytes; otherwise SCAT_E_WORKSPACE.
 * cost: cost_s at the returned p; accepted: the number of accepted steps, 0..iters. */
int scat_mano_fit_seq_verts(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                            const float* hands_mean, const float* targets, const float* weights, const float* normals, float* p,
                            float* cost, int* accepted, void* ws, int64_t ws_bytes, int S, int T, int V, uint64_t parents,
                            int iters, int init, float w_tangent, float lambda0, float w_pose, float w_beta, float s_rots,
                            float s_poses, float s_betas, float s_trans, float s_scale, uint64_t free_mask, void* stream);

/* Bytes of workspace scat_mano_fit_points_seq needs; 0 for sizes the launch refuses.  F = 0: no topology (nearest
 * vertex); otherwise 1 <= F <= SCAT_RENDER_MAX_F.  scat_mano_fit_points_ws' parts for B = S T hands (then the normals
 * when F > 0), then scat_mano_fit_seq_verts_ws(S, T, V).  After the call its first 4 S T doubles are the last
 * assignment's stats[S T,4]. */
int64_t scat_mano_fit_points_seq_ws(int S, int T, int N, int V, int F);

/* ICP over a track of clouds: points[S,T,N,3], weights[S,T,N] (null: all ones); faces, vf_off, vf_idx all three
 * (point-to-plane, scat_mano_fit_points_plane's round) or all null with F = 0 (nearest vertex, scat_mano_fit_points').
 * `rounds` times { one assignment launch over the S T frames at p; one track solve (scat_mano_fit_seq_verts, init = 0,
 * `iters` iterations) on the workspace's per-vertex centroids and weights, with the round's normals in the plane form },
 * then one more assignment: rounds (2 iters + 3) + 1 launches.  p[S,T,62] is the caller's start, read and written.
 *   NOTHING MATCHED  a frame in which no point is matched (all beyond max_dist, or of weight zero) is BRIDGED inside
 *                this loop, as if its weights were zero: it does not refuse its sequence.
 *   UNUSABLE     a frame with a point, weight or unknown that is not finite, or a negative weight, refuses its sequence
 *                for that round: its p stays.  The other sequences are not affected.
 * data_cost[S,T]: the last assignment's data cost per frame (the metric one with a topology), +inf for an unusable
 * frame; accepted[S]: the accepted steps summed over the rounds; idx, dist [S,T,N] (nullable): the last assignment's.
 * rounds, iters, max_dist, w_tangent and the limits (SCAT_FIT_POINTS_MAX_ROUNDS, SCAT_FIT_POINTS_MAX_STEPS) are
 * scat_mano_fit_points_plane's; s_rots .. s_scale as above, against a data term summed over the matched points. */
int scat_mano_fit_points_seq(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                             const float* hands_mean, const float* points, const float* weights, const int32_t* faces,
                             const int32_t* vf_off, const int32_t* vf_idx, float* p, float* data_cost, int* accepted, int* idx,
                             float* dist, void* ws, int64_t ws_bytes, int S, int T, int N, int V, int F, uint64_t parents,
                             int rounds, int iters, float max_dist, float w_tangent, float lambda0, float w_pose, float w_beta,
                             float s_rots, float s_poses, float s_betas, float s_trans, float s_scale, uint64_t free_mask,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
