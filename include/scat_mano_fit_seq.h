/* libscat_hip — C ABI of the on-device MANO fit to a track of frames (public header of the one library; the conventions
 * are those of scat_mano_fit.h: device pointers owned by the caller, explicit sizes, hipStream_t as void* last,
 * stream-ordered, never synchronises, never allocates, retains no pointer, returns 0 or a negative SCAT_E_* code).  The
 * model arrays, V, parents, tip0..4, joint_map (CLAMPED to 0..20 on the device) and the 62 unknowns of one frame,
 *     p[62] = rots[3] ++ poses[45] ++ betas[10] ++ trans[3] ++ log_scale[1],
 * are scat_mano_fit's.  Every operand but the workspace may sit at any 4-byte-aligned address.
 *
 * scat_mano_fit's problem over S sequences of T frames each, the frames of a sequence coupled by a quadratic penalty on
 * the difference of consecutive unknowns.  With m_tj = exp(log_scale_t) x(p_t)[joint_map[j]] + trans_t the model joints
 * of frame t, X_tj the targets and w_tj the weights, the cost of sequence s is
 *     cost_s = sum_t ( sum_j w_tj |m_tj - X_tj|^2 + w_pose |poses_t|^2 + w_beta |betas_t|^2 )
 *            + sum_{t >= 1} sum_i d_i (p_t,i - p_t-1,i)^2,
 * d_i the smoothness weight of unknown i's group: s_rots, s_poses, s_betas, s_trans, s_scale.  All five zero decouples
 * the frames: every frame is then scat_mano_fit's problem, under one shared lambda and one accept / reject.
 *
 * UNITS.  The data term is in the targets' unit squared (square metres for targets in metres).  A smoothness weight
 * multiplies a squared difference in the unknown's OWN unit: radians squared for s_rots and s_poses, the shape
 * coefficients' unit squared for s_betas, the targets' unit squared for s_trans, and the square of a log-ratio (a pure
 * number) for s_scale.  So s_trans = 1 counts a step of the translation like one joint's residual of the same size, and
 * for targets in metres s_rots = 1e-4 counts 0.1 rad per frame like a 1 mm residual.  The penalty is on the axis-angle
 * numbers themselves, not on the rotations they stand for: r and r (1 - 2 pi / |r|) are the same rotation and not the
 * same numbers, and a track that is continuous as rotations pays for such a jump.  init = 1 starts without one.
 *
 * The solver is one Levenberg-Marquardt over the whole sequence: one lambda, one accept / reject and one accepted count
 * per sequence.  Per iteration and frame, A_t and g_t are scat_mano_fit's; smoothness adds c_t d_i to the diagonal of A_t
 * (c_t the number of neighbours of frame t: 1 at the ends, 2 inside, 0 for T = 1) and
 * d_i ((p_t - p_t-1) + (p_t - p_t+1))_i to g_t, each bracket only where that neighbour exists; the off-diagonal blocks
 * are -D, D = diag(d).  Marquardt damping multiplies the full diagonal, smoothness included, by 1 + lambda.  The
 * block-tridiagonal system is solved exactly by block Cholesky along t:
 *     forward    L_0 = chol(H_0),  M_t = -D L_t-1^-T,  L_t = chol(H_t - M_t M_t^T),  y_t = L_t^-1 (g_t - M_t y_t-1)
 *     backward   x_t = L_t^-T (y_t - M_t+1^T x_t+1),  delta = -x.
 * A frozen unknown (free_mask, the same mask for every frame) is a unit row in every H_t with a zero in g_t and in the D
 * of the system; its smoothness term still counts in the cost, where it is a constant.  A pivot of any frame that is not
 * positive or not finite is a rejection.  The trial is accepted only if every trial unknown of every frame is finite and
 * cost_s drops; then lambda /= 10, otherwise lambda *= 10 (within 1e-12..1e12).  There is no data-dependent exit and no
 * floating-point atomic.  Every sum runs in a fixed order: frames ascend, within a frame the order is scat_mano_fit's,
 * then come the smoothness terms, t ascending, i ascending.  The same call gives the same bits, and the bits of a
 * sequence depend neither on S nor on its index.
 */
#ifndef SCAT_MANO_FIT_SEQ_H
#define SCAT_MANO_FIT_SEQ_H
#include <stdint.h>

#include "scat_mano_fit.h"
#ifdef __cplusplus
extern "C" {
#endif

#define SCAT_FIT_SEQ_MAX_T 256

/* Bytes of workspace scat_mano_fit_seq needs for S sequences of T frames; 0 for S < 1 or T outside
 * 1..SCAT_FIT_SEQ_MAX_T, which the launch refuses.  Per frame: L_t with y_t as its 63rd row (63 x 62 floats), M_t^T
 * (62 x 62), and two copies of the 62 unknowns (current and trial).  Each sequence's part is written and read back by
 * the one workgroup that owns the sequence, and holds nothing of use after the call. */
int64_t scat_mano_fit_seq_ws(int S, int T);

/* targets[S,T,21,3], weights[S,T,21] (null: all ones), joint_map[21] -> p[S,T,62], cost[S], accepted[S].  `iters`
 * iterations (1..SCAT_FIT_MAX_ITERS) inside one launch, one workgroup per sequence, T in 1..SCAT_FIT_SEQ_MAX_T.
 * ws: 16-byte aligned, at least scat_mano_fit_seq_ws(S, T) bytes; otherwise SCAT_E_WORKSPACE, before any HIP call.
 *   init = 0     p is read: the caller's start.  p is written only after an accepted step.
 *   init = 1     p is written only: poses = betas = 0 and, frame by frame, scat_mano_fit's Procrustes start.  For
 *                t >= 1, rots_t is replaced by the same rotation's r (1 - 2 pi / |r|) when that is closer to rots_t-1,
 *                so that a track that crosses the angle pi pays no spurious penalty.  A frame of total weight zero
 *                takes the start of the frame before it; frame 0 takes that of the first frame that has weight; if no
 *                frame has weight the start is zeros.
 * A frame whose weights are all zero is legal whatever its finite targets: it has no data term, is bridged by its
 * neighbours through the smoothness, and its targets do not reach the result.  This is also how a short clip is padded.
 * A sequence with a target or weight that is not finite, or with a negative weight, in any frame is not fitted:
 * cost = +inf, accepted = 0, and p is its start (init = 0: the caller's, untouched; init = 1: zeros).  The other
 * sequences are not affected.
 *   s_rots .. s_scale   the smoothness weights, each finite and not negative (UNITS above).
 *   cost         cost_s at the returned p; accepted: the number of accepted steps, 0..iters. */
int scat_mano_fit_seq(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                      const float* hands_mean, const float* targets, const float* weights, const int* joint_map, float* p,
                      float* cost, int* accepted, void* ws, int64_t ws_bytes, int S, int T, int V, uint64_t parents, int tip0,
                      int tip1, int tip2, int tip3, int tip4, int iters, int init, float lambda0, float w_pose, float w_beta,
                      float s_rots, float s_poses, float s_betas, float s_trans, float s_scale, uint64_t free_mask,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
