/* libscat_hip — C ABI of the on-device MANO fit to a track of 2-D keypoints seen by C calibrated pinhole cameras: the
 * frame of scat_mano_fit_views.h inside the track of scat_mano_fit_seq.h (public header of the one library; the
 * conventions are those of scat_mano_fit.h: device pointers owned by the caller, explicit sizes, hipStream_t as void*
 * last, stream-ordered, never synchronises, never allocates, retains no pointer, returns 0 or a negative SCAT_E_* code,
 * every check before any HIP call).  The model arrays, V, parents, tip0..4, joint_map (CLAMPED to 0..20 on the device) and
 * the 62 unknowns of one frame,
 *     p[62] = rots[3] ++ poses[45] ++ betas[10] ++ trans[3] ++ log_scale[1],
 * are scat_mano_fit's.  Every operand but the workspace may sit at any 4-byte-aligned address.  There are no camera
 * unknowns: the cameras are data, and the rig is fixed along a track.
 *
 * Cameras are cams[cam_batch, C, 16] in scat_mano_fit_views.h's layout (R[9] row-major, t[3], fx, fy, cx, cy), with
 * cam_batch = 1 (one rig for all sequences) or cam_batch = S (one rig per sequence), 1 <= C <= SCAT_FIT_VIEWS_MAX_C.
 * With cost_views(p_t; frame t) exactly the cost that scat_mano_fit_views.h writes for the keypoints U_tcj and weights
 * w_tcj of frame t (the pixel term with Geman-McClure rho(e; sigma2), w_pose |poses|^2, w_beta |betas|^2 and the limits),
 *     cost_s = sum_t cost_views(p_t; frame t) + sum_{t >= 1} sum_i d_i (p_t,i - p_t-1,i)^2,
 * d_i the smoothness weight of unknown i's group, scat_mano_fit_seq.h's five: s_rots, s_poses, s_betas, s_trans, s_scale.
 * All five zero decouples the frames: every frame is then scat_mano_fit_views' problem, under one shared lambda and one
 * accept / reject.
 *
 * UNITS.  The data term is in pixels squared, summed over up to 21 C view-joints per frame; w_pose, w_beta and w_limit
 * multiply squared radians and squared shape coefficients beside it as in scat_mano_fit_views.h (w_pose = 1e2 counts
 * 0.1 rad like a pixel).  A smoothness weight multiplies a squared difference in the unknown's OWN unit: radians squared
 * for s_rots and s_poses, the shape coefficients' unit squared for s_betas, metres squared for s_trans (the cameras'
 * unit of length), and the square of a log-ratio for s_scale.  A hand of size s at depth z moves by fx s / z pixels per
 * radian and by fx / z pixels per metre: about 100 px / rad and 1200 px / m for fx = 600, s = 0.08 m, z = 0.5 m.  So a
 * step of 0.1 rad per frame counts like one view-joint's residual of a pixel at s_rots = 1e2, and a step of 1 mm per
 * frame does at s_trans = 1e6; scat_mano_fit_seq's figures, chosen beside metres squared, are no smoothness at all here.
 * The penalty is on the axis-angle numbers themselves, as scat_mano_fit_seq.h explains; init = 1 starts without a jump.
 *
 * The solver is scat_mano_fit_seq's, word for word: one Levenberg-Marquardt over the whole sequence, one lambda, one
 * accept / reject and one accepted count per sequence.  Per iteration and frame, A_t and g_t are scat_mano_fit_views':
 * from the per-joint metric M_j and h_j, A_t = sum_j G_j^T M_j G_j and g_t = sum_j G_j^T h_j, views ascending inside a
 * joint, joints ascending, then the priors, then the limits.  Smoothness adds c_t d_i to the diagonal of A_t (c_t the
 * number of neighbours of frame t) and d_i ((p_t - p_t-1) + (p_t - p_t+1))_i to g_t, each bracket only where that
 * neighbour exists; the off-diagonal blocks are -D.  Marquardt damping multiplies the full diagonal, smoothness included,
 * by 1 + lambda.  The block-tridiagonal system is solved exactly by block Cholesky along t (scat_mano_fit_seq.h has the
 * recurrences).  A frozen unknown (free_mask, the same for every frame) is a unit row in every H_t with a zero in g_t and
 * in the D of the system; its smoothness term still counts in the cost.  A pivot of any frame that is not positive or not
 * finite is a rejection.  The trial is accepted only if every trial unknown of every frame is finite and cost_s drops;
 * then lambda /= 10, otherwise lambda *= 10 (within 1e-12..1e12).  No atomic, no data-dependent exit.  Every sum runs in
 * a fixed order: frames ascend, within a frame the order is scat_mano_fit_views', then come the smoothness terms, t
 * ascending, i ascending.  The same call gives the same bits, and the bits of a sequence depend neither on S nor on its
 * index.
 *
 * BEHIND THE CAMERA.  z_near > 0.  If a view-joint of positive weight has q.z <= z_near at the start, in any frame, the
 * sequence is not fitted: cost = +inf, accepted = 0, and p is its start (init = 0: the caller's, untouched; init = 1: the
 * scanned closed-form start below).  A trial with such a view-joint in any frame is rejected, like a failed pivot.
 * A sequence with a keypoint, weight or camera entry that is not finite, or with a negative weight, in any frame is not
 * fitted either: cost = +inf, accepted = 0, p its initial value (init = 0: the caller's, untouched; init = 1: zeros).
 * The other sequences are not affected.
 *
 * A frame whose weights are all zero is legal whatever its finite keypoints: it has no data term and is bridged by its
 * neighbours through the smoothness, which is also how a short clip is padded.  A frame with weight in only one view is
 * legal too and its rows count, although alone it has no closed-form start and its depth is not observable.
 */
#ifndef SCAT_MANO_FIT_SEQ_VIEWS_H
#define SCAT_MANO_FIT_SEQ_VIEWS_H
#include <stdint.h>

#include "../include/scat_mano_fit_seq.h"
#include "scat_mano_fit_views.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace scat_mano_fit_seq_views needs for S sequences of T frames: scat_mano_fit_seq_ws(S, T), whose layout
 * it shares; 0 for S < 1 or T outside 1..SCAT_FIT_SEQ_MAX_T, which the launch refuses. */
int64_t scat_mano_fit_seq_views_ws(int S, int T);

/* cams[cam_batch,C,16], targets2[S,T,C,21,2] / weights2[S,T,C,21] or null (all ones), joint_map[21], pose_lo[45] /
 * pose_hi[45] (both null: no limits; an entry that is not finite is no limit) -> p[S,T,62], cost[S], accepted[S].
 * `iters` iterations (1..SCAT_FIT_MAX_ITERS) inside one launch, one workgroup per sequence, T in 1..SCAT_FIT_SEQ_MAX_T.
 * ws: 16-byte aligned, at least scat_mano_fit_seq_views_ws(S, T) bytes; otherwise SCAT_E_WORKSPACE, before any HIP call.
 *   init = 0     p is read: the caller's start.  p is written only after an accepted step.  The only way in for C = 1.
 *   init = 1     p is written only.  A launch before the walk, one workgroup per frame, gives every frame
 *                scat_mano_fit_views' start (poses = betas = 0; rots, trans, log_scale from the Procrustes onto the
 *                triangulated joints) if at least 3 of its joints are triangulated.  A frame without such a start takes
 *                rots, trans, log_scale of the frame before it; frame 0 takes those of the first frame that has one;
 *                for t >= 1 rots_t is unwrapped against rots_t-1 as in scat_mano_fit_seq.h.  If no frame of a sequence
 *                has a start the sequence is not fitted: cost = +inf, accepted = 0, p = zeros.  C = 1 is refused with
 *                SCAT_E_ARG before any launch.
 *   s_rots .. s_scale   the smoothness weights, each finite and not negative (UNITS above).
 *   free_mask    bit i set: unknown i < 62 is solved for in every frame; clear: it keeps its initial bits.
 *   cost         cost_s at the returned p; accepted: the number of accepted steps, 0..iters. */
int scat_mano_fit_seq_views(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                            const float* hands_mean, const float* cams, int cam_batch, const float* targets2,
                            const float* weights2, const int* joint_map, const float* pose_lo, const float* pose_hi, float* p,
                            float* cost, int* accepted, void* ws, int64_t ws_bytes, int S, int T, int C, int V,
                            uint64_t parents, int tip0, int tip1, int tip2, int tip3, int tip4, int iters, int init,
                            float lambda0, float w_pose, float w_beta, float w_limit, float sigma2, float z_near, float s_rots,
                            float s_poses, float s_betas, float s_trans, float s_scale, uint64_t free_mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif
