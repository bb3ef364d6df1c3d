/* libscat_hip — C ABI of the on-device MANO fit to a track of keypoints: scat_mano_fit_kp's problem (scat_mano_fit_kp.h:
 * 3-D joints, 2-D keypoints through a weak-perspective camera, a Geman-McClure loss, joint limits) over the T frames of a
 * sequence, coupled as scat_mano_fit_seq couples them (scat_mano_fit_seq.h) and solved as one Levenberg-Marquardt (public
 * header of the one library; the conventions are those of scat_mano_fit_seq.h: device pointers owned by the caller,
 * explicit sizes, hipStream_t as void* last, stream-ordered, never synchronises, never allocates, retains no pointer,
 * returns 0 or a negative SCAT_E_* code).  The model arrays, V, parents, tip0..4, joint_map (CLAMPED to 0..20 on the
 * device) are scat_mano_fit's, and the 65 unknowns of one frame are scat_mano_fit_kp's,
 *     p[65] = rots[3] ++ poses[45] ++ betas[10] ++ trans[3] ++ log_scale[1] ++ cam[3],   cam = (cs, ctx, cty).
 * Every operand but the workspace may sit at any 4-byte-aligned address.
 *
 * With cost_kp(p_t; frame t) the cost that scat_mano_fit_kp.h writes out (the 3-D term, the 2-D term through cam, rho with
 * sigma3 / sigma2, w_pose, w_beta, and the limits with w_limit), the cost of sequence s is
 *     cost_s = sum_t cost_kp(p_t; frame t) + sum_{t >= 1} sum_i d_i (p_t,i - p_t-1,i)^2,
 * d_i the smoothness weight of unknown i's group: s_rots, s_poses, s_betas, s_trans, s_scale, s_cs (the camera scale cs)
 * and s_ct (ctx and cty).  All seven zero decouples the frames: every frame is then scat_mano_fit_kp's problem, under one
 * shared lambda and one accept / reject.
 *
 * UNITS.  The 3-D term is in the 3-D targets' unit squared, the 2-D term in pixels squared, balanced by weights2 as in
 * scat_mano_fit_kp.h.  A smoothness weight multiplies a squared difference in the unknown's OWN unit: radians squared for
 * s_rots and s_poses (on the axis-angle numbers themselves, not on the rotations they stand for; init = 1 starts without
 * a 2 pi jump), the shape coefficients' unit squared for s_betas, the 3-D targets' unit squared for s_trans, the square of
 * a log-ratio (a pure number) for s_scale, a pure number squared for s_cs (cs is stored as it is, not as a logarithm),
 * and the 3-D targets' unit squared for s_ct (ctx and cty are added to the model joints).  For targets in metres
 * s_rots = 1e-4 counts 0.1 rad per frame like a 1 mm residual.  A CONSTANT SHAPE over the track is obtained with a large
 * s_betas; there is no hard constraint.
 *
 * The solver is one Levenberg-Marquardt over the whole sequence: one lambda, one accept / reject and one accepted count
 * per sequence.  Per iteration and frame, A_t and g_t are scat_mano_fit_kp's, with the IRLS row weights w rho'(e) taken
 * at the current iterate and the active limits on the diagonal and in g.  Smoothness enters exactly as in
 * scat_mano_fit_seq, now over 65 unknowns: c_t d_i on the diagonal of A_t (c_t the number of neighbours of frame t),
 * d_i ((p_t - p_t-1) + (p_t - p_t+1))_i in g_t, each bracket only where that neighbour exists, and -D = -diag(d) beside
 * the diagonal.  Marquardt damping multiplies the full diagonal, smoothness included, by 1 + lambda.  The block-tridiagonal
 * system is solved exactly by block Cholesky along t:
 *     forward    L_0 = chol(H_0),  M_t = -D L_t-1^-T,  L_t = chol(H_t - M_t M_t^T),  y_t = L_t^-1 (g_t - M_t y_t-1)
 *     backward   x_t = L_t^-T (y_t - M_t+1^T x_t+1),  delta = -x.
 * A frozen unknown (free_mask for the first 62, free_cam for cs, ctx, cty; the same for every frame) is a unit row in
 * every H_t with a zero in g_t and in the D of the system; its smoothness term still counts in the cost, where it is a
 * constant.  A step is accepted only if every pivot of every frame is positive, every pivot of every frame is finite,
 * every trial unknown of every frame is finite, and cost_s, the robust cost as written above, drops; then lambda /= 10,
 * otherwise lambda *= 10 (within 1e-12..1e12).  There is no second-order robust term, no data-dependent exit and no
 * floating-point atomic.  Every sum runs in a fixed order: frames ascend, within a frame the order is scat_mano_fit_kp's,
 * then come the smoothness terms, t ascending, i ascending.  The same call gives the same bits, and the bits of a
 * sequence depend neither on S nor on its index.
 */
#ifndef SCAT_MANO_FIT_SEQ_KP_H
#define SCAT_MANO_FIT_SEQ_KP_H
#include <stdint.h>

#include "scat_mano_fit_kp.h"
#include "scat_mano_fit_seq.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace scat_mano_fit_seq_kp needs for S sequences of T frames; 0 for S < 1 or T outside
 * 1..SCAT_FIT_SEQ_MAX_T, which the launch refuses.  Per frame: L_t with y_t as its 66th row (66 x 65 floats), M_t^T
 * (65 x 65), and two copies of the 65 unknowns (current and trial).  Each sequence's part is written and read back by
 * the one workgroup that owns the sequence, and holds nothing of use after the call. */
int64_t scat_mano_fit_seq_kp_ws(int S, int T);

/* targets3[S,T,21,3] / weights3[S,T,21], targets2[S,T,21,2] / weights2[S,T,21], joint_map[21], pose_lo[45] / pose_hi[45]
 * -> p[S,T,65], cost[S], accepted[S].  `iters` iterations (1..SCAT_FIT_MAX_ITERS) inside one launch, one workgroup per
 * sequence, T in 1..SCAT_FIT_SEQ_MAX_T.  Every check, the workspace's size and alignment included, comes before any HIP
 * call.
 *   targets3, targets2   as in scat_mano_fit_kp: a null pointer leaves the term out; at least one must be given; weights
 *                without their targets are refused; a null weights pointer of a present term means all ones.
 *   pose_lo, pose_hi     both null (no limits) or both given; an entry that is not finite is no limit.
 *   ws           16-byte aligned, at least scat_mano_fit_seq_kp_ws(S, T) bytes; otherwise SCAT_E_WORKSPACE.
 *   init = 0     p is read: the caller's start.  p is written only after an accepted step.
 *   init = 1     p is written only: frame by frame scat_mano_fit_kp's closed-form start (poses = betas = 0; Procrustes
 *                and the camera's least squares where the frame has 3-D weight, the better of the two in-plane
 *                candidates Rz(phi), Rz(phi) Ry(pi) from 2-D alone), then scat_mano_fit_seq's scan: a frame whose total
 *                weight sum w3 + sum w2 is zero takes the rots, trans, log_scale and camera of the frame before it,
 *                frame 0 those of the first frame that has weight (if no frame has weight every start is zeros and the
 *                camera (1, 0, 0)); and for t >= 1 rots_t is replaced by the same rotation's r (1 - 2 pi / |r|) when
 *                that is closer to rots_t-1.  The per-frame choice between the two 2-D-only candidates is NOT revisited:
 *                each frame keeps the candidate its own least squares preferred, the scan does not make the choice
 *                consistent along the track.
 * A frame whose weights are all zero is legal whatever its finite targets: it has no data term, is bridged by its
 * neighbours through the smoothness, and its targets do not reach the result.  This is also how a short clip is padded.
 * A sequence with a target or weight of a present term that is not finite, or with a negative weight, in any frame is
 * not fitted: cost = +inf, accepted = 0, and p is its start (init = 0: the caller's, untouched; init = 1: zeros and the
 * camera (1, 0, 0) in every frame).  The other sequences are not affected.
 *   w_limit, sigma3, sigma2, half_w, half_h   scat_mano_fit_kp's.
 *   s_rots .. s_ct   the seven smoothness weights, each finite and not negative (UNITS above).
 *   free_mask    bit i set: unknown i < 62 is solved for in every frame; clear: it keeps its initial bits.  Bits 62..63
 *                must be clear.
 *   free_cam     the same for the camera, 0..7: bit 0 cs, bit 1 ctx, bit 2 cty.  With no 2-D term the camera has no rows:
 *                pass 0.  With no 3-D term trans and log_scale are a gauge of the camera: freeze them.
 *   cost         cost_s at the returned p; accepted: the number of accepted steps, 0..iters. */
int scat_mano_fit_seq_kp(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                         const float* hands_mean, const float* targets3, const float* weights3, const float* targets2,
                         const float* weights2, const int* joint_map, const float* pose_lo, const float* pose_hi, float* p,
                         float* cost, int* accepted, void* ws, int64_t ws_bytes, int S, int T, int V, uint64_t parents,
                         int tip0, int tip1, int tip2, int tip3, int tip4, int iters, int init, float lambda0, float w_pose,
                         float w_beta, float w_limit, float sigma3, float sigma2, float half_w, float half_h, float s_rots,
                         float s_poses, float s_betas, float s_trans, float s_scale, float s_cs, float s_ct,
                         uint64_t free_mask, int free_cam, void* stream);

#ifdef __cplusplus
}
#endif
#endif
