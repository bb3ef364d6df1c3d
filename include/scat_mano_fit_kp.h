/* libscat_hip — C ABI of the on-device MANO fit to keypoints: scat_mano_fit (scat_mano_fit.h) with a 2-D reprojection
 * term, a robust loss and joint limits (public header of the one library; the conventions are those of scat_mano_fit.h:
 * device pointers owned by the caller at any 4-byte-aligned address, explicit sizes, hipStream_t as void* last,
 * stream-ordered, never synchronises, never allocates, retains no pointer, returns 0 or a negative SCAT_E_* code).  No
 * workspace is needed.  The model arrays, V, parents, tip0..4, joint_map (CLAMPED to 0..20 on the device) and the joints
 * x(rots, poses, betas)[21][3] are those of scat_mano_fit.h.
 *
 * The unknowns of one hand are p[65] = rots[3] ++ poses[45] ++ betas[10] ++ trans[3] ++ log_scale[1] ++ cam[3], the first
 * 62 in scat_mano_fit's order, cam = (cs, ctx, cty) the weak-perspective camera [s, tx, ty] as the networks predict it
 * (stored as it is, not as a logarithm).  With
 *     m_j = exp(log_scale) x[joint_map[j]] + trans                                       the 3-D model joint
 *     u_j = ( cs (m_j.x + ctx) half_w + half_w ,  cs (m_j.y + cty) half_h + half_h )     its projection, pixels
 * the cost is
 *     sum_j w3_j rho(|m_j - X_j|^2; sigma3) + sum_j w2_j rho(|u_j - U_j|^2; sigma2) + w_pose |poses|^2 + w_beta |betas|^2
 *       + w_limit sum_i ( max(0, poses_i - hi_i)^2 + max(0, lo_i - poses_i)^2 )
 * with Geman-McClure rho(e; sigma) = sigma^2 e / (sigma^2 + e) on a joint's squared distance; sigma = 0 is the plain e.
 * UNITS: the 3-D term is in the targets' unit squared, the 2-D term in pixels squared, and the caller balances them with
 * weights2: for targets in metres, weights2 = 1e-6 makes a pixel count like a millimetre.
 */
#ifndef SCAT_MANO_FIT_KP_H
#define SCAT_MANO_FIT_KP_H
#include <stdint.h>

#include "scat_mano_fit.h"
#ifdef __cplusplus
extern "C" {
#endif

#define SCAT_FIT_KP_UNKNOWNS 65

/* targets3[B,21,3] / weights3[B,21], targets2[B,21,2] / weights2[B,21], joint_map[21], pose_lo[45] / pose_hi[45] ->
 * p[B,65], cost[B], accepted[B].  `iters` Levenberg-Marquardt iterations inside one launch, one workgroup per sample,
 * everything in LDS.
 *   targets3, targets2   a null pointer leaves the term out; at least one must be given.  weights without their targets
 *                are refused; a null weights pointer of a present term means all ones.
 *   pose_lo, pose_hi     both null (no limits) or both given; an entry that is not finite is no limit.
 *   init = 0     p is read: the caller's start.
 *   init = 1     p is written only: poses = betas = 0 and a closed-form start, in fp64 by one thread.
 *                With a 3-D term of positive total weight: rots, trans, log_scale from scat_mano_fit's weighted
 *                Procrustes, and the camera from the weighted least squares of y = (U - half) / half on a = m.xy at that
 *                start with one isotropic scale: cs = sum w2 (a - abar).(y - ybar) / sum w2 |a - abar|^2,
 *                ct = ybar / cs - abar; without a 2-D term, or with cs outside (1e-30, 1e30), the camera is (1, 0, 0).
 *                Otherwise (2-D only): trans = 0, log_scale = 0, and of the two rotations Rz(phi) and Rz(phi) Ry(pi) the
 *                one whose weighted complex least squares y ~ z a + t on the zero-pose joints' xy (a = (C x0).xy, C = I or
 *                Ry(pi), phi = arg z) leaves the smaller residual, a tie going to the first; rots is its axis-angle by
 *                scat_mano_fit's quaternion path, cs = |z|, ct = t / cs.  The rotation out of the image plane is left
 *                to the iterations.  With |z| outside (1e-30, 1e30): rots = 0, camera (1, 0, 0).
 * Each iteration is scat_mano_fit's with iteratively reweighted rows: a joint's rows get the weight
 * w (sigma^2 / (sigma^2 + e))^2 at the current p, which is w rho'(e), so that g is half the gradient of the cost; there
 * is no second-order term.  An active limit adds w_limit to its diagonal entry and w_limit (poses_i - hi_i), or
 * -w_limit (lo_i - poses_i), to g.  A + lambda diag(A), Cholesky and solve; the trial is accepted only if every trial
 * unknown is finite and the robust cost as written above drops; lambda /= 10 or *= 10 within 1e-12..1e12; a failed
 * factorisation is a rejection.  No data-dependent exit, no floating-point atomic, every sum in a fixed order (3-D joints
 * ascending, then 2-D joints ascending, then the priors, then the limits): the same call gives the same bits.
 *   free_mask    bit i set: unknown i < 62 is solved for; clear: it keeps its initial bits.  Bits 62..63 must be clear.
 *   free_cam     the same for the camera: bit 0 cs, bit 1 ctx, bit 2 cty.  With no 2-D term the camera has no rows: pass 0.
 *                With no 3-D term trans and log_scale are a gauge of the camera (and trans.z has no rows): freeze them.
 *   cost         the cost at the returned p; accepted: the number of accepted steps, 0..iters.
 * A sample with a target or weight of a present term that is not finite, or with a negative weight, is not fitted:
 * cost = +inf, accepted = 0, and p is its initial value (init = 0: the caller's, untouched; init = 1: zeros and the
 * camera (1, 0, 0)).  With init = 0, p is written only after an accepted step.  A joint of weight zero does not count,
 * whatever its finite target. */
int scat_mano_fit_kp(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                     const float* hands_mean, const float* targets3, const float* weights3, const float* targets2,
                     const float* weights2, const int* joint_map, const float* pose_lo, const float* pose_hi, float* p,
                     float* cost, int* accepted, int B, int V, uint64_t parents, int tip0, int tip1, int tip2, int tip3,
                     int tip4, int iters, int init, float lambda0, float w_pose, float w_beta, float w_limit, float sigma3,
                     float sigma2, float half_w, float half_h, uint64_t free_mask, int free_cam, void* stream);

#ifdef __cplusplus
}
#endif
#endif
