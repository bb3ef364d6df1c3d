/* libscat_hip — C ABI of the on-device MANO fit to 2-D keypoints seen by C calibrated pinhole cameras, and of the
 * triangulation that makes its closed-form start (public header of the one library; the conventions are those of
 * scat_mano_fit.h: device pointers owned by the caller at any 4-byte-aligned address, explicit sizes, hipStream_t as void*
 * last, stream-ordered, never synchronises, never allocates, retains no pointer, returns 0 or a negative SCAT_E_* code,
 * every check before any HIP call).  No workspace is needed.  The model arrays, V, parents, tip0..4, joint_map (CLAMPED
 * to 0..20 on the device) and the joints x(rots, poses, betas)[21][3] are those of scat_mano_fit.h.
 *
 * The unknowns of one hand are scat_mano_fit's p[62] = rots[3] ++ poses[45] ++ betas[10] ++ trans[3] ++ log_scale[1].
 * There are no camera unknowns: the cameras are data.
 *
 * Cameras are cams[Bc, C, 16] in fp32 with Bc in {1, B}, passed as cam_batch: cam_batch = 1 is one rig for the whole
 * batch and cam_batch = B is one rig per sample.  Each camera is R[9] row-major, then t[3], then fx, fy, cx, cy.
 * 1 <= C <= SCAT_FIT_VIEWS_MAX_C = 8.  With m_j = exp(log_scale) x[joint_map[j]] + trans, as in scat_mano_fit_kp.h:
 *     q_cj = R_c m_j + t_c                                      the joint in camera c, which looks along +z
 *     u_cj = ( fx q.x / q.z + cx ,  fy q.y / q.z + cy )         pixels
 *     cost = sum_j sum_c w_cj rho(|u_cj - U_cj|^2; sigma2) + w_pose |poses|^2 + w_beta |betas|^2
 *            + w_limit sum_i ( max(0, poses_i - hi_i)^2 + max(0, lo_i - poses_i)^2 )
 * with rho, the IRLS row weight wi = w rho'(e) and the limits those of scat_mano_fit_kp.h (Geman-McClure
 * rho(e; sigma) = sigma^2 e / (sigma^2 + e) on a view-joint's squared distance; sigma2 = 0 is the plain e).  A view-joint
 * of weight zero does not count, whatever its finite target: this is how a joint that a view does not see is passed.
 * UNITS: the data term is in pixels squared, summed over up to 21 C view-joints, and w_pose, w_beta and w_limit multiply
 * squared radians and squared shape coefficients beside it.  A hand of size s at depth z moves by fx s / z pixels per
 * radian, about 100 px for fx = 600, s = 0.08 m, z = 0.5 m, so a prior that counts 0.1 rad like a pixel is w_pose = 1e2;
 * scat_mano_fit's 1e-6, chosen beside metres squared, is no prior at all here.
 *
 * The 42 C rows of the Jacobian are not stored.  With D = [[fx / q.z, 0, -fx q.x / q.z^2], [0, fy / q.z, -fy q.y / q.z^2]]
 * and P_cj = D R_c (2 x 3), r_cj = u_cj - U_cj:
 *     M_j = sum_c wi_cj P^T P   (3 x 3)           h_j = sum_c wi_cj P^T r_cj   (3)
 *     A   = sum_j G_j^T M_j G_j                   g   = sum_j G_j^T h_j
 * where G_j is rows 3 j .. 3 j + 2 of the 63 x 62 Jacobian of m (the similarity's columns included): the whole multi-view
 * term is a 3 x 3 metric per joint, and neither the assembly nor the LDS grow with C.  Every sum runs in a fixed order:
 * views ascending inside a joint, joints ascending, then the priors, then the limits.  No atomic, no data-dependent exit:
 * the same call gives the same bits.
 *
 * BEHIND THE CAMERA.  z_near > 0.  If a view-joint of positive weight has q.z <= z_near at the start p, the sample is not
 * fitted: cost = +inf, accepted = 0, p its start.  A trial with such a view-joint is rejected, like a failed factorisation.
 * A sample with a keypoint, weight or camera entry that is not finite, or with a negative weight, is not fitted either:
 * cost = +inf, accepted = 0, p its initial value (init = 0: the caller's, untouched; init = 1: zeros).
 */
#ifndef SCAT_MANO_FIT_VIEWS_H
#define SCAT_MANO_FIT_VIEWS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCAT_FIT_VIEWS_MAX_C 8
#define SCAT_FIT_VIEWS_CAM 16 /* floats per camera: R[9] row-major, t[3], fx, fy, cx, cy */

/* cams[cam_batch,C,16], targets2[B,C,21,2] / weights2[B,C,21] or null (all ones), joint_map[21], pose_lo[45] / pose_hi[45]
 * (both null: no limits; an entry that is not finite is no limit) -> p[B,62], cost[B], accepted[B].  `iters`
 * Levenberg-Marquardt iterations inside one launch, one workgroup per hand, everything in LDS.
 *   init = 0     p is read: the caller's start.  The only way in for C = 1, where depth and scale cannot be told apart
 *                and nothing can be triangulated.
 *   init = 1     p is written only: poses = betas = 0, and rots, trans, log_scale from scat_mano_fit's weighted Procrustes
 *                of the zero-pose joints onto the joints that scat_triangulate (below, the same device function) gives,
 *                rounded to fp32, with weight 1 for a triangulated joint and 0 for the others.  With fewer than 3
 *                triangulated joints the sample is not fitted: cost = +inf, accepted = 0, p = zeros.
 * Damping (A + lambda diag(A)), Cholesky, accept / reject (the trial is taken only if every trial unknown is finite and
 * the robust cost as written above drops), lambda /= 10 or *= 10 within 1e-12..1e12, "p is written only after an accepted
 * step" with init = 0, and the outputs are scat_mano_fit's; an active limit adds to A and g as in scat_mano_fit_kp.h.
 *   free_mask    bit i set: unknown i < 62 is solved for; clear: it keeps its initial bits.  Bits 62..63 must be clear.
 *   cost         the cost at the returned p; accepted: the number of accepted steps, 0..iters. */
int scat_mano_fit_views(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                        const float* hands_mean, const float* cams, int cam_batch, const float* targets2,
                        const float* weights2, const int* joint_map, const float* pose_lo, const float* pose_hi, float* p,
                        float* cost, int* accepted, int B, int C, int V, uint64_t parents, int tip0, int tip1, int tip2,
                        int tip3, int tip4, int iters, int init, float lambda0, float w_pose, float w_beta, float w_limit,
                        float sigma2, float z_near, uint64_t free_mask, void* stream);

/* cams[cam_batch,C,16], targets2[B,C,21,2], weights2[B,C,21] or null (all ones) -> points[B,21,3], valid[B,21] int32.  Per
 * joint, in fp64, by one thread: the rays o_c = -R_c^T t_c, d_c = normalise(R_c^T ((U.x - cx) / fx, (U.y - cy) / fy, 1)) of
 * its views of positive weight, and the point X that minimises sum_c w_c |(I - d_c d_c^T)(X - o_c)|^2, a 3 x 3 symmetric
 * system solved by Cholesky; X is rounded to fp32.  A joint is triangulated iff
 *   - at least two of its views have positive weight,
 *   - every pivot (a squared diagonal entry of the factor) exceeds 1e-6 x the trace of the system, and
 *   - X has q.z > z_near in each contributing view.
 * For two rays of equal weight at the angle theta the system is w (2 I - d_1 d_1^T - d_2 d_2^T) with the eigenvalues
 * 2 w, w (1 + cos theta) and w (1 - cos theta) ~ w theta^2 / 2 and the trace 4 w: the smallest eigenvalue over the trace
 * is theta^2 / 8, and no pivot is smaller than the smallest eigenvalue.  So 1e-6 refuses only rays closer than sqrt(8e-6),
 * about 3 mrad, and always refuses parallel ones; between the two it depends on where the rays point, the last pivot being
 * the smallest eigenvalue over the squared z component of its direction.
 * An untriangulated joint gets valid = 0 and points = 0; every word of both outputs is written.  In a sample with a
 * keypoint, weight or camera entry that is not finite, or a negative weight, no joint is triangulated. */
int scat_triangulate(const float* cams, int cam_batch, const float* targets2, const float* weights2, float* points,
                     int* valid, int B, int C, float z_near, void* stream);

#ifdef __cplusplus
}
#endif
#endif
