/* libscat_hip — C ABI of the on-device MANO fit: the inverse of the MANO layer (public header of the one library; the
 * conventions are those of scat_mano.h: device pointers owned by the caller, explicit sizes, hipStream_t as void* last,
 * stream-ordered, never synchronises, never allocates, retains no pointer, returns 0 or a negative SCAT_E_* code).  No
 * workspace is needed.  The model arrays (blend, joint_t, joint_s, weights_t, hands_mean), V, parents and tip0..4 are
 * those of scat_mano.h, and so are the joints: x(rots, poses, betas)[21][3] are the first 21 rows of scat_mano_fwd's
 * output, joint 1 at the origin.  Every operand may sit at any 4-byte-aligned address.
 *
 * The unknowns of one hand are p[62] = rots[3] ++ poses[45] ++ betas[10] ++ trans[3] ++ log_scale[1], the model joints
 *     model_j = exp(log_scale) x[joint_map[j]] + trans,                      j = 0..20
 * and the cost
 *     sum_j w[j] |model_j - target_j|^2 + w_pose |poses|^2 + w_beta |betas|^2.
 * joint_map[21] is a device array of ints, a permutation of 0..20 by contract.  It is read on the device, so it cannot be
 * refused on the host: every entry is CLAMPED to 0..20 there, and an array that is no permutation fits a repeated joint
 * instead of reading out of bounds.
 */
#ifndef SCAT_MANO_FIT_H
#define SCAT_MANO_FIT_H
#include <stdint.h>

#include "scat_mano.h"
#ifdef __cplusplus
extern "C" {
#endif

#define SCAT_FIT_UNKNOWNS 62
#define SCAT_FIT_MODEL_UNKNOWNS 58
#define SCAT_FIT_MAX_ITERS 64

/* rots[B,3], poses[B,45], betas[B,10] -> joints[B,21,3] and jac[B,63,58] = d joints / d (rots, poses, betas), row
 * 3 j + c, column order rots, poses, betas.  One launch, one workgroup per sample.  Joints only: the folded joint arrays,
 * the chain, and the blend and skinning of the five tip vertices; no pass over the mesh.  Forward mode: a pose parameter
 * of joint k moves k's subtree by Omega (t_i - t_k) with Omega = RG_parent(k) dR_k RG_k^T, and a tip through the joints
 * it is skinned to and through posedirs.  Rodrigues and its derivative are the t = theta^2 forms of the layer: finite
 * at zero, no division by theta. */
int scat_mano_joints_jac(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                         const float* hands_mean, const float* rots, const float* poses, const float* betas,
                         float* joints, float* jac, int B, int V, uint64_t parents, int tip0, int tip1, int tip2, int tip3,
                         int tip4, void* stream);

/* targets[B,21,3], weights[B,21] (null: all ones), joint_map[21] -> p[B,62], cost[B], accepted[B].  `iters`
 * Levenberg-Marquardt iterations inside one launch, one workgroup per sample, everything in LDS.
 *   init = 0     p is read: the caller's start.
 *   init = 1     p is written only: poses = betas = 0, and rots, trans and log_scale from the weighted similarity
 *                Procrustes of the zero-pose model joints onto the targets (Horn's quaternion in fp64; the axis-angle is
 *                2 atan2(|v|, w) v / |v| of the quaternion with w >= 0, accurate at 0 and at pi).
 * Each iteration: residuals and Jacobian at p (the translation and log-scale columns added), A = J^T W J + priors and
 * g = J^T W r + prior gradient, A + lambda diag(A), Cholesky and solve, the cost at p + delta.  The step is accepted only
 * if every trial unknown is finite and the cost drops; then lambda /= 10, otherwise lambda *= 10 and the step is
 * discarded (lambda is kept within 1e-12..1e12).  A failed factorisation (a pivot that is not positive) is a rejection.
 * lambda starts at lambda0 > 0.  There is no data-dependent exit: the time of a launch depends on B and iters only.
 * Every sum runs in a fixed order and there is no floating-point atomic: the same call gives the same bits.
 *   free_mask    bit i set: unknown i is solved for; clear: it stays at its initial value bit for bit.  Bits 62..63 must
 *                be clear.
 *   cost         the cost at the returned p; accepted: the number of accepted steps, 0..iters.
 * A sample whose targets or weights are not finite (or whose weights are negative) is not fitted: cost = +inf,
 * accepted = 0, and p is its initial value (init = 0: the caller's, untouched; init = 1: zeros, the identity
 * similarity).  With init = 0, p is written only after an accepted step, so no non-finite parameter is ever written. */
int scat_mano_fit(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                  const float* hands_mean, const float* targets, const float* weights, const int* joint_map, float* p,
                  float* cost, int* accepted, int B, int V, uint64_t parents, int tip0, int tip1, int tip2, int tip3,
                  int tip4, int iters, int init, float lambda0, float w_pose, float w_beta, uint64_t free_mask,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif
