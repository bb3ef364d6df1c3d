/* libscat_hip — C ABI of the on-device MANO fit to a full mesh: the mesh with its analytic Jacobian, and the fit of
 * scat_mano_fit.h with the V vertices as data instead of 21 joints (public header of the one library; the conventions are
 * those of scat_mano.h: device pointers owned by the caller, explicit sizes, hipStream_t as void* last, stream-ordered,
 * never synchronises, never allocates, retains no pointer, returns 0 or a negative SCAT_E_* code).  No workspace is
 * needed.  The model arrays (blend, joint_t, joint_s, weights_t, hands_mean), V and parents are those of scat_mano.h;
 * the tips are not needed.  verts(rots, poses, betas)[V][3] are rows 21.. of scat_mano_fwd's output: the mesh after the
 * global rotation, joint 1 subtracted.  Every operand may sit at any 4-byte-aligned address.
 *
 * UNITS: rots and poses are axis-angles in radians (poses on top of hands_mean, as in scat_mano.h), the vertices are in
 * the model's unit (metres for MANO), trans in the targets' unit, and the cost in the targets' unit squared.
 *
 * The unknowns of one hand are those of scat_mano_fit.h, p[62] = rots[3] ++ poses[45] ++ betas[10] ++ trans[3] ++
 * log_scale[1], the model points
 *     model_v = exp(log_scale) verts[v] + trans,                             v = 0..V-1
 * and the cost
 *     sum_v w[v] |model_v - target_v|^2 + w_pose |poses|^2 + w_beta |betas|^2.
 * There is no joint_map: vertex v of the targets is vertex v of the model.
 */
#ifndef SCAT_MANO_FIT_VERTS_H
#define SCAT_MANO_FIT_VERTS_H
#include <stdint.h>

#include "scat_mano_fit.h"
#ifdef __cplusplus
extern "C" {
#endif

/* rots[B,3], poses[B,45], betas[B,10] -> verts[B,V,3] and jac[B,3V,58] = d verts / d (rots, poses, betas), row 3 v + c,
 * column order rots, poses, betas.  One launch, one workgroup per sample, the threads loop over the vertices.  Forward
 * mode, and exact: a pose parameter of joint k moves a vertex through the joints of k's subtree that it is skinned to
 * (Omega sum_i w_i (RG_i (v_posed - J_i) + t_i - t_k), Omega = RG_parent(k) dR_k RG_k^T) and through the pose correctives
 * (T posedirs_k . dR_k, T the blended skinning rotation); joint 1, which is subtracted, does not move with the pose
 * because its parent is the root.  Rodrigues and its derivative are the t = theta^2 forms of the layer: finite at zero. */
int scat_mano_verts_jac(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                        const float* hands_mean, const float* rots, const float* poses, const float* betas, float* verts,
                        float* jac, int B, int V, uint64_t parents, void* stream);

/* targets[B,V,3], weights[B,V] (null: all ones) -> p[B,62], cost[B], accepted[B].  `iters` Levenberg-Marquardt
 * iterations (1..SCAT_FIT_MAX_ITERS) inside one launch, one workgroup per hand.
 *   init = 0     p is read: the caller's start.
 *   init = 1     p is written only: poses = betas = 0, and rots, trans and log_scale from the weighted similarity
 *                Procrustes of the zero-pose vertices onto the targets (the moments summed in fp64 in a fixed order,
 *                Horn's quaternion in fp64, the axis-angle as in scat_mano_fit).
 * Each iteration is scat_mano_fit's: residuals and Jacobian at p, A = J^T W J + priors and g = J^T W r + prior gradient
 * (summed over the 3 V rows tile by tile, the tiles and the rows of a tile ascending), A + lambda diag(A), Cholesky and
 * solve, the cost at p + delta from a forward pass over the mesh.  The step is accepted only if every trial unknown is
 * finite and the cost drops; then lambda /= 10, otherwise lambda *= 10 and the step is discarded (lambda is kept within
 * 1e-12..1e12).  A failed factorisation is a rejection.  lambda starts at lambda0 > 0.  There is no data-dependent exit:
 * the time of a launch depends on B, V and iters only.  Every sum runs in an order fixed by V alone and there is no
 * floating-point atomic: the same call gives the same bits.
 *   weights      a vertex of weight 0 does not count, whatever its finite target.
 *   free_mask    bit i set: unknown i is solved for; clear: it stays at its initial value bit for bit.  Bits 62..63 must
 *                be clear.
 *   cost         the cost at the returned p; accepted: the number of accepted steps, 0..iters.
 * A hand whose targets or weights are not finite (or whose weights are negative) is not fitted: cost = +inf,
 * accepted = 0, and p is its initial value (init = 0: the caller's, untouched; init = 1: zeros, the identity
 * similarity).  With init = 0, p is written only after an accepted step, so no non-finite parameter is ever written. */
int scat_mano_fit_verts(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                        const float* hands_mean, const float* targets, const float* weights, float* p, float* cost,
                        int* accepted, int B, int V, uint64_t parents, int iters, int init, float lambda0, float w_pose,
                        float w_beta, uint64_t free_mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif
