/* libscat_hip — C ABI of the on-device MANO layer (third public header of the one library; the conventions are those of
 * scat_eval.h: device pointers owned by the caller, explicit sizes, hipStream_t as void* last, stream-ordered, never
 * synchronises, never allocates, retains no pointer, returns 0 or a negative SCAT_E_* code).  No workspace is needed.
 *
 * Stands in for rot_pose_beta_to_mesh of the reference (models/mano.py:280-391, reference checkout tomguluson92/SCAT),
 * which turns the 3 + 45 + 10 MANO parameters of H3DWEncoder's output into 21 joints and V vertices:
 *   mano.py:284-286    pose = [0,0,0] ++ (hands_mean + poses): 16 axis-angles, the chain's root rotation is the identity
 *   mano.py:288-292    v_shaped = v_template + shapedirs . beta
 *   mano.py:302-304    J = J_regressor . v_shaped (16 joints)
 *   mano.py:270-277    pw = concat_{k=1..15}(R(pose_k) - I), row-major, 135 values
 *   mano.py:296-300    v_posed = v_shaped + posedirs . pw
 *   mano.py:322-327    G_0 = [R_0 | J_0], G_i = G_parent(i) . [R_i | J_i - J_parent(i)]
 *   mano.py:331-337    A_i = G_i with translation t_i - R^G_i . J_i
 *   mano.py:339-348    v' = (sum_i w[v,i] A_i) . [v_posed; 1]
 *   mano.py:353-380    joints = the 16 translations of G_i, then v' at the five tip vertices (:374-378 uses 320, 443, 671,
 *                      554, 744 in that order)
 *   mano.py:351,382-383 both multiplied by R(rots)
 *   mano.py:386-388    joint 1 (the transformed one) subtracted from both
 *   mano.py:391        output [B, 21 + V, 3]: joints first, then vertices
 *   mano.py:236-267    Rodrigues: R = I + a S(r) + b S(r)^2, a = sin(theta)/theta, b = (1 - cos(theta))/theta^2
 *
 * One deliberate difference.  The reference switches to a Taylor form below theta = 1e-30 (mano.py:258-265), so its
 * forward is finite at a zero rotation, but its autograd differentiates r / theta on the other branch as well and
 * returns NaN there.  Here a and b are functions of theta^2 with a series below theta^2 = 0.25 (terms to theta^8) and
 * b = 2 sin^2(theta/2) / theta^2 above: value and gradient are accurate from theta = 0 to beyond pi, and the backward
 * returns the finite limit at a zero rotation.
 *
 * The model arrays are data, prepared once per model by the caller (scat_amd/mano.py ManoModel.to), all fp32:
 *   blend[146][3][V]     vertex-minor blend table: row 0 v_template, rows 1..10 shapedirs[:, :, k], rows 11..145
 *                        posedirs[:, :, k]; blend[k][c][v]
 *   joint_t[16][3]       J_regressor . v_template
 *   joint_s[16][3][10]   J_regressor . shapedirs (the regressor is linear, so it is folded into the model once)
 *   weights_t[16][V]     skinning weights, transposed
 *   hands_mean[45]
 * 1 <= V <= SCAT_MANO_MAX_V: the backward keeps nine floats per vertex in the workgroup's LDS (36 bytes x 1536 = 54 KiB
 * of the 64 KiB a workgroup may declare statically).  Every operand may sit at any 4-byte-aligned address.
 *
 * The kinematic tree and the tips travel by value:
 *   parents   16 nibbles, parent[i] = (parents >> 4 i) & 15; parent[0] = 0 marks the root, 0 <= parent[i] < i otherwise
 *   tip0..4   vertex indices, 0 <= tip < V; joints 16..20 are v' at these vertices
 *
 * One workgroup per sample in both directions; V may exceed the workgroup size (threads loop over vertices).
 */
#ifndef SCAT_MANO_H
#define SCAT_MANO_H
#include <stdint.h>

#include "scat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define SCAT_MANO_MAX_V 1536
#define SCAT_MANO_JOINTS 16
#define SCAT_MANO_TIPS 5

/* rots[B,3], poses[B,45], betas[B,10] -> out[B, 21 + V, 3].  One launch. */
int scat_mano_fwd(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                  const float* hands_mean, const float* rots, const float* poses, const float* betas, float* out, int B,
                  int V, uint64_t parents, int tip0, int tip1, int tip2, int tip3, int tip4, void* stream);

/* dout[B, 21 + V, 3] -> drots[B,3], dposes[B,45], dbetas[B,10]; the model arrays get no gradient.  One launch: the
 * forward quantities are recomputed from the inputs, nothing is kept between the two calls.  The sums over vertices
 * (16 x 12 for the A_i, 135 + 10 for the blend coefficients, 9 + 3 for the global rotation and the root) run in an order
 * fixed by V alone (strided partial sums per lane, a shuffle butterfly per wavefront, then ascending over wavefronts in
 * LDS); there is no floating-point atomic, so the same call gives the same bits. */
int scat_mano_bwd(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                  const float* hands_mean, const float* rots, const float* poses, const float* betas, const float* dout,
                  float* drots, float* dposes, float* dbetas, int B, int V, uint64_t parents, int tip0, int tip1,
                  int tip2, int tip3, int tip4, void* stream);

#ifdef __cplusplus
}
#endif
#endif
