/* libscat_hip — C ABI of the on-device MANO fit to a surface point cloud: point-to-plane ICP, the loop of
 * scat_mano_fit_points.h with the residual of a point weighed along and across the normal of the model vertex it is
 * matched to (public header of the one library; the conventions are those of scat_mano_fit_points.h: device pointers
 * owned by the caller, explicit sizes, hipStream_t as void* last, stream-ordered, never synchronises, never allocates,
 * retains no pointer, returns 0 or a negative SCAT_E_* code, every check before any HIP call).  The model arrays, V,
 * parents, the 62 unknowns p[62] and the model points model_v = exp(log_scale) verts[v] + trans are
 * scat_mano_fit_verts.h's; the assignment, its reduction, `matched`, `unusable` and the NaN hand-over are
 * scat_mano_fit_points.h's; the topology faces[F,3], vf_off[V+1], vf_idx[3F] (int32) is scat_render.h's: vf_idx[vf_off[v]
 * .. vf_off[v+1]) are the faces that name vertex v.  Every fp32 and int32 operand may sit at any 4-byte-aligned address;
 * stats holds doubles and is 8-byte aligned, the workspace 16-byte aligned.
 *
 * UNITS: as in scat_mano_fit_points.h; normals and w_tangent are pure numbers.
 *
 * THE NORMALS.  n_v = s / |s| with s = sum over the faces (a, b, c) in vf_idx[vf_off[v] .. vf_off[v+1]), in that order,
 * of (x_b - x_a) x (x_c - x_a): the area-weighted vertex normal of scat_render_project.  The differences, the cross
 * products (each product and each difference rounded once, no fused multiply-add), their sum, |s| = sqrt((sx sx + sy sy)
 * + sz sz) and the three quotients run in IEEE fp64 on the fp32 coordinates, and each quotient is rounded to fp32 once.
 * A face index outside 0..F-1 or a face that names a vertex outside 0..V-1 is skipped, never followed; vf_off is clamped
 * to 0..3F.  n_v = (0, 0, 0) exactly where |s|^2 is zero or not finite, which includes a vertex that is in no face.
 *
 * THE METRIC.  With tau = w_tangent in [0, 1] the metric of vertex v is fixed during a round,
 *     M_v = n_v n_v^T + tau (I - n_v n_v^T),            M_v = I for a zero n_v,
 *     rho_v(r) = r^T M_v r = tau |r|^2 + (1 - tau) (n_v . r)^2    (|r|^2 for a zero n_v),
 * tau = 1 is the Euclidean cost of scat_mano_fit_points.h and tau = 0 the pure point-to-plane cost.  Because M depends
 * on the matched vertex alone, the reduction of scat_mano_fit_points.h survives in form:
 *     sum_n w_n rho_c(n)(model_c(n) - q_n) = sum_v W_v rho_v(model_v - qbar_v) + const,
 * with the same W_v and qbar_v, so a round is still one assignment launch and one per-vertex solve.  In the solve the
 * three weighted rows sqrt(W_v) [J_v r_v] of vertex v are multiplied from the left by
 *     sqrt(M_v) = a I + (1 - a) n_v n_v^T,   a = sqrt(tau)   (a = 1 for a zero n_v),
 * column by column c' = a c + (1 - a) (n_v . c) n_v on the three entries of a column.  NORMALS ARE USED AS GIVEN, NOT
 * RENORMALISED: sqrt(M)^2 = M holds for a unit n_v (to rounding for the fp32 normals that scat_mesh_normals writes);
 * with normals of another length the step solves for sqrt(M)^2 while the accept / reject decides on rho, which is a valid
 * (if slower) descent on rho and nothing this header promises more about.
 */
#ifndef SCAT_MANO_FIT_PLANE_H
#define SCAT_MANO_FIT_PLANE_H
#include <stdint.h>

#include "scat_mano_fit_points.h"
#include "scat_render.h"
#ifdef __cplusplus
extern "C" {
#endif

/* verts[B,V,3] -> normals[B,V,3] by the rule above.  One launch, one workgroup of 256 threads per mesh, the vertices in
 * LDS.  A vertex that is not finite gives zero normals where it is summed.  1 <= V <= SCAT_MANO_MAX_V,
 * 1 <= F <= SCAT_RENDER_MAX_F. */
int scat_mesh_normals(const float* verts, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_idx, float* normals,
                      int B, int V, int F, void* stream);

/* scat_mano_fit_verts (init = 0: p is the caller's start, read and written) with the cost
 *     sum_v w[v] rho_v(model_v - target_v) + w_pose |poses|^2 + w_beta |betas|^2
 * for normals[B,V,3] and 0 <= w_tangent <= 1: the rows of the normal equations go through sqrt(M_v) as above, the trial
 * cost is rho summed as scat_mano_fit_verts sums |r|^2, and everything else (the tiles, the accumulation, the solve,
 * accept / reject, lambda, free_mask, the fixed order of every sum) is scat_mano_fit_verts'.  A hand with a normal that
 * is not finite is unusable like one with a weight that is not finite: cost = +inf, accepted = 0, p untouched. */
int scat_mano_fit_verts_metric(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                               const float* hands_mean, const float* targets, const float* weights, const float* normals,
                               float* p, float* cost, int* accepted, int B, int V, uint64_t parents, int iters, float w_tangent,
                               float lambda0, float w_pose, float w_beta, uint64_t free_mask, void* stream);

/* scat_mano_cloud_assign with normals[B,V,3] as a further output: the normals of the fp32 model points it posed (the
 * bits of scat_mesh_normals on model_pts; zeros for an unusable hand).  stats[b][3] is the metric data cost
 *     sum_n w_n rho_c(n)(model_c(n) - q_n) over the matched points
 * in fp64 on the fp32 numbers (n_v as rounded to fp32, tau = (double)w_tangent), rho = tau d2 + (1 - tau) (nr nr) with
 * nr = (nx rx + ny ry) + nz rz and r = q_n - model_c(n), every product and sum rounded once, summed like
 * scat_mano_cloud_assign's.  idx, dist (Euclidean, to
 * the nearest vertex: the search does not know the metric), vw, vtarget, model_pts, stats[b][0..2] and the NaN hand-over
 * have the bits of scat_mano_cloud_assign on the same inputs. */
int scat_mano_cloud_assign_plane(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                 const float* hands_mean, const float* p, const float* points, const float* weights,
                                 const int32_t* faces, const int32_t* vf_off, const int32_t* vf_idx, float max_dist,
                                 float w_tangent, float* model_pts, float* normals, int* idx, float* dist, float* vw,
                                 float* vtarget, double* stats, int B, int N, int V, int F, uint64_t parents, void* stream);

/* Bytes of workspace scat_mano_fit_points_plane needs; 0 for sizes the launch refuses.  scat_mano_fit_points_ws' parts,
 * then the normals.  After the call its first 4 B doubles are the last assignment's stats[B,4]. */
int64_t scat_mano_fit_points_plane_ws(int B, int N, int V, int F);

/* Point-to-plane ICP: scat_mano_fit_points' loop, `rounds` times { scat_mano_cloud_assign_plane at p;
 * scat_mano_fit_verts_metric(iters) on the workspace's (vtarget, vw, normals) }, then one more assignment: 2 rounds + 1
 * launches on the caller's stream, no data-dependent exit.  rounds, iters, max_dist, lambda0, w_pose, w_beta, free_mask,
 * accepted, idx, dist and the limits are scat_mano_fit_points'; data_cost[B] is the last assignment's metric data cost
 * rounded to fp32.  ws: 16-byte aligned, at least scat_mano_fit_points_plane_ws(B, N, V, F) bytes. */
int scat_mano_fit_points_plane(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                               const float* hands_mean, const float* points, const float* weights, const int32_t* faces,
                               const int32_t* vf_off, const int32_t* vf_idx, float* p, float* data_cost, int* accepted, int* idx,
                               float* dist, void* ws, int64_t ws_bytes, int B, int N, int V, int F, uint64_t parents, int rounds,
                               int iters, float max_dist, float w_tangent, float lambda0, float w_pose, float w_beta,
                               uint64_t free_mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif
