// What the fit kernels share (mano_fit.hip: 3-D joints, quadratic; mano_fit_kp.hip: 2-D keypoints, robust loss, joint
// limits; mano_fit_seq.hip: a track of frames; mano_fit_seq_kp.hip: a track of keypoints; mano_fit_verts.hip: a full mesh;
// mano_fit_points.hip: a point cloud): the constants, the LDS state of the joints' Jacobian with jac_load_model and
// jac_eval, the usable-inputs scan over global memory (fit_unusable), the Procrustes start with fit_axis_angle, the track
// kernels' scan over the frames' starts (fit_start_scan), fit_finite, the quadratic joints problem's residuals and cost
// (fit_residual, fit_cost), the steps of the solver that do not depend on the problem (lm_factor, lm_backsub, lm_solve,
// lm_decide, lm_accept, lm_commit, lm_write) and the entry points' shared argument handling.  mano_fit.hip's header
// comment has the derivation of the Jacobian's columns.  What stays in each kernel is what its problem decides: staging,
// the start, the robust or per-vertex residuals and cost, and the walk that assembles the normal equations, whose row sums
// compile well only in the kernel; what the two keypoint kernels share of that is mano_fit_kp_common.h's.  The mesh kernel
// (mano_fit_verts.hip) keeps all of its device code, its scan included (DESIGN.md 13 has why).
#pragma once
#include "mano_common.h"

#include "../../include/scat_mano_fit.h"
#include "eval_solve.h"

namespace scat {

constexpr int kFThreads = 256;
constexpr int kFJoints = kMJ + kMTips;        // 21
constexpr int kFRows = 3 * kFJoints;          // 63
constexpr int kFModel = SCAT_FIT_MODEL_UNKNOWNS;   // 58: rots, poses, betas
constexpr int kFU = SCAT_FIT_UNKNOWNS;        // 62: + trans, log_scale
constexpr int kFPose = 3 * (kMJ - 1);         // 45
constexpr float kFLambdaMin = 1e-12f, kFLambdaMax = 1e12f;

struct JacLds {
    ManoPose s;
    float tb[kMTips][1 + kMCoef][3];   // the tips' rows of the blend table: template, shapedirs, posedirs
    float tw[kMTips][kMJ];             // the tips' skinning weights
    float D[kFPose][9];                // dR_k / dr_m, index 3 (k - 1) + m
    float Om[kFPose][9];               // RG_parent(k) D RG_k^T
    float dRg[3][9];                   // dRg / d rots_m
    float dtb[kMJ][kMBeta][3];         // d t_i / d beta_b
    float vp[kMTips][3];               // the tips' v_posed
    float T[kMTips][9];                // the tips' blended rotation
    float y[kFJoints][3];              // y_i - t_1, un-rotated
    float x[kFRows];                   // Rg (y_map[j] - y_1): the joints in the caller's order
    int map[kFJoints];
    uint32_t anc[kMJ];                 // bit k: k is i or an ancestor of i
};

// dR/dr_m for R = I + a(t) S(r) + b(t) (r r^T - t I), t = |r|^2: the forward-mode twin of rod_bwd
__device__ __forceinline__ void rod_fwd(const float r[3], int m, float D[9]) {
    const float x = r[0], y = r[1], z = r[2];
    const float t = x * x + y * y + z * z;
    const RodCoef c = rod_coef(t);
    const float S[9] = {0.f, -z, y, z, 0.f, -x, -y, x, 0.f};
    const float rm = r[m], k = 2.f * rm;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float Sm = (i != j && 3 - i - j == m) ? (((3 + j - i) % 3 == 1) ? -1.f : 1.f) : 0.f;   // S(e_m)
            const float em = ((i == m) ? r[j] : 0.f) + ((j == m) ? r[i] : 0.f) - ((i == j) ? k : 0.f);
            const float q = r[i] * r[j] - ((i == j) ? t : 0.f);
            D[3 * i + j] = c.a * Sm + c.b * em + k * (c.da * S[3 * i + j] + c.db * q);
        }
}

// once per workgroup: what the tips need of the model, and the ancestor masks
__device__ void jac_load_model(JacLds& m, const ManoArgs& p) {
    const int tid = threadIdx.x, V = p.V;
    constexpr int per = (1 + kMCoef) * 3;
    for (int w = tid; w < kMTips * per; w += kFThreads) {
        const int j = w / per, kc = w % per;
        m.tb[j][kc / 3][kc % 3] = p.blend[(int64_t)kc * V + p.tips.v[j]];
    }
    for (int w = tid; w < kMTips * kMJ; w += kFThreads) m.tw[w / kMJ][w % kMJ] = p.weights_t[(w % kMJ) * V + p.tips.v[w / kMJ]];
    if (tid < kMJ) {
        uint32_t a = 1u << tid;
        int c = tid;
        while (c > 0) {
            c = mano_parent(p.parents, c);
            a |= 1u << c;
        }
        m.anc[tid] = a;
    }
}

// d y_i / d pose (k, m), q = 3 (k - 1) + m
__device__ __forceinline__ void jac_pose_col(const JacLds& m, int i, int q, int k, float out[3]) {
    const ManoPose& s = m.s;
    float Om[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) Om[e] = m.Om[q][e];
    if (i < kMJ) {
        float d[3] = {0.f, 0.f, 0.f};
        if (((m.anc[i] >> k) & 1u) && i != k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = s.t[i][c] - s.t[k][c];
        }
        mv(Om, d, out);
        return;
    }
    const int tj = i - kMJ;
    float u[3] = {0.f, 0.f, 0.f};
    for (int ii = 1; ii < kMJ; ++ii) {
        const float w = m.tw[tj][ii];
        if (!((m.anc[ii] >> k) & 1u) || w == 0.f) continue;
        float RGi[9], e[3], f[3];
#pragma unroll
        for (int c = 0; c < 9; ++c) RGi[c] = s.RG[ii][c];
#pragma unroll
        for (int c = 0; c < 3; ++c) e[c] = m.vp[tj][c] - s.J[ii][c];
        mv(RGi, e, f);
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] += w * (f[c] + (s.t[ii][c] - s.t[k][c]));
    }
    float o1[3], o2[3], pd[3] = {0.f, 0.f, 0.f}, T[9];
    mv(Om, u, o1);
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        const float De = m.D[q][e];
        T[e] = m.T[tj][e];
#pragma unroll
        for (int c = 0; c < 3; ++c) pd[c] += m.tb[tj][1 + kMBeta + 9 * (k - 1) + e][c] * De;
    }
    mv(T, pd, o2);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = o1[c] + o2[c];
}

// d y_i / d beta_b
__device__ __forceinline__ void jac_beta_col(const JacLds& m, const ManoArgs& p, int i, int b, float out[3]) {
    const ManoPose& s = m.s;
    if (i < kMJ) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = m.dtb[i][b][c];
        return;
    }
    const int tj = i - kMJ;
    float u[3] = {0.f, 0.f, 0.f};
    for (int ii = 0; ii < kMJ; ++ii) {
        const float w = m.tw[tj][ii];
        if (w == 0.f) continue;
        float RGi[9], e[3], f[3];
#pragma unroll
        for (int c = 0; c < 9; ++c) RGi[c] = s.RG[ii][c];
#pragma unroll
        for (int c = 0; c < 3; ++c) e[c] = m.tb[tj][1 + b][c] - p.joint_s[(ii * 3 + c) * kMBeta + b];
        mv(RGi, e, f);
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] += w * (f[c] + m.dtb[ii][b][c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = u[c];
}

// Joints, and with want_jac the 58 model columns of the Jacobian times `scale`, for the parameters p.rots / p.poses /
// p.betas of sample b (global memory, or LDS with b = 0).  m.x gets the joints in the order of m.map; J[(3 j + c) ld + q].
// Called by all threads; begins and ends with a barrier.
__device__ void jac_eval(JacLds& m, const ManoArgs& p, int64_t b, bool want_jac, float scale, float* J, int ld) {
    const int tid = threadIdx.x;
    __syncthreads();
    mano_setup(m.s, p, b);
    const ManoPose& s = m.s;
    if (tid < kMTips) {   // mano_vertex from the LDS copy, same order of sums
        float acc[kMBlendGroup][3];
#pragma unroll
        for (int q = 0; q < kMBlendGroup; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[q][c] = 0.f;
        for (int k0 = 0; k0 < kMCoef; k0 += kMBlendGroup) {
#pragma unroll
            for (int q = 0; q < kMBlendGroup; ++q) {
                const float ck = s.coef[k0 + q];
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[q][c] += ck * m.tb[tid][1 + k0 + q][c];
            }
        }
        float vp[3], T[9], Ta[3] = {0.f, 0.f, 0.f}, x[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) vp[c] = m.tb[tid][0][c] + (((acc[0][c] + acc[1][c]) + (acc[2][c] + acc[3][c])) + acc[4][c]);
#pragma unroll
        for (int e = 0; e < 9; ++e) T[e] = 0.f;
        for (int i = 0; i < kMJ; ++i) {
            const float w = m.tw[tid][i];
#pragma unroll
            for (int e = 0; e < 9; ++e) T[e] += w * s.RG[i][e];
#pragma unroll
            for (int c = 0; c < 3; ++c) Ta[c] += w * s.a[i][c];
        }
        mv(T, vp, x);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            m.vp[tid][c] = vp[c];
            m.y[kMJ + tid][c] = (x[c] + Ta[c]) - s.t[1][c];
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) m.T[tid][e] = T[e];
    } else if (tid >= 64 && tid < 64 + kMJ) {
        const int i = tid - 64;
#pragma unroll
        for (int c = 0; c < 3; ++c) m.y[i][c] = s.t[i][c] - s.t[1][c];
    }
    if (want_jac) {
        if (tid >= 128 && tid < 128 + kFPose) {
            const int q = tid - 128, k = 1 + q / 3, pa = mano_parent(p.parents, k);
            float r[3], D[9], RGp[9], RGk[9], t1[9], Om[9];
#pragma unroll
            for (int c = 0; c < 3; ++c) r[c] = s.r[k][c];
            rod_fwd(r, q % 3, D);
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                RGp[e] = s.RG[pa][e];
                RGk[e] = s.RG[k][e];
            }
            mm(RGp, D, t1);
            mmt(t1, RGk, Om);
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                m.D[q][e] = D[e];
                m.Om[q][e] = Om[e];
            }
        } else if (tid >= 192 && tid < 195) {
            float r[3], D[9];
#pragma unroll
            for (int c = 0; c < 3; ++c) r[c] = s.rg[c];
            rod_fwd(r, tid - 192, D);
#pragma unroll
            for (int e = 0; e < 9; ++e) m.dRg[tid - 192][e] = D[e];
        }
        for (int w = tid; w < kMJ * kMBeta; w += kFThreads) {
            const int i = w / kMBeta, bb = w % kMBeta;
            float acc[3] = {0.f, 0.f, 0.f};
            int c = i;
            while (c > 0) {
                const int pa = mano_parent(p.parents, c);
                float RGp[9], d[3], f[3];
#pragma unroll
                for (int e = 0; e < 9; ++e) RGp[e] = s.RG[pa][e];
#pragma unroll
                for (int cc = 0; cc < 3; ++cc)
                    d[cc] = p.joint_s[(c * 3 + cc) * kMBeta + bb] - p.joint_s[(pa * 3 + cc) * kMBeta + bb];
                mv(RGp, d, f);
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) acc[cc] += f[cc];
                c = pa;
            }
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) m.dtb[i][bb][cc] = acc[cc] + p.joint_s[cc * kMBeta + bb];
        }
    }
    __syncthreads();
    float Rg[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) Rg[e] = s.Rg[e];
    if (tid < kFJoints) {
        const int jm = m.map[tid];
        float d[3], v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = m.y[jm][c];
        mv(Rg, d, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) m.x[3 * tid + c] = v[c];
    }
    if (want_jac) {
        for (int w = tid; w < kFJoints * kFModel; w += kFThreads) {
            const int j = w / kFModel, q = w % kFModel, jm = m.map[j];
            float v[3];
            if (q < 3) {
                float D[9], d[3];
#pragma unroll
                for (int e = 0; e < 9; ++e) D[e] = m.dRg[q][e];
#pragma unroll
                for (int c = 0; c < 3; ++c) d[c] = m.y[jm][c];
                mv(D, d, v);
            } else {
                float dy[3], d1[3];
                if (q < 3 + kFPose) {
                    const int q2 = q - 3, k = 1 + q2 / 3;
                    jac_pose_col(m, jm, q2, k, dy);
                    jac_pose_col(m, 1, q2, k, d1);
                } else {
                    jac_beta_col(m, p, jm, q - 3 - kFPose, dy);
                    jac_beta_col(m, p, 1, q - 3 - kFPose, d1);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) dy[c] -= d1[c];
                mv(Rg, dy, v);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) J[(3 * j + c) * ld + q] = scale * v[c];
        }
    }
    __syncthreads();
}

__device__ __forceinline__ bool fit_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// This thread's share of the usable-inputs scan: nonzero if one of the nx values is not finite, or one of the nw weights
// (w may be null) is not finite or negative.  The caller ORs over the workgroup with __syncthreads_or
__device__ __forceinline__ int fit_unusable(const float* x, int nx, const float* w, int nw) {
    const int tid = threadIdx.x;
    int bad = 0;
    for (int i = tid; i < nx; i += kFThreads) bad |= !fit_finite(x[i]);
    if (w) {
        for (int i = tid; i < nw; i += kFThreads) bad |= !(fit_finite(w[i]) && w[i] >= 0.f);
    }
    return bad;
}

// The rotation matrix R as an axis-angle r: R -> unit quaternion by the largest of the four candidates, w >= 0, then
// r = 2 atan2(|v|, w) v / |v|
__device__ void fit_axis_angle(const double* R, float* r) {
    double qw, qx, qy, qz;
    const double tr = R[0] + R[4] + R[8];
    if (tr > 0.0) {
        const double S = 2.0 * sqrt(tr + 1.0);
        qw = 0.25 * S, qx = (R[7] - R[5]) / S, qy = (R[2] - R[6]) / S, qz = (R[3] - R[1]) / S;
    } else if (R[0] > R[4] && R[0] > R[8]) {
        const double S = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
        qw = (R[7] - R[5]) / S, qx = 0.25 * S, qy = (R[1] + R[3]) / S, qz = (R[2] + R[6]) / S;
    } else if (R[4] > R[8]) {
        const double S = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
        qw = (R[2] - R[6]) / S, qx = (R[1] + R[3]) / S, qy = 0.25 * S, qz = (R[5] + R[7]) / S;
    } else {
        const double S = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
        qw = (R[3] - R[1]) / S, qx = (R[2] + R[6]) / S, qy = (R[5] + R[7]) / S, qz = 0.25 * S;
    }
    if (qw < 0.0) qw = -qw, qx = -qx, qy = -qy, qz = -qz;
    const double n = sqrt(qx * qx + qy * qy + qz * qz);
    const double k = n > 1e-12 ? 2.0 * atan2(n, qw) / n : 2.0;
    r[0] = (float)(k * qx), r[1] = (float)(k * qy), r[2] = (float)(k * qz);
}

// init = 1, one thread: rots, trans, log_scale of the weighted similarity that takes the model joints x onto the targets y
__device__ void fit_procrustes(const float* x, const float* y, const float* w, float* p) {
    double W = 0.0, mx[3] = {0, 0, 0}, my[3] = {0, 0, 0};
    for (int j = 0; j < kFJoints; ++j) {
        W += w[j];
        for (int c = 0; c < 3; ++c) {
            mx[c] += (double)w[j] * x[3 * j + c];
            my[c] += (double)w[j] * y[3 * j + c];
        }
    }
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, sc = 1.0;
    if (W > 0.0) {
        for (int c = 0; c < 3; ++c) {
            mx[c] /= W;
            my[c] /= W;
        }
        double K[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, var = 0.0;
        for (int j = 0; j < kFJoints; ++j)
            for (int a = 0; a < 3; ++a) {
                const double xa = x[3 * j + a] - mx[a];
                var += w[j] * xa * xa;
                for (int c = 0; c < 3; ++c) K[3 * a + c] += w[j] * xa * (y[3 * j + c] - my[c]);
            }
        horn_rotation(K, R);   // maximises sum_j y_j . R x_j
        double num = 0.0;
        for (int c = 0; c < 3; ++c)
            for (int a = 0; a < 3; ++a) num += R[3 * c + a] * K[3 * a + c];
        sc = num / var;
        if (!(sc > 1e-30 && sc < 1e30)) sc = 1.0;   // a degenerate point set: keep the model's size
    } else {
        for (int c = 0; c < 3; ++c) mx[c] = my[c] = 0.0;
    }
    fit_axis_angle(R, p);
    for (int c = 0; c < 3; ++c)
        p[kFModel + c] = (float)(my[c] - sc * (R[3 * c] * mx[0] + R[3 * c + 1] * mx[1] + R[3 * c + 2] * mx[2]));
    p[kFU - 1] = (float)log(sc);
}

// init = 1 of the track kernels (mano_fit_seq.hip, mano_fit_seq_kp.hip), one thread, after every frame's own start in
// P[T][N]: a frame without weight (has[t] == 0) takes the rots and what follows the model unknowns (the similarity, and the
// camera where N has one) of the frame before it, frame 0 those of the first frame that has weight; and rots_t takes the
// equivalent axis-angle that is closer to rots_t-1
template <int N>
__device__ void fit_start_scan(const unsigned char* has, float* P, int T) {
    int first = -1;
    for (int t = 0; t < T && first < 0; ++t)
        if (has[t]) first = t;
    if (first < 0) return;   // every start is the identity similarity: zeros
    for (int t = 0; t < T; ++t) {
        float* q = P + t * N;
        if (!has[t]) {
            const float* src = P + (t > 0 ? t - 1 : first) * N;
            for (int i = 0; i < 3; ++i) q[i] = src[i];
            for (int i = kFModel; i < N; ++i) q[i] = src[i];
        } else if (t > 0) {
            const float* pr = q - N;
            double r[3], n2 = 0.0;
            for (int c = 0; c < 3; ++c) {
                r[c] = q[c];
                n2 += r[c] * r[c];
            }
            const double n = sqrt(n2);
            if (n > 0.0) {
                const double k = 1.0 - 6.283185307179586477 / n;
                double da = 0.0, db = 0.0;
                for (int c = 0; c < 3; ++c) {
                    const double ea = r[c] * k - pr[c], eb = r[c] - pr[c];
                    da += ea * ea;
                    db += eb * eb;
                }
                if (da < db)
                    for (int c = 0; c < 3; ++c) q[c] = (float)(r[c] * k);
            }
        }
    }
}

// The quadratic joints problem (mano_fit.hip, mano_fit_seq.hip) on a kernel's LDS state f with J, r, tgt and w: the
// residuals of the model joints m.x under the similarity of pp; with_cols: the four similarity columns of J as well
template <class F>
__device__ __forceinline__ void fit_residual(const JacLds& m, F& f, const float* pp, bool with_cols) {
    const int row = threadIdx.x;
    if (row < kFRows) {
        const int c = row % 3;
        const float sx = expf(pp[kFU - 1]) * m.x[row];
        f.r[row] = (sx + pp[kFModel + c]) - f.tgt[row];
        if (with_cols) {
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) f.J[row][kFModel + cc] = cc == c ? 1.f : 0.f;
            f.J[row][kFU - 1] = sx;
        }
    }
}

// one thread, ascending: the joints, then the priors
template <class F>
__device__ __forceinline__ float fit_cost(const F& f, const float* pp, float w_pose, float w_beta) {
    float c = 0.f, sp = 0.f, sb = 0.f;
    for (int row = 0; row < kFRows; ++row) c += f.w[row / 3] * (f.r[row] * f.r[row]);
    for (int i = 3; i < 3 + kFPose; ++i) sp += pp[i] * pp[i];
    for (int i = 3 + kFPose; i < kFModel; ++i) sb += pp[i] * pp[i];
    return c + (w_pose * sp + w_beta * sb);
}

// The steps of Levenberg-Marquardt that do not depend on the problem, on a kernel's LDS state f: A[N + 1][N] (lower
// triangle: the damped normal matrix, g as row N), col[N + 1], delta, p, pt[N], cost, lambda, acc, fail, take.
//
// lm_factor: a left-looking Cholesky, one thread per row, two barriers per column; row N (g) rides along and ends as
// L^-1 g.  lm_backsub: L^T x = L^-1 g by columns, last first, one barrier per column; delta = -x.  lm_solve is the two; the
// sequence kernel changes the right-hand side between them.
template <int N, class F>
__device__ __forceinline__ void lm_factor(F& f) {
    const int tid = threadIdx.x;
    for (int k = 0; k < N; ++k) {
        if (tid >= k && tid <= N) {
            float s = f.A[tid][k];
            for (int j = 0; j < k; ++j) s -= f.A[tid][j] * f.A[k][j];
            f.col[tid] = s;
        }
        __syncthreads();
        const float d = f.col[k];
        if (!(d > 0.f) || !fit_finite(d)) {
            if (tid == 0) f.fail = 1;
        }
        const float l = sqrtf(d);
        if (tid == k) f.A[k][k] = l;
        else if (tid > k && tid <= N) f.A[tid][k] = f.col[tid] / l;
        __syncthreads();
    }
}

template <int N, class F>
__device__ __forceinline__ void lm_backsub(F& f) {
    const int tid = threadIdx.x;
    for (int k = N - 1; k >= 0; --k) {
        const float xk = f.A[N][k] / f.A[k][k];
        if (tid < k) f.A[N][tid] -= f.A[k][tid] * xk;
        else if (tid == k) f.delta[k] = -xk;
        __syncthreads();
    }
}

template <int N, class F>
__device__ __forceinline__ void lm_solve(F& f) {
    lm_factor<N>(f);
    lm_backsub<N>(f);
}

// One thread: the step with the cost ct is taken (ok) or not; cost, acc and the schedule of lambda
template <class F>
__device__ __forceinline__ void lm_decide(F& f, bool ok, float ct) {
    if (ok) {
        f.cost = ct;
        f.acc += 1;
        f.lambda = fmaxf(f.lambda * 0.1f, kFLambdaMin);
    } else {
        f.lambda = fminf(f.lambda * 10.f, kFLambdaMax);
    }
}

// One thread, ct the cost at pt: the step is taken if the pivots were positive, pt is finite and the cost drops
template <int N, class F>
__device__ __forceinline__ void lm_accept(F& f, float ct) {
    bool ok = !f.fail && ct < f.cost;
    for (int i = 0; i < N; ++i) ok = ok && fit_finite(f.pt[i]);
    f.take = ok;
    lm_decide(f, ok, ct);
}

// All threads, after lm_accept
template <int N, class F>
__device__ __forceinline__ void lm_commit(F& f) {
    __syncthreads();
    if (f.take && threadIdx.x < N) f.p[threadIdx.x] = f.pt[threadIdx.x];
    __syncthreads();
}

// The results of sample b.  A sample that was not fitted has acc = 0 and cost = +inf from the start: accepted 0, p its start
template <int N, class F, class A>
__device__ __forceinline__ void lm_write(const F& f, const A& a, int64_t b) {
    const int tid = threadIdx.x;
    if ((a.init || f.acc > 0) && tid < N) a.p[b * N + tid] = f.p[tid];
    if (tid == 0) {
        a.cost[b] = fit_finite(f.cost) ? f.cost : INFINITY;   // also NaN: a start that is not finite
        a.accepted[b] = f.acc;
    }
}

}  // namespace scat

// The model's arguments of a fit's entry point; rots / poses / betas are set by the kernel (LDS), levels by mano_validate
static scat::ManoArgs fit_model_args(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                     const float* hands_mean, int V, uint64_t parents, const int* tips) {
    return {blend, joint_t, joint_s, weights_t, hands_mean, nullptr, nullptr, nullptr, V, 0, parents,
            {{tips[0], tips[1], tips[2], tips[3], tips[4]}}};
}

// the mesh and cloud kernels read no tip: vertex 0 stands in for the five, which every V >= 1 has
static const int kNoTips[scat::kMTips] = {0, 0, 0, 0, 0};

// The checks that the fits' entry points share, each text in one place.  fit_check_args is the three in a row, as
// scat_mano_fit and scat_mano_fit_verts make them; an entry point with checks of its own between them (the frames and the
// smoothness weights of scat_mano_fit_seq, the steps of scat_mano_fit_points, the camera of scat_mano_fit_kp) calls the
// parts in its order.  weights may be null; mano_validate has seen the pointers that may not be
static int fit_check_weights(const char* fn, const float* weights) {
    SCAT_REQUIRE(((uintptr_t)weights & 3) == 0, SCAT_E_ARG, "%s: fp32 operands must be 4-byte aligned", fn);
    return SCAT_OK;
}

// start: what the entry point calls its closed-form start
static int fit_check_solver(const char* fn, const char* start, int iters, int init, float lambda0, float w_pose, float w_beta) {
    using namespace scat;
    SCAT_REQUIRE(iters >= 1 && iters <= SCAT_FIT_MAX_ITERS, SCAT_E_ARG, "%s: %d iterations outside 1..%d", fn, iters,
                 SCAT_FIT_MAX_ITERS);
    SCAT_REQUIRE(init == 0 || init == 1, SCAT_E_ARG, "%s: init %d must be 0 (p is the start) or 1 (%s)", fn, init, start);
    SCAT_REQUIRE(lambda0 > 0.f && lambda0 <= kFLambdaMax, SCAT_E_ARG, "%s: lambda0 %g outside (0, %g]", fn, (double)lambda0,
                 (double)kFLambdaMax);
    SCAT_REQUIRE(w_pose >= 0.f && w_pose < INFINITY, SCAT_E_ARG, "%s: w_pose %g must be finite and not negative", fn, (double)w_pose);
    SCAT_REQUIRE(w_beta >= 0.f && w_beta < INFINITY, SCAT_E_ARG, "%s: w_beta %g must be finite and not negative", fn, (double)w_beta);
    return SCAT_OK;
}

static int fit_check_mask(const char* fn, uint64_t free_mask) {
    SCAT_REQUIRE((free_mask >> scat::kFU) == 0, SCAT_E_ARG, "%s: free_mask has bits above %d set", fn, scat::kFU - 1);
    return SCAT_OK;
}

static int fit_check_args(const char* fn, const char* start, const float* weights, int iters, int init, float lambda0,
                          float w_pose, float w_beta, uint64_t free_mask) {
    int rc = fit_check_weights(fn, weights);
    if (rc == SCAT_OK) rc = fit_check_solver(fn, start, iters, init, lambda0, w_pose, w_beta);
    if (rc == SCAT_OK) rc = fit_check_mask(fn, free_mask);
    return rc;
}
