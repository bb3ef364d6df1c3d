// What the mesh kernels share (mano_fit_verts.hip: one hand per workgroup, solver included; mano_fit_seq_verts.hip: one
// frame of a track per workgroup, no solver): the tile constants, the staged tile VertStage, the pose state with the
// derivatives the columns are built from (vj_ancestors, vj_derivs, vj_setup), the blend and skinning of a tile (vj_stage),
// the columns of a vertex (vj_cols), the square root of the plane metric on a column (vfit_sqrt_metric), the 3 x 3 block of
// the normal equations that a thread owns (vfit_block) and the Procrustes start over the vertices (vfit_procrustes).
// mano_fit_verts.hip's header comment has the derivation of the columns.  The tile walk that fills the blocks and the fp64
// sum of the priors stand written out in both kernels, on purpose: profiles/fit_mesh_cloud_refactor.txt, section A.
#pragma once
#include "mano_fit_common.h"

namespace scat {

constexpr int kVTile = 32;                            // vertices per tile: what 64 KiB leave beside JacLds and the solver
constexpr int kVCols = kFU + 1;                       // 63: the unknowns, then the residual
constexpr int kVBlocks = kVCols / 3;                  // 21 blocks of 3 columns
constexpr int kVOwners = kVBlocks * (kVBlocks + 1) / 2;   // 231 blocks of the lower triangle, one thread each
constexpr int kVWaves = kFThreads / 64;
constexpr int kVMoments = 17;                         // W, sum w x [3], sum w y [3], sum w |x|^2, sum w x y^T [9]
static_assert(kVCols % 3 == 0 && kVOwners <= kFThreads, "one thread per 3 x 3 block");
static_assert(kMBlendGroup * kVTile <= kFThreads, "the stage's partial sums take one thread each");

template <int TV>
struct VertStage {
    float part[TV][kMBlendGroup][3];   // the partial sums of the blend
    float vp[TV][3];                   // v_posed
    float T[TV][9];                    // the blended rotation
    float d[TV][3];                    // y_v - t_1, un-rotated
    float skw[TV][kMJ];                // the skinning weights
};

// bit k of anc[i]: k is i or an ancestor of i
__device__ __forceinline__ void vj_ancestors(JacLds& m, uint64_t parents) {
    const int tid = threadIdx.x;
    if (tid < kMJ) {
        uint32_t a = 1u << tid;
        int c = tid;
        while (c > 0) {
            c = mano_parent(parents, c);
            a |= 1u << c;
        }
        m.anc[tid] = a;
    }
}

// D, Om, dRg and dtb at the pose that mano_setup left in m.s: what the columns are built from.  A copy of the block inside
// jac_eval, on purpose: with the block lifted into a function that both call, the joint kernels compiled to other code
// (DESIGN.md 16), and mano_fit_common.h is to keep their bits.  vj_ancestors above copies the end of jac_load_model for the
// same reason.  Called by all threads after mano_setup; the caller holds the barrier before the columns are read.
__device__ __forceinline__ void vj_derivs(JacLds& m, const ManoArgs& p) {
    const int tid = threadIdx.x;
    const ManoPose& s = m.s;
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

// the pose state of sample b, with want_jac what the columns need as well.  All threads; begins and ends with a barrier
__device__ __forceinline__ void vj_setup(JacLds& m, const ManoArgs& p, int64_t b, bool want_jac) {
    __syncthreads();
    mano_setup(m.s, p, b);
    if (want_jac) {
        vj_derivs(m, p);
        __syncthreads();
    }
}

// vertices v0 .. v0 + nv - 1 into g: mano_vertex's blend, its five partial sums on five threads, and the skinning
// relative to joint 1.  All threads; ends with a barrier
template <int TV>
__device__ __forceinline__ void vj_stage(const ManoPose& s, const ManoArgs& p, VertStage<TV>& g, int v0, int nv) {
    const int tid = threadIdx.x, V = p.V;
    if (tid < kMBlendGroup * TV) {
        const int q = tid / TV, vl = tid % TV;
        if (vl < nv) {
            const float* bl = p.blend + v0 + vl;
            float acc[3] = {0.f, 0.f, 0.f};
            // unrolled by ten: a thread's loads are independent, and one after the other each would wait for L2
#pragma unroll 10
            for (int n = 0; n < kMCoef / kMBlendGroup; ++n) {
                const int k = q + n * kMBlendGroup;
                const float ck = s.coef[k];
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] += ck * bl[((1 + k) * 3 + c) * V];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) g.part[vl][q][c] = acc[c];
        }
    }
    __syncthreads();
    if (tid < nv) {
        const int v = v0 + tid;
        float vp[3], T[9], d[3] = {0.f, 0.f, 0.f}, wsum = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c)
            vp[c] = p.blend[c * V + v] +
                    (((g.part[tid][0][c] + g.part[tid][1][c]) + (g.part[tid][2][c] + g.part[tid][3][c])) + g.part[tid][4][c]);
#pragma unroll
        for (int e = 0; e < 9; ++e) T[e] = 0.f;
        // y_v - t_1 = sum_i w_i (RG_i (v_posed - J_i) + (t_i - t_1)) + (sum_i w_i - 1) t_1: differences of neighbours,
        // where mano_vertex's (T v_posed + sum_i w_i a_i) - t_1 cancels three vectors of the hand's size.  The last term
        // is zero for weights that sum to one and keeps the layer's meaning for weights that do not
        float wq[kMJ];
#pragma unroll
        for (int i = 0; i < kMJ; ++i) wq[i] = p.weights_t[i * V + v];
#pragma unroll
        for (int i = 0; i < kMJ; ++i) {
            const float w = wq[i];
            g.skw[tid][i] = w;
            if (w == 0.f) continue;
            wsum += w;
            float RGi[9], e[3], f[3];
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                RGi[c] = s.RG[i][c];
                T[c] += w * RGi[c];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) e[c] = vp[c] - s.J[i][c];
            mv(RGi, e, f);
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] += w * (f[c] + (s.t[i][c] - s.t[1][c]));
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            g.vp[tid][c] = vp[c];
            g.d[tid][c] = d[c] + (wsum - 1.f) * s.t[1][c];
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) g.T[tid][e] = T[e];
    }
    __syncthreads();
}

// Columns of vertex v (slot vl of g) times `scale`, out[c ld + column]: k = 0 the three of rots and the ten of betas,
// k = 1..15 the three of joint k's pose
template <int TV>
__device__ __forceinline__ void vj_cols(const JacLds& m, const ManoArgs& p, const VertStage<TV>& g, int vl, int v, int k, float scale,
                                        float* out, int ld) {
    const ManoPose& s = m.s;
    const int V = p.V;
    float Rg[9], col[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) Rg[e] = s.Rg[e];
    if (k == 0) {
        float d[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = g.d[vl][c];
        for (int q = 0; q < 3; ++q) {
            float D[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) D[e] = m.dRg[q][e];
            mv(D, d, col);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c * ld + q] = scale * col[c];
        }
        float sd[kMBeta][3], u[kMBeta][3];   // the joints outside, the ten columns inside: each column's sum still runs up i
#pragma unroll
        for (int b = 0; b < kMBeta; ++b)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                sd[b][c] = p.blend[((1 + b) * 3 + c) * V + v];
                u[b][c] = 0.f;
            }
        for (int i = 0; i < kMJ; ++i) {
            const float w = g.skw[vl][i];
            if (w == 0.f) continue;
            float RGi[9];
#pragma unroll
            for (int c = 0; c < 9; ++c) RGi[c] = s.RG[i][c];
#pragma unroll
            for (int b = 0; b < kMBeta; ++b) {
                float e[3], f[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) e[c] = sd[b][c] - p.joint_s[(i * 3 + c) * kMBeta + b];
                mv(RGi, e, f);
#pragma unroll
                for (int c = 0; c < 3; ++c) u[b][c] += w * (f[c] + m.dtb[i][b][c]);
            }
        }
#pragma unroll
        for (int b = 0; b < kMBeta; ++b) {
            float ub[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) ub[c] = u[b][c] - m.dtb[1][b][c];
            mv(Rg, ub, col);
#pragma unroll
            for (int c = 0; c < 3; ++c) out[c * ld + 3 + kFPose + b] = scale * col[c];
        }
        return;
    }
    float vp[3], T[9], u[3] = {0.f, 0.f, 0.f}, pdir[9][3];
#pragma unroll
    for (int c = 0; c < 3; ++c) vp[c] = g.vp[vl][c];
#pragma unroll
    for (int e = 0; e < 9; ++e) T[e] = g.T[vl][e];
    for (int i = 1; i < kMJ; ++i) {
        const float w = g.skw[vl][i];
        if (!((m.anc[i] >> k) & 1u) || w == 0.f) continue;
        float RGi[9], e[3], f[3];
#pragma unroll
        for (int c = 0; c < 9; ++c) RGi[c] = s.RG[i][c];
#pragma unroll
        for (int c = 0; c < 3; ++c) e[c] = vp[c] - s.J[i][c];
        mv(RGi, e, f);
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] += w * (f[c] + (s.t[i][c] - s.t[k][c]));
    }
#pragma unroll
    for (int e = 0; e < 9; ++e)
#pragma unroll
        for (int c = 0; c < 3; ++c) pdir[e][c] = p.blend[((1 + kMBeta + 9 * (k - 1) + e) * 3 + c) * V + v];
    for (int mm3 = 0; mm3 < 3; ++mm3) {
        const int q = 3 * (k - 1) + mm3;
        float Om[9], o1[3], o2[3], pd[3] = {0.f, 0.f, 0.f}, dy[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            const float De = m.D[q][e];
            Om[e] = m.Om[q][e];
#pragma unroll
            for (int c = 0; c < 3; ++c) pd[c] += pdir[e][c] * De;
        }
        mv(Om, u, o1);
        mv(T, pd, o2);
#pragma unroll
        for (int c = 0; c < 3; ++c) dy[c] = o1[c] + o2[c];
        mv(Rg, dy, col);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c * ld + 3 + q] = scale * col[c];
    }
}

// kMetric: the three entries c[0], c[ld], c[2 ld] of a column through a I + (1 - a) n n^T
__device__ __forceinline__ void vfit_sqrt_metric(float* c, int ld, const float n[3], float a) {
    const float c0 = c[0], c1 = c[ld], c2 = c[2 * ld];
    const float k = (1.f - a) * ((n[0] * c0 + n[1] * c1) + n[2] * c2);
    c[0] = a * c0 + k * n[0];
    c[ld] = a * c1 + k * n[1];
    c[2 * ld] = a * c2 + k * n[2];
}

// The 3 x 3 block of the lower triangle of [J r]^T [J r] that thread tid < kVOwners keeps: rows 3 bi0.., columns 3 bj0..,
// bj0 <= bi0.  The last owner's is block (20, 20), whose entry (62, 62) is the data cost
__device__ __forceinline__ void vfit_block(int tid, int& bi0, int& bj0) {
    bi0 = 0;
    while ((bi0 + 1) * (bi0 + 2) / 2 <= tid) ++bi0;
    bj0 = tid - bi0 * (bi0 + 1) / 2;
}

// init = 1: rots, trans, log_scale of the weighted similarity that takes the zero-pose vertices onto the targets.  The
// moments about the origin in fp64: each thread its vertices ascending, a butterfly over the wavefront, the wavefronts
// ascending; they are centred at the end, which costs fp64 a few digits of its sixteen.  All threads, after vj_setup
__device__ void vfit_procrustes(const ManoPose& s, const ManoArgs& pm, const float* tgt, const float* wts, double* mom, float* p) {
    const int tid = threadIdx.x, V = pm.V;
    float Rg[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) Rg[e] = s.Rg[e];
    double acc[kVMoments];
#pragma unroll
    for (int i = 0; i < kVMoments; ++i) acc[i] = 0.0;
    for (int v = tid; v < V; v += kFThreads) {
        const float w = wts ? wts[v] : 1.f;
        if (w == 0.f) continue;
        float vp[3], T[9], d[3], x[3];
        mano_vertex(s, pm, v, vp, T, d);
        mv(Rg, d, x);
        acc[0] += w;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double wx = (double)w * x[a];
            acc[1 + a] += wx;
            acc[4 + a] += (double)w * tgt[3 * v + a];
            acc[7] += wx * x[a];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[8 + 3 * a + c] += wx * tgt[3 * v + c];
        }
    }
#pragma unroll
    for (int i = 0; i < kVMoments; ++i) {
        double t = acc[i];
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        if ((tid & 63) == 0) mom[(tid >> 6) * kVMoments + i] = t;
    }
    __syncthreads();
    if (tid == 0) {
        double M[kVMoments];
        for (int i = 0; i < kVMoments; ++i) {
            M[i] = mom[i];
            for (int wv = 1; wv < kVWaves; ++wv) M[i] += mom[wv * kVMoments + i];
        }
        const double W = M[0];
        double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, sc = 1.0, mx[3] = {0, 0, 0}, my[3] = {0, 0, 0};
        if (W > 0.0) {
            double K[9], var = M[7];
            for (int c = 0; c < 3; ++c) {
                mx[c] = M[1 + c] / W;
                my[c] = M[4 + c] / W;
            }
            for (int a = 0; a < 3; ++a) {
                var -= M[1 + a] * mx[a];
                for (int c = 0; c < 3; ++c) K[3 * a + c] = M[8 + 3 * a + c] - M[1 + a] * my[c];
            }
            horn_rotation(K, R);   // maximises sum_v y_v . R x_v
            double num = 0.0;
            for (int c = 0; c < 3; ++c)
                for (int a = 0; a < 3; ++a) num += R[3 * c + a] * K[3 * a + c];
            sc = num / var;
            if (!(sc > 1e-30 && sc < 1e30)) sc = 1.0;   // a degenerate point set: keep the model's size
        }
        fit_axis_angle(R, p);
        for (int c = 0; c < 3; ++c)
            p[kFModel + c] = (float)(my[c] - sc * (R[3 * c] * mx[0] + R[3 * c + 1] * mx[1] + R[3 * c + 2] * mx[2]));
        p[kFU - 1] = (float)log(sc);
    }
    __syncthreads();
}

}  // namespace scat
