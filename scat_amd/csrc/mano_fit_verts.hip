// The MANO fit to a full mesh, include/scat_mano_fit_verts.h: the V vertices with their analytic Jacobian, and the
// Levenberg-Marquardt fit of mano_fit.hip with 3 V rows of data instead of 63.  One workgroup of 256 threads per hand.
//
// The mesh is walked in tiles of kVTile vertices.  vj_stage blends and skins a tile into LDS in mano_vertex's order of
// sums, the five partial sums of a vertex on five threads.  vj_cols is forward mode, one (vertex, joint) pair per
// work-item.  With y_v = sum_i w_i (RG_i (v_posed - J_i) + t_i) the un-rotated vertex, x_v = Rg (y_v - t_1):
//   rots m        dRg/dr_m (y_v - t_1)
//   pose (k, m)   Omega sum over i in k's subtree of w_i (RG_i (v_posed - J_i) + t_i - t_k), as for a tip in
//                 mano_fit.hip, plus T (posedirs_k . dR_k/dr_m): nine entries of dR_k times nine blend rows, through the
//                 blended rotation T.  Joint 1 does not move: its parent is the root, whose rotation is the identity
//   beta b        sum_i w_i (RG_i (shapedirs_b - dJ_i) + d t_i) - d t_1
// D, Omega, dRg and d t_i / d beta are vj_derivs, what jac_eval computes for the joints.
//
// mano_fit_verts_kernel assembles the normal equations tile by tile: the work-items write their vertex's weighted
// 3 x 62 rows, the weighted residual as column 62, into an LDS tile; after a barrier each of 231 threads adds the tile's
// rows, ascending, into the 3 x 3 block of the lower triangle of [J r]^T [J r] that it keeps in registers over the whole
// walk (fp32 within a tile, the tiles' sums added in fp64).  Row 62 of that product is g.  The trial cost of a step is a
// forward pass with mano_vertex, one vertex per thread.  The solver's steps are mano_fit_common.h's.  All sums run in an
// order fixed by V.
//
// kMetric (include/scat_mano_fit_plane.h): the cost of a vertex is r^T M r, M = n n^T + tau (I - n n^T) with the caller's
// normal n.  The work-item that wrote the columns of a vertex into the tile takes them through sqrt(M) = a I + (1 - a) n n^T
// in place, three entries of a column at a time, before the tile's barrier: no barrier and no LDS is added, and the
// accumulation, the solve and accept / commit do not know.  vfit_cost sums rho instead of |r|^2.
#include "mano_fit_common.h"

#include "../../include/scat_mano_fit_plane.h"
#include "../../include/scat_mano_fit_verts.h"

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

// grid = B, block = 256
__global__ __launch_bounds__(kFThreads) void mano_verts_jac_kernel(ManoArgs p, float* __restrict__ verts, float* __restrict__ jac) {
    __shared__ JacLds m;
    __shared__ VertStage<kVTile> g;
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, V = p.V;
    vj_ancestors(m, p.parents);
    vj_setup(m, p, b, true);
    float* vo = verts + b * 3 * (int64_t)V;
    float* jo = jac + b * 3 * (int64_t)V * kFModel;
    for (int v0 = 0; v0 < V; v0 += kVTile) {
        const int nv = min(kVTile, V - v0);
        vj_stage(m.s, p, g, v0, nv);
        if (tid < nv) {
            float Rg[9], d[3], x[3];
#pragma unroll
            for (int e = 0; e < 9; ++e) Rg[e] = m.s.Rg[e];
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = g.d[tid][c];
            mv(Rg, d, x);
#pragma unroll
            for (int c = 0; c < 3; ++c) vo[3 * (v0 + tid) + c] = x[c];
        }
        for (int w = tid; w < kMJ * kVTile; w += kFThreads) {
            const int vl = w % kVTile, k = w / kVTile;
            if (vl < nv) vj_cols(m, p, g, vl, v0 + vl, k, 1.f, jo + 3 * (int64_t)(v0 + vl) * kFModel, kFModel);
        }
    }
}

struct VFitArgs {
    ManoArgs m;   // rots / poses / betas are set by the kernel (LDS)
    const float* targets;
    const float* weights;
    float* p;
    float* cost;
    int* accepted;
    int iters, init;
    float lambda0, w_pose, w_beta;
    uint64_t free_mask;
    const float* normals;   // kMetric: [B,V,3]
    float w_tangent;        // kMetric: tau
};

// kMetric: the three entries c[0], c[ld], c[2 ld] of a column through a I + (1 - a) n n^T
__device__ __forceinline__ void vfit_sqrt_metric(float* c, int ld, const float n[3], float a) {
    const float c0 = c[0], c1 = c[ld], c2 = c[2 * ld];
    const float k = (1.f - a) * ((n[0] * c0 + n[1] * c1) + n[2] * c2);
    c[0] = a * c0 + k * n[0];
    c[ld] = a * c1 + k * n[1];
    c[2 * ld] = a * c2 + k * n[2];
}

struct VFitLds {
    float A[kFU + 1][kFU];   // lower triangle: the damped normal matrix, then its factor; row 62: g, then L^-1 g
    float col[kFU + 1];
    float delta[kFU];
    float p[kFU], pt[kFU];
    float red[kVWaves];
    float cost, ct, lambda;
    int acc, fail, take;
};

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

// f.ct = the cost at pp (pm's parameters): a forward pass, one vertex per thread, each thread its vertices ascending, a
// butterfly over the wavefront, the wavefronts pairwise, then the priors.  All threads; begins and ends with a barrier.
// kMetric: rho = tau |r|^2 + (1 - tau) (n . r)^2 for the normals nrm [V,3], |r|^2 where the normal is zero
template <bool kMetric>
__device__ void vfit_cost(JacLds& m, VFitLds& f, const ManoArgs& pm, const float* pp, const float* tgt, const float* wts,
                          float w_pose, float w_beta, const float* nrm, float tau) {
    const int tid = threadIdx.x, V = pm.V;
    vj_setup(m, pm, 0, false);
    const ManoPose& s = m.s;
    const float sc = expf(pp[kFU - 1]);
    float Rg[9], tr[3], c = 0.f;
#pragma unroll
    for (int e = 0; e < 9; ++e) Rg[e] = s.Rg[e];
#pragma unroll
    for (int a = 0; a < 3; ++a) tr[a] = pp[kFModel + a];
    for (int v = tid; v < V; v += kFThreads) {
        const float w = wts ? wts[v] : 1.f;
        if (w == 0.f) continue;
        float vp[3], T[9], d[3], x[3], r[3];
        mano_vertex(s, pm, v, vp, T, d);
        mv(Rg, d, x);
#pragma unroll
        for (int a = 0; a < 3; ++a) r[a] = (sc * x[a] + tr[a]) - tgt[3 * v + a];
        if constexpr (kMetric) {
            const float n0 = nrm[3 * v], n1 = nrm[3 * v + 1], n2 = nrm[3 * v + 2];
            const float r2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2], nr = (n0 * r[0] + n1 * r[1]) + n2 * r[2];
            const bool flat = n0 == 0.f && n1 == 0.f && n2 == 0.f;
            c += w * (flat ? r2 : tau * r2 + (1.f - tau) * (nr * nr));
        } else {
            c += w * ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
        }
    }
    c = mano_wave_sum(c);
    if ((tid & 63) == 0) f.red[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        // near the minimum of a clean mesh the priors are most of the cost: their 55 squares in fp64, rounded once
        double sp = 0.0, sb = 0.0;
        for (int i = 3; i < 3 + kFPose; ++i) sp += (double)pp[i] * pp[i];
        for (int i = 3 + kFPose; i < kFModel; ++i) sb += (double)pp[i] * pp[i];
        const double data = ((double)f.red[0] + f.red[1]) + ((double)f.red[2] + f.red[3]);
        f.ct = (float)(data + ((double)w_pose * sp + (double)w_beta * sb));
    }
    __syncthreads();
}
static_assert(kVWaves == 4, "vfit_cost adds four wavefronts");

// grid = B, block = 256; TV: the tile, kVTile in the product; kMetric: scat_mano_fit_verts_metric
template <int TV, bool kMetric>
__global__ __launch_bounds__(kFThreads) void mano_fit_verts_kernel(VFitArgs a) {
    __shared__ JacLds m;
    __shared__ VFitLds f;
    __shared__ VertStage<TV> g;
    __shared__ alignas(8) float tile[3 * TV][kVCols];   // the weighted rows [J r] of a tile; the start's moments before
    static_assert(sizeof(JacLds) + sizeof(VFitLds) + sizeof(VertStage<TV>) + sizeof(tile) <= 64 * 1024, "static LDS");
    static_assert(sizeof(tile) >= kVWaves * kVMoments * sizeof(double), "the moments fit the tile");
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, V = a.m.V;
    const float* tgt = a.targets + b * 3 * (int64_t)V;
    const float* wts = a.weights ? a.weights + b * (int64_t)V : nullptr;
    const float* nrm = nullptr;
    float tau = 1.f, ma = 1.f;
    if constexpr (kMetric) {
        nrm = a.normals + b * 3 * (int64_t)V;
        tau = a.w_tangent;
        ma = sqrtf(tau);
    }
    vj_ancestors(m, a.m.parents);
    if (tid < kFU) f.p[tid] = a.init ? 0.f : a.p[b * kFU + tid];
    int bad = 0;
    for (int i = tid; i < 3 * V; i += kFThreads) bad |= !fit_finite(tgt[i]);
    if (wts) {
        for (int i = tid; i < V; i += kFThreads) bad |= !(fit_finite(wts[i]) && wts[i] >= 0.f);
    }
    if constexpr (kMetric) {
        for (int i = tid; i < 3 * V; i += kFThreads) bad |= !fit_finite(nrm[i]);
    }
    if (tid == 0) {
        f.acc = 0;
        f.lambda = a.lambda0;
        f.cost = INFINITY;
    }
    bad = __syncthreads_or(bad);
    if (bad) {   // the same for every thread of the workgroup; acc and cost are as lm_write wants them
        lm_write<kFU>(f, a, b);
        return;
    }
    ManoArgs pc = a.m, pt = a.m;
    pc.rots = f.p, pc.poses = f.p + 3, pc.betas = f.p + 3 + kFPose;
    pt.rots = f.pt, pt.poses = f.pt + 3, pt.betas = f.pt + 3 + kFPose;
    if (a.init) {
        vj_setup(m, pc, 0, false);   // the zero pose
        vfit_procrustes(m.s, pc, tgt, wts, reinterpret_cast<double*>(&tile[0][0]), f.p);
    }
    vfit_cost<kMetric>(m, f, pc, f.p, tgt, wts, a.w_pose, a.w_beta, nrm, tau);
    if (tid == 0) f.cost = f.ct;
    const uint64_t fm = a.free_mask;
    int bi0 = 0;   // this thread's block of [J r]^T [J r]: rows 3 bi0.., columns 3 bj0.., bj0 <= bi0
    while ((bi0 + 1) * (bi0 + 2) / 2 <= tid) ++bi0;
    const int bj0 = tid - bi0 * (bi0 + 1) / 2;
    for (int it = 0; it < a.iters; ++it) {
        vj_setup(m, pc, 0, true);
        const float sc = expf(f.p[kFU - 1]);
        float Rg[9], tr[3];
        double tot[3][3];   // a tile's sums in fp32, the tiles' in fp64: 3 V sequential fp32 terms would cost the step a digit
#pragma unroll
        for (int e = 0; e < 9; ++e) Rg[e] = m.s.Rg[e];
#pragma unroll
        for (int c = 0; c < 3; ++c) tr[c] = f.p[kFModel + c];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) tot[i][j] = 0.0;
        for (int v0 = 0; v0 < V; v0 += TV) {
            const int nv = min(TV, V - v0);
            vj_stage(m.s, pc, g, v0, nv);
            for (int w = tid; w < kMJ * TV; w += kFThreads) {
                const int vl = w % TV, k = w / TV, v = v0 + vl;
                if (vl >= nv) continue;
                const float wv = wts ? wts[v] : 1.f, sw = sqrtf(wv);
                float* row = &tile[3 * vl][0];
                vj_cols(m, pc, g, vl, v, k, sc * sw, row, kVCols);
                if (k == 0) {   // the similarity's columns and the residual; a vertex of weight 0 is a row of zeros
                    float d[3], x[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) d[c] = g.d[vl][c];
                    mv(Rg, d, x);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float sx = sc * x[c];
#pragma unroll
                        for (int cc = 0; cc < 3; ++cc) row[c * kVCols + kFModel + cc] = cc == c ? sw : 0.f;
                        row[c * kVCols + kFU - 1] = sw * sx;
                        row[c * kVCols + kFU] = wv != 0.f ? sw * ((sx + tr[c]) - tgt[3 * v + c]) : 0.f;
                    }
                }
                if constexpr (kMetric) {   // the columns this work-item wrote, through sqrt(M_v)
                    const float n[3] = {nrm[3 * v], nrm[3 * v + 1], nrm[3 * v + 2]};
                    const float av = (n[0] == 0.f && n[1] == 0.f && n[2] == 0.f) ? 1.f : ma;
                    if (k == 0) {
                        for (int q = 0; q < 3; ++q) vfit_sqrt_metric(row + q, kVCols, n, av);
                        for (int q = 3 + kFPose; q < kVCols; ++q) vfit_sqrt_metric(row + q, kVCols, n, av);
                    } else {
                        for (int q = 3 * k; q < 3 * k + 3; ++q) vfit_sqrt_metric(row + q, kVCols, n, av);
                    }
                }
            }
            __syncthreads();
            if (tid < kVOwners) {
                float acc[3][3];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) acc[i][j] = 0.f;
                for (int r = 0; r < 3 * nv; ++r) {
                    float ra[3], rb[3];
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        ra[i] = tile[r][3 * bi0 + i];
                        rb[i] = tile[r][3 * bj0 + i];
                    }
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j) acc[i][j] += ra[i] * rb[j];
                }
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) tot[i][j] += (double)acc[i][j];
            }
        }
        // A = J^T W J + priors (lower triangle), g = J^T W r + the priors' gradient as row 62; a frozen unknown is a unit row
        if (tid < kVOwners) {
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int ai = 3 * bi0 + i, bi = 3 * bj0 + j;
                    if (bi > ai || bi >= kFU) continue;
                    const bool fb = (fm >> bi) & 1u;
                    float sum = (float)tot[i][j];
                    if (ai == kFU) {
                        if (bi >= 3 && bi < kFModel) sum += (bi < 3 + kFPose ? a.w_pose : a.w_beta) * f.p[bi];
                        f.A[kFU][bi] = fb ? sum : 0.f;
                    } else {
                        const bool fa = (fm >> ai) & 1u;
                        if (ai == bi) {
                            if (ai >= 3 && ai < kFModel) sum += ai < 3 + kFPose ? a.w_pose : a.w_beta;
                            sum *= 1.f + f.lambda;   // Marquardt: A + lambda diag(A)
                        }
                        f.A[ai][bi] = (fa && fb) ? sum : (ai == bi ? 1.f : 0.f);
                    }
                }
        }
        if (tid == 0) f.fail = 0;
        __syncthreads();
        lm_solve<kFU>(f);
        if (tid < kFU) f.pt[tid] = ((fm >> tid) & 1u) ? f.p[tid] + f.delta[tid] : f.p[tid];
        vfit_cost<kMetric>(m, f, pt, f.pt, tgt, wts, a.w_pose, a.w_beta, nrm, tau);
        if (tid == 0) lm_accept<kFU>(f, f.ct);
        lm_commit<kFU>(f);
    }
    lm_write<kFU>(f, a, b);
}

}  // namespace scat

using namespace scat;

extern "C" int scat_mano_verts_jac(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                   const float* hands_mean, const float* rots, const float* poses, const float* betas,
                                   float* verts, float* jac, int B, int V, uint64_t parents, void* stream) {
    const void* ptrs[] = {blend, joint_t, joint_s, weights_t, hands_mean, rots, poses, betas, verts, jac};
    ManoArgs p = {blend, joint_t, joint_s, weights_t, hands_mean, rots, poses, betas, V, 0, parents, {{0, 0, 0, 0, 0}}};
    const int rc = mano_validate("scat_mano_verts_jac", ptrs, 10, B, V, parents, kNoTips, &p.levels);
    if (rc != SCAT_OK) return rc;
    hipLaunchKernelGGL(mano_verts_jac_kernel, dim3(B), dim3(kFThreads), 0, (hipStream_t)stream, p, verts, jac);
    SCAT_LAUNCH_CHECK("scat_mano_verts_jac");
    set_kernel_label("mano_verts_jac_v%d", V);
    return SCAT_OK;
}

// Both fits' entry points: the checks, then the kernel with `tile` vertices per tile (kVTile in the product; the others
// are compiled into the diag build only)
static int fit_verts_launch(const char* fn, const float* blend, const float* joint_t, const float* joint_s,
                            const float* weights_t, const float* hands_mean, const float* targets, const float* weights,
                            float* p, float* cost, int* accepted, int B, int V, uint64_t parents, int iters, int init,
                            float lambda0, float w_pose, float w_beta, uint64_t free_mask, int tile, void* stream) {
    const void* ptrs[] = {blend, joint_t, joint_s, weights_t, hands_mean, targets, p, cost, accepted};
    VFitArgs a = {fit_model_args(blend, joint_t, joint_s, weights_t, hands_mean, V, parents, kNoTips),
                  targets, weights, p, cost, accepted, iters, init, lambda0, w_pose, w_beta, free_mask, nullptr, 1.f};
    int rc = mano_validate(fn, ptrs, 9, B, V, parents, kNoTips, &a.m.levels);
    if (rc != SCAT_OK) return rc;
    rc = fit_check_args(fn, "Procrustes over the vertices", weights, iters, init, lambda0, w_pose, w_beta, free_mask);
    if (rc != SCAT_OK) return rc;
    const dim3 grid(B), block(kFThreads);
    if (tile == kVTile) {
        hipLaunchKernelGGL((mano_fit_verts_kernel<kVTile, false>), grid, block, 0, (hipStream_t)stream, a);
        set_kernel_label("mano_fit_verts_v%d_i%d", V, iters);
#ifdef SCAT_DIAG
    } else if (tile == 8 || tile == 16) {
        if (tile == 8) hipLaunchKernelGGL((mano_fit_verts_kernel<8, false>), grid, block, 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((mano_fit_verts_kernel<16, false>), grid, block, 0, (hipStream_t)stream, a);
        set_kernel_label("mano_fit_verts_v%d_i%d_t%d", V, iters, tile);
#endif
    } else {
        SCAT_REQUIRE(false, SCAT_E_ARG, "%s: no kernel with a tile of %d vertices", fn, tile);
    }
    SCAT_LAUNCH_CHECK(fn);
    return SCAT_OK;
}

extern "C" int scat_mano_fit_verts(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                   const float* hands_mean, const float* targets, const float* weights, float* p, float* cost,
                                   int* accepted, int B, int V, uint64_t parents, int iters, int init, float lambda0,
                                   float w_pose, float w_beta, uint64_t free_mask, void* stream) {
    return fit_verts_launch("scat_mano_fit_verts", blend, joint_t, joint_s, weights_t, hands_mean, targets, weights, p, cost,
                            accepted, B, V, parents, iters, init, lambda0, w_pose, w_beta, free_mask, kVTile, stream);
}

extern "C" int scat_mano_fit_verts_metric(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                          const float* hands_mean, const float* targets, const float* weights,
                                          const float* normals, float* p, float* cost, int* accepted, int B, int V,
                                          uint64_t parents, int iters, float w_tangent, float lambda0, float w_pose,
                                          float w_beta, uint64_t free_mask, void* stream) {
    const char* fn = "scat_mano_fit_verts_metric";
    const void* ptrs[] = {blend, joint_t, joint_s, weights_t, hands_mean, targets, normals, p, cost, accepted};
    VFitArgs a = {fit_model_args(blend, joint_t, joint_s, weights_t, hands_mean, V, parents, kNoTips),
                  targets, weights, p, cost, accepted, iters, 0, lambda0, w_pose, w_beta, free_mask, normals, w_tangent};
    int rc = mano_validate(fn, ptrs, 10, B, V, parents, kNoTips, &a.m.levels);
    if (rc != SCAT_OK) return rc;
    rc = fit_check_args(fn, "none: the start is the caller's", weights, iters, 0, lambda0, w_pose, w_beta, free_mask);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE(w_tangent >= 0.f && w_tangent <= 1.f, SCAT_E_ARG, "%s: w_tangent %g outside 0..1", fn, (double)w_tangent);
    hipLaunchKernelGGL((mano_fit_verts_kernel<kVTile, true>), dim3(B), dim3(kFThreads), 0, (hipStream_t)stream, a);
    SCAT_LAUNCH_CHECK(fn);
    set_kernel_label("mano_fit_verts_metric_v%d_i%d", V, iters);
    return SCAT_OK;
}

#ifdef SCAT_DIAG
// tools/fit_verts_bench.py: the fit with another tile (8, 16 or 32 vertices), to see what the tile's barriers and the
// accumulation cost
extern "C" int scat_mano_fit_verts_tile(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                        const float* hands_mean, const float* targets, const float* weights, float* p,
                                        float* cost, int* accepted, int B, int V, uint64_t parents, int iters, int init,
                                        float lambda0, float w_pose, float w_beta, uint64_t free_mask, int tile, void* stream) {
    return fit_verts_launch("scat_mano_fit_verts_tile", blend, joint_t, joint_s, weights_t, hands_mean, targets, weights, p,
                            cost, accepted, B, V, parents, iters, init, lambda0, w_pose, w_beta, free_mask, tile, stream);
}
#endif
