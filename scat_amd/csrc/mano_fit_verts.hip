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
//
// Host: both entry points pack a VertsCall (mano_fit_verts.h) for fit_verts_check, every refusal, and fit_verts_launch, the
// kernel; the ICP loop of mano_fit_points.hip checks once and launches once per round.
#include "mano_fit_verts_common.h"

#include "../../include/scat_mano_fit_plane.h"
#include "../../include/scat_mano_fit_verts.h"
#include "mano_fit_verts.h"

namespace scat {

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

struct VFitLds {
    float A[kFU + 1][kFU];   // lower triangle: the damped normal matrix, then its factor; row 62: g, then L^-1 g
    float col[kFU + 1];
    float delta[kFU];
    float p[kFU], pt[kFU];
    float red[kVWaves];
    float cost, ct, lambda;
    int acc, fail, take;
};

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
    int bi0, bj0;   // this thread's block of [J r]^T [J r]
    vfit_block(tid, bi0, bj0);
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

int fit_check_tau(const char* fn, float w_tangent) {
    SCAT_REQUIRE(w_tangent >= 0.f && w_tangent <= 1.f, SCAT_E_ARG, "%s: w_tangent %g outside 0..1", fn, (double)w_tangent);
    return SCAT_OK;
}

int fit_verts_check(const char* fn, const VertsCall& c, int* levels) {
    const void* ptrs[] = {c.blend, c.joint_t, c.joint_s, c.weights_t, c.hands_mean, c.targets, c.p, c.cost, c.accepted, c.normals};
    int rc = mano_validate(fn, ptrs, c.metric ? 10 : 9, c.B, c.V, c.parents, kNoTips, levels);
    if (rc != SCAT_OK) return rc;
    rc = fit_check_args(fn, c.metric ? "none: the start is the caller's" : "Procrustes over the vertices", c.weights, c.iters, c.init,
                        c.lambda0, c.w_pose, c.w_beta, c.free_mask);
    if (rc == SCAT_OK && c.metric) rc = fit_check_tau(fn, c.w_tangent);
    return rc;
}

// the kernel with c.tile vertices per tile (0: kVTile, the product's; the others are compiled into the diag build only)
int fit_verts_launch(const char* fn, const VertsCall& c, int levels) {
    VFitArgs a = {fit_model_args(c.blend, c.joint_t, c.joint_s, c.weights_t, c.hands_mean, c.V, c.parents, kNoTips),
                  c.targets, c.weights, c.p, c.cost, c.accepted, c.iters, c.init, c.lambda0, c.w_pose, c.w_beta, c.free_mask,
                  c.metric ? c.normals : nullptr, c.metric ? c.w_tangent : 1.f};
    a.m.levels = levels;
    const dim3 grid(c.B), block(kFThreads);
    hipStream_t stream = (hipStream_t)c.stream;
    if (c.tile == 0 || c.tile == kVTile) {
        if (c.metric) hipLaunchKernelGGL((mano_fit_verts_kernel<kVTile, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((mano_fit_verts_kernel<kVTile, false>), grid, block, 0, stream, a);
#ifdef SCAT_DIAG
    } else if ((c.tile == 8 || c.tile == 16) && !c.metric) {
        if (c.tile == 8) hipLaunchKernelGGL((mano_fit_verts_kernel<8, false>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((mano_fit_verts_kernel<16, false>), grid, block, 0, stream, a);
#endif
    } else {
        SCAT_REQUIRE(false, SCAT_E_ARG, "%s: no kernel with a tile of %d vertices", fn, c.tile);
    }
    SCAT_LAUNCH_CHECK(fn);
    return SCAT_OK;
}

// The public entry points: the checks, the launch, the label
static int fit_verts_entry(const char* fn, const VertsCall& c) {
    int levels = 0;
    int rc = fit_verts_check(fn, c, &levels);
    if (rc == SCAT_OK) rc = fit_verts_launch(fn, c, levels);
    if (rc != SCAT_OK) return rc;
    if (c.metric) set_kernel_label("mano_fit_verts_metric_v%d_i%d", c.V, c.iters);
    else if (c.tile == 0 || c.tile == kVTile) set_kernel_label("mano_fit_verts_v%d_i%d", c.V, c.iters);
    else set_kernel_label("mano_fit_verts_v%d_i%d_t%d", c.V, c.iters, c.tile);
    return SCAT_OK;
}

extern "C" int scat_mano_fit_verts(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                   const float* hands_mean, const float* targets, const float* weights, float* p, float* cost,
                                   int* accepted, int B, int V, uint64_t parents, int iters, int init, float lambda0,
                                   float w_pose, float w_beta, uint64_t free_mask, void* stream) {
    return fit_verts_entry("scat_mano_fit_verts", {blend, joint_t, joint_s, weights_t, hands_mean, targets, weights, nullptr, p, cost,
                                                   accepted, B, V, parents, iters, init, 0, 1.f, lambda0, w_pose, w_beta, free_mask,
                                                   0, stream});
}

extern "C" int scat_mano_fit_verts_metric(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                          const float* hands_mean, const float* targets, const float* weights,
                                          const float* normals, float* p, float* cost, int* accepted, int B, int V,
                                          uint64_t parents, int iters, float w_tangent, float lambda0, float w_pose,
                                          float w_beta, uint64_t free_mask, void* stream) {
    return fit_verts_entry("scat_mano_fit_verts_metric", {blend, joint_t, joint_s, weights_t, hands_mean, targets, weights, normals, p,
                                                          cost, accepted, B, V, parents, iters, 0, 1, w_tangent, lambda0, w_pose,
                                                          w_beta, free_mask, 0, stream});
}

#ifdef SCAT_DIAG
// tools/fit_verts_bench.py: the fit with another tile (8, 16 or 32 vertices), to see what the tile's barriers and the
// accumulation cost
extern "C" int scat_mano_fit_verts_tile(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                        const float* hands_mean, const float* targets, const float* weights, float* p,
                                        float* cost, int* accepted, int B, int V, uint64_t parents, int iters, int init,
                                        float lambda0, float w_pose, float w_beta, uint64_t free_mask, int tile, void* stream) {
    return fit_verts_entry("scat_mano_fit_verts_tile", {blend, joint_t, joint_s, weights_t, hands_mean, targets, weights, nullptr, p,
                                                        cost, accepted, B, V, parents, iters, init, 0, 1.f, lambda0, w_pose, w_beta,
                                                        free_mask, tile, stream});
}
#endif
