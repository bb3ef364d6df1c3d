// The MANO fit to an unordered point cloud, include/scat_mano_fit_points.h: the correspondence kernel between the layer
// and scat_mano_fit_verts, and the loop of launches around the two.  One workgroup of 256 threads per hand.
//
// cloud_assign_kernel<kParams>, one template in two forms:
//   model points   kParams: p[b] into LDS, a ManoArgs pointed at it (b = 0) as vfit_cost does, mano_setup, then
//                  mano_vertex, x = Rg d and exp(p[61]) x + trans for every vertex, into LDS as x / y / z arrays and
//                  into model_pts.  Otherwise the caller's verts are copied there.
//   nearest vertex a thread takes the points tid, tid + 256, ..., four at a time, and walks all V vertices once for the
//                  four: every lane reads the same LDS address, a broadcast (mesh_eval.hip's nn_walk, with the index
//                  kept beside the minimum).  fp64 on the fp32 numbers, contraction off, strict < ascending.  The vertex
//                  of a matched point goes into an LDS index array of N ints, -1 for the others.
//   reduction      a thread takes the vertices tid, tid + 256, ... and scans the index array once per vertex, n
//                  ascending (four indices per LDS read), adding w, w q and w d2 of its points in fp64 (d2 recomputed by the walk's expression: the
//                  same bits).  The three totals of stats: each thread's vertices ascending, an xor butterfly over the
//                  wavefront, the four wavefronts ascending.
// The usable-inputs scan of the points and their weights is mano_fit_common.h's fit_unusable.
// Static LDS at the largest sizes: 18 KiB of vertices, 32 KiB of indices, 2.6 KiB of pose state: 53 KiB of the 64.
// icp_loop is every loop of launches: the checks, the workspace (points_ws, which knows whether the normals and a track
// solve's part follow), the CloudArgs (cloud_args, the assignment entry points' filler too) and `rounds` times {assign,
// solve}, then one last assign.  The solve is passed in, checked once and launched unchecked every round: the mesh fit
// (mano_fit_verts.h) for scat_mano_fit_points, where each assign after the first adds the accepted count of the fit
// before it to the caller's total, and the track solve (mano_fit_seq_verts.h) for scat_mano_fit_points_seq.
//
// kPlane (include/scat_mano_fit_plane.h, point-to-plane ICP): the thread that owns vertex v in the reduction first forms
// the vertex normal from the LDS model points and the topology in global memory (mesh_vertex_normal, fp64), keeps it in
// registers, writes it to the caller, and adds rho instead of d2 to the data cost; W, S, the walk and the index array do
// not know, so every other output keeps the bits of the plain form.  No LDS is added.  mesh_normals_kernel is the same
// function on the caller's vertices.  scat_mano_fit_points_plane is icp_loop with a topology and the metric mesh fit.
#include "mano_fit_seq_common.h"

#include "../../include/scat_mano_fit_plane.h"
#include "../../include/scat_mano_fit_points.h"
#include "../../include/scat_mano_fit_seq_verts.h"
#include "mano_fit_seq_verts.h"
#include "mano_fit_verts.h"

namespace scat {

constexpr int kPMaxN = SCAT_FIT_POINTS_MAX_N;
constexpr int kPQ = 4;                      // points a thread walks at once
constexpr int kPWaves = kFThreads / 64;
static_assert(kPWaves == 4, "the totals add four wavefronts");

struct CloudArgs {
    ManoArgs m;            // kParams; rots / poses / betas are set by the kernel (LDS)
    const float* p;        // kParams: [B,62]
    const float* verts;    // otherwise: [B,V,3]
    const float* points;   // [B,N,3]
    const float* weights;  // [B,N] or null
    float max_dist;
    float* model_pts;      // kParams: [B,V,3] or null
    int* idx;              // [B,N]
    float* dist;           // [B,N]
    float* vw;             // [B,V]
    float* vtarget;        // [B,V,3]
    double* stats;         // [B,4]
    // scat_mano_fit_points: fold 1 zeroes acc_total, fold 2 adds the round's count to it; data_cost from the last assign
    const int* acc_round;
    int* acc_total;
    float* data_cost;
    int fold;
    int N, V;
    // kPlane (scat_mano_fit_plane.h): the topology, the normals of the model points, tau
    const int32_t* faces;
    const int32_t* vf_off;
    const int32_t* vf_idx;
    float* normals;        // [B,V,3]
    float w_tangent;
    int F;
};

template <bool kParams>
struct CloudPose {};
template <>
struct CloudPose<true> {
    ManoPose s;
    float p[kFU];
};

// the squared distance of the walk and of the data cost: every product and sum rounded once
__device__ __forceinline__ double cloud_d2(double qx, double qy, double qz, double x, double y, double z) {
#pragma clang fp contract(off)
    const double dx = qx - x, dy = qy - y, dz = qz - z;
    return (dx * dx + dy * dy) + dz * dz;
}

// kPlane, the metric data cost of a matched point: d2 its squared distance, (rx, ry, rz) = q - x, n the vertex normal as
// rounded to fp32 (not zero), tau the tangential weight.  scat_mano_fit_plane.h's rho, every product and sum rounded once
__device__ __forceinline__ double cloud_rho(double d2, double rx, double ry, double rz, const double (&n)[3], double tau) {
#pragma clang fp contract(off)
    const double nr = (n[0] * rx + n[1] * ry) + n[2] * rz;
    return tau * d2 + (1.0 - tau) * (nr * nr);
}

// The normal of vertex v of the mesh mp (x / y / z arrays) by scat_mano_fit_plane.h's rule: the cross products of the
// incident faces in vf_idx order and their sum in fp64 on the fp32 numbers, every product and sum rounded once, the
// quotients rounded to fp32 once.  A corrupt index skips the face; no read leaves faces[3 F], vf_off[V + 1], vf_idx[3 F]
__device__ __forceinline__ void mesh_vertex_normal(const float (*mp)[kMMaxV], const int32_t* faces, const int32_t* vf_off,
                                                   const int32_t* vf_idx, int V, int F, int v, float (&n)[3]) {
#pragma clang fp contract(off)
    double sx = 0.0, sy = 0.0, sz = 0.0;
    const int k0 = max(vf_off[v], 0), k1 = min(vf_off[v + 1], 3 * F);
    for (int k = k0; k < k1; ++k) {
        const int f = vf_idx[k];
        if (f < 0 || f >= F) continue;
        const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
        if ((unsigned)ia >= (unsigned)V || (unsigned)ib >= (unsigned)V || (unsigned)ic >= (unsigned)V) continue;
        const double ax = (double)mp[0][ia], ay = (double)mp[1][ia], az = (double)mp[2][ia];
        const double ux = (double)mp[0][ib] - ax, uy = (double)mp[1][ib] - ay, uz = (double)mp[2][ib] - az;
        const double wx = (double)mp[0][ic] - ax, wy = (double)mp[1][ic] - ay, wz = (double)mp[2][ic] - az;
        sx += uy * wz - uz * wy;
        sy += uz * wx - ux * wz;
        sz += ux * wy - uy * wx;
    }
    const double l2 = (sx * sx + sy * sy) + sz * sz;
    const bool ok = l2 > 0.0 && l2 < __builtin_huge_val();   // not zero, not NaN, not inf
    const double l = sqrt(l2);
    n[0] = ok ? (float)(sx / l) : 0.f;
    n[1] = ok ? (float)(sy / l) : 0.f;
    n[2] = ok ? (float)(sz / l) : 0.f;
}

// each of NQ points against all V vertices, ascending; the vertex address is wave-uniform
template <int NQ>
__device__ __forceinline__ void cloud_walk(const double (&qx)[kPQ], const double (&qy)[kPQ], const double (&qz)[kPQ],
                                           const float (*mp)[kMMaxV], int V, double (&best)[kPQ], int (&bi)[kPQ]) {
#pragma unroll 4
    for (int j = 0; j < V; ++j) {
        const double x = (double)mp[0][j], y = (double)mp[1][j], z = (double)mp[2][j];
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            const double d2 = cloud_d2(qx[k], qy[k], qz[k], x, y, z);
            if (d2 < best[k]) {
                best[k] = d2;
                bi[k] = j;
            }
        }
    }
}

// a hand that is not assigned.  All threads
__device__ __forceinline__ void cloud_unusable(const CloudArgs& a, int64_t b, bool zero_model) {
    const int tid = threadIdx.x, N = a.N, V = a.V;
    for (int n = tid; n < N; n += kFThreads) {
        a.idx[b * N + n] = -1;
        a.dist[b * N + n] = 0.f;
    }
    for (int v = tid; v < V; v += kFThreads) a.vw[b * V + v] = NAN;
    for (int i = tid; i < 3 * V; i += kFThreads) {
        a.vtarget[b * 3 * V + i] = 0.f;
        if (zero_model && a.model_pts) a.model_pts[b * 3 * V + i] = 0.f;
    }
    if (tid == 0) {
        double* st = a.stats + b * 4;
        st[0] = 2.0, st[1] = 0.0, st[2] = 0.0, st[3] = __builtin_huge_val();
        if (a.data_cost) a.data_cost[b] = INFINITY;
    }
}

// the normals of a hand that is not assigned (kPlane).  All threads
__device__ __forceinline__ void cloud_zero_normals(const CloudArgs& a, int64_t b) {
    for (int i = threadIdx.x; i < 3 * a.V; i += kFThreads) a.normals[b * 3 * a.V + i] = 0.f;
}

// grid = B, block = 256
template <bool kParams, bool kPlane = false>
__global__ __launch_bounds__(kFThreads) void cloud_assign_kernel(CloudArgs a) {
    __shared__ float mp[3][kMMaxV];      // the model points, x / y / z
    __shared__ alignas(16) int sidx[kPMaxN];   // the vertex of a matched point, -1 otherwise; read four at a time
    __shared__ CloudPose<kParams> ps;
    __shared__ double red[3][kPWaves];
    static_assert(sizeof(mp) + sizeof(sidx) + sizeof(CloudPose<kParams>) + sizeof(red) <= 64 * 1024, "static LDS");
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, N = a.N, V = a.V;
    const float* pts = a.points + b * 3 * (int64_t)N;
    const float* wts = a.weights ? a.weights + b * (int64_t)N : nullptr;
    if (tid == 0 && a.fold) a.acc_total[b] = a.fold == 1 ? 0 : a.acc_total[b] + a.acc_round[b];

    int bad = fit_unusable(pts, 3 * N, wts, N);
    if constexpr (kParams) {
        if (tid < kFU) {
            const float v = a.p[b * kFU + tid];
            ps.p[tid] = v;
            bad |= !fit_finite(v);
        }
    }
    if (__syncthreads_or(bad)) {   // the same for every thread of the workgroup
        cloud_unusable(a, b, true);
        if constexpr (kPlane) cloud_zero_normals(a, b);
        return;
    }

    // the model points
    bad = 0;
    if constexpr (kParams) {
        ManoArgs pm = a.m;
        pm.rots = ps.p, pm.poses = ps.p + 3, pm.betas = ps.p + 3 + kFPose;
        mano_setup(ps.s, pm, 0);
        const float sc = expf(ps.p[kFU - 1]);
        float Rg[9], tr[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) Rg[e] = ps.s.Rg[e];
#pragma unroll
        for (int c = 0; c < 3; ++c) tr[c] = ps.p[kFModel + c];
        for (int v = tid; v < V; v += kFThreads) {
            float vp[3], T[9], d[3], x[3];
            mano_vertex(ps.s, pm, v, vp, T, d);
            mv(Rg, d, x);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float mc = sc * x[c] + tr[c];
                mp[c][v] = mc;
                bad |= !fit_finite(mc);
                if (a.model_pts) a.model_pts[(b * V + v) * 3 + c] = mc;
            }
        }
    } else {
        const float* vs = a.verts + b * 3 * (int64_t)V;
        for (int i = tid; i < 3 * V; i += kFThreads) {
            const int v = i / 3, c = i - 3 * v;
            const float mc = vs[i];
            mp[c][v] = mc;
            bad |= !fit_finite(mc);
        }
    }
    if (__syncthreads_or(bad)) {   // (also the barrier that publishes mp)
        cloud_unusable(a, b, false);
        if constexpr (kPlane) cloud_zero_normals(a, b);
        return;
    }

    // the nearest vertex of every point
    const double md2 = (double)a.max_dist * (double)a.max_dist;
    for (int n0 = 0; n0 < N; n0 += kPQ * kFThreads) {
        const int nq = min(kPQ, (N - n0 + kFThreads - 1) / kFThreads);   // slots with a point in them: workgroup-uniform
        bool live[kPQ];
        double qx[kPQ], qy[kPQ], qz[kPQ], best[kPQ];
        int bi[kPQ];
#pragma unroll
        for (int k = 0; k < kPQ; ++k) {
            const int n = n0 + k * kFThreads + tid;
            live[k] = n < N && (wts ? wts[n] : 1.f) > 0.f;
            qx[k] = live[k] ? (double)pts[3 * n] : 0.0;
            qy[k] = live[k] ? (double)pts[3 * n + 1] : 0.0;
            qz[k] = live[k] ? (double)pts[3 * n + 2] : 0.0;
            best[k] = __builtin_huge_val();
            bi[k] = 0;
        }
        switch (nq) {
            case 1: cloud_walk<1>(qx, qy, qz, mp, V, best, bi); break;
            case 2: cloud_walk<2>(qx, qy, qz, mp, V, best, bi); break;
            case 3: cloud_walk<3>(qx, qy, qz, mp, V, best, bi); break;
            default: cloud_walk<4>(qx, qy, qz, mp, V, best, bi); break;
        }
#pragma unroll
        for (int k = 0; k < kPQ; ++k) {
            const int n = n0 + k * kFThreads + tid;
            if (n >= N) continue;
            a.idx[b * N + n] = live[k] ? bi[k] : -1;
            a.dist[b * N + n] = live[k] ? (float)sqrt(best[k]) : 0.f;
            sidx[n] = (live[k] && best[k] <= md2) ? bi[k] : -1;
        }
    }
    if (tid < 3 && N + tid < ((N + 3) & ~3)) sidx[N + tid] = -1;   // the last group of four
    __syncthreads();

    // per vertex: weight, centroid and cost of its matched points, n ascending
    double tot[3] = {0.0, 0.0, 0.0};   // matched weight, matched count, data cost
    for (int v = tid; v < V; v += kFThreads) {
        const double x = (double)mp[0][v], y = (double)mp[1][v], z = (double)mp[2][v];
        double W = 0.0, S[3] = {0.0, 0.0, 0.0}, C = 0.0;
        int cnt = 0;
        // kPlane: this vertex's normal from the LDS model points, into registers and to the caller, before the scan
        double nv[3] = {0.0, 0.0, 0.0};
        bool flat = true;
        if constexpr (kPlane) {
            float n[3];
            mesh_vertex_normal(mp, a.faces, a.vf_off, a.vf_idx, V, a.F, v, n);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                a.normals[(b * V + v) * 3 + c] = n[c];
                nv[c] = (double)n[c];
            }
            flat = n[0] == 0.f && n[1] == 0.f && n[2] == 0.f;
        }
        const auto take = [&](int n) {
            const double w = wts ? (double)wts[n] : 1.0;
            const double q0 = (double)pts[3 * n], q1 = (double)pts[3 * n + 1], q2 = (double)pts[3 * n + 2];
            W += w;
            S[0] += w * q0, S[1] += w * q1, S[2] += w * q2;   // fp32 x fp32: the products are exact in fp64
            if constexpr (kPlane) {
                const double d2 = cloud_d2(q0, q1, q2, x, y, z);
                C += w * (flat ? d2 : cloud_rho(d2, q0 - x, q1 - y, q2 - z, nv, (double)a.w_tangent));
            } else {
                C += w * cloud_d2(q0, q1, q2, x, y, z);
            }
            ++cnt;
        };
        // four indices per LDS read, two reads in flight: one index per read made a scan 130 cycles per point, the
        // latency of the read, and the scans two thirds of the kernel (profiles/fit_points_bench.txt)
        const int4* s4 = reinterpret_cast<const int4*>(sidx);
        const int groups = (N + 3) >> 2;
#pragma unroll 2
        for (int g = 0; g < groups; ++g) {
            const int4 c = s4[g];
            if (c.x == v || c.y == v || c.z == v || c.w == v) {
                if (c.x == v) take(4 * g);
                if (c.y == v) take(4 * g + 1);
                if (c.z == v) take(4 * g + 2);
                if (c.w == v) take(4 * g + 3);
            }
        }
        a.vw[b * V + v] = (float)W;
#pragma unroll
        for (int c = 0; c < 3; ++c) a.vtarget[(b * V + v) * 3 + c] = W > 0.0 ? (float)(S[c] / W) : 0.f;
        tot[0] += W, tot[1] += (double)cnt, tot[2] += C;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double t = tot[i];
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        if ((tid & 63) == 0) red[i][tid >> 6] = t;
    }
    __syncthreads();
    const double mw = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];   // the same bits on every thread
    if (!(mw > 0.0)) {   // nothing matched: the fit is to leave this hand alone
        for (int v = tid; v < V; v += kFThreads) a.vw[b * V + v] = NAN;   // each thread over the entries it wrote itself
    }
    if (tid == 0) {
        const double dc = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
        double* st = a.stats + b * 4;
        st[0] = 0.0;
        st[1] = mw;
        st[2] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        st[3] = dc;
        if (a.data_cost) a.data_cost[b] = (float)dc;
    }
}

// scat_mesh_normals: the caller's vertices into LDS, then mesh_vertex_normal per vertex.  grid = B, block = 256
__global__ __launch_bounds__(kFThreads) void mesh_normals_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                                 const int32_t* __restrict__ vf_off,
                                                                 const int32_t* __restrict__ vf_idx, float* __restrict__ normals,
                                                                 int V, int F) {
    __shared__ float mp[3][kMMaxV];
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const float* vs = verts + b * 3 * (int64_t)V;
    for (int i = tid; i < 3 * V; i += kFThreads) {
        const int v = i / 3, c = i - 3 * v;
        mp[c][v] = vs[i];
    }
    __syncthreads();
    for (int v = tid; v < V; v += kFThreads) {
        float n[3];
        mesh_vertex_normal(mp, faces, vf_off, vf_idx, V, F, v, n);
#pragma unroll
        for (int c = 0; c < 3; ++c) normals[(b * V + v) * 3 + c] = n[c];
    }
}

}  // namespace scat

using namespace scat;

// what the three entry points check alike, after the pointers that must not be null
static int cloud_check(const char* fn, const void* const* nullable, int nn, const double* stats, int N, float max_dist) {
    uintptr_t all = 0;
    for (int i = 0; i < nn; ++i) all |= (uintptr_t)nullable[i];
    SCAT_REQUIRE((all & 3) == 0, SCAT_E_ARG, "%s: fp32 operands must be 4-byte aligned", fn);
    SCAT_REQUIRE(((uintptr_t)stats & 7) == 0, SCAT_E_ARG, "%s: stats must be 8-byte aligned", fn);
    SCAT_REQUIRE(N >= 1 && N <= kPMaxN, SCAT_E_SHAPE, "%s: %d points outside 1..%d", fn, N, kPMaxN);
    SCAT_REQUIRE(max_dist > 0.f, SCAT_E_ARG, "%s: max_dist %g must be positive (+inf: no trim)", fn, (double)max_dist);
    return SCAT_OK;
}

template <bool kParams, bool kPlane = false>
static int cloud_launch(const char* fn, const CloudArgs& a, int B, void* stream) {
    hipLaunchKernelGGL((cloud_assign_kernel<kParams, kPlane>), dim3(B), dim3(kFThreads), 0, (hipStream_t)stream, a);
    SCAT_LAUNCH_CHECK(fn);
    return SCAT_OK;
}

// the topology of a plane entry point: the three arrays present and aligned, F in range, tau in 0..1
struct CloudTopo {
    const int32_t* faces;
    const int32_t* vf_off;
    const int32_t* vf_idx;
    int F;
    float w_tangent;
};

static int topo_check(const char* fn, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_idx, int F) {
    SCAT_REQUIRE(faces && vf_off && vf_idx, SCAT_E_ARG, "%s: null pointer", fn);
    SCAT_REQUIRE((((uintptr_t)faces | (uintptr_t)vf_off | (uintptr_t)vf_idx) & 3) == 0, SCAT_E_ARG,
                 "%s: int32 operands must be 4-byte aligned", fn);
    SCAT_REQUIRE(F >= 1 && F <= SCAT_RENDER_MAX_F, SCAT_E_SHAPE, "%s: %d faces outside 1..%d", fn, F, SCAT_RENDER_MAX_F);
    return SCAT_OK;
}

// The one filler of CloudArgs, for the three assignment entry points and the ICP loop.  m and p: the model's form, verts:
// the other; topo and normals: kPlane, or both null.  The ICP loop sets the fold and data_cost itself
static CloudArgs cloud_args(const ManoArgs& m, const float* p, const float* verts, const float* points, const float* weights,
                            float max_dist, float* model_pts, int* idx, float* dist, float* vw, float* vtarget, double* stats, int N,
                            int V, const CloudTopo* topo, float* normals) {
    CloudArgs a = {};
    a.m = m, a.p = p, a.verts = verts, a.points = points, a.weights = weights, a.max_dist = max_dist, a.model_pts = model_pts;
    a.idx = idx, a.dist = dist, a.vw = vw, a.vtarget = vtarget, a.stats = stats, a.N = N, a.V = V;
    if (topo) {
        a.faces = topo->faces, a.vf_off = topo->vf_off, a.vf_idx = topo->vf_idx, a.F = topo->F, a.w_tangent = topo->w_tangent;
        a.normals = normals;
    }
    return a;
}

extern "C" int scat_cloud_assign(const float* verts, const float* points, const float* weights, float max_dist, int* idx,
                                 float* dist, float* vw, float* vtarget, double* stats, int B, int N, int V, void* stream) {
    const char* fn = "scat_cloud_assign";
    const void* ptrs[] = {verts, points, idx, dist, vw, vtarget, stats};
    uintptr_t all = 0;
    for (const void* q : ptrs) {
        SCAT_REQUIRE(q, SCAT_E_ARG, "%s: null pointer", fn);
        all |= (uintptr_t)q;
    }
    SCAT_REQUIRE((all & 3) == 0, SCAT_E_ARG, "%s: fp32 operands must be 4-byte aligned", fn);
    SCAT_REQUIRE(B > 0, SCAT_E_SHAPE, "%s: batch %d must be positive", fn, B);
    SCAT_REQUIRE(V >= 1 && V <= kMMaxV, SCAT_E_SHAPE, "%s: %d vertices outside 1..%d", fn, V, kMMaxV);
    const void* nullable[] = {weights};
    int rc = cloud_check(fn, nullable, 1, stats, N, max_dist);
    if (rc != SCAT_OK) return rc;
    rc = cloud_launch<false>(fn, cloud_args({}, nullptr, verts, points, weights, max_dist, nullptr, idx, dist, vw, vtarget, stats, N, V,
                                            nullptr, nullptr), B, stream);
    if (rc != SCAT_OK) return rc;
    set_kernel_label("cloud_assign_v%d_n%d", V, N);
    return SCAT_OK;
}

// Both model forms of the assignment: the checks, then the launch.  topo null: scat_mano_cloud_assign
static int mano_assign(const char* fn, const CloudTopo* topo, const float* blend, const float* joint_t, const float* joint_s,
                       const float* weights_t, const float* hands_mean, const float* p, const float* points, const float* weights,
                       float max_dist, float* model_pts, float* normals, int* idx, float* dist, float* vw, float* vtarget,
                       double* stats, int B, int N, int V, uint64_t parents, void* stream) {
    const void* ptrs[] = {blend, joint_t, joint_s, weights_t, hands_mean, p, points, idx, dist, vw, vtarget, stats, normals};
    ManoArgs m = fit_model_args(blend, joint_t, joint_s, weights_t, hands_mean, V, parents, kNoTips);
    int rc = mano_validate(fn, ptrs, topo ? 13 : 12, B, V, parents, kNoTips, &m.levels);
    if (rc != SCAT_OK) return rc;
    const void* nullable[] = {weights, model_pts};
    rc = cloud_check(fn, nullable, 2, stats, N, max_dist);
    if (rc == SCAT_OK && topo) rc = topo_check(fn, topo->faces, topo->vf_off, topo->vf_idx, topo->F);
    if (rc == SCAT_OK && topo) rc = fit_check_tau(fn, topo->w_tangent);
    if (rc != SCAT_OK) return rc;
    const CloudArgs a = cloud_args(m, p, nullptr, points, weights, max_dist, model_pts, idx, dist, vw, vtarget, stats, N, V, topo, normals);
    return topo ? cloud_launch<true, true>(fn, a, B, stream) : cloud_launch<true>(fn, a, B, stream);
}

extern "C" int scat_mano_cloud_assign(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                      const float* hands_mean, const float* p, const float* points, const float* weights,
                                      float max_dist, float* model_pts, int* idx, float* dist, float* vw, float* vtarget,
                                      double* stats, int B, int N, int V, uint64_t parents, void* stream) {
    const int rc = mano_assign("scat_mano_cloud_assign", nullptr, blend, joint_t, joint_s, weights_t, hands_mean, p, points, weights,
                               max_dist, model_pts, nullptr, idx, dist, vw, vtarget, stats, B, N, V, parents, stream);
    if (rc != SCAT_OK) return rc;
    set_kernel_label("mano_cloud_assign_v%d_n%d", V, N);
    return SCAT_OK;
}

extern "C" int scat_mano_cloud_assign_plane(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                            const float* hands_mean, const float* p, const float* points, const float* weights,
                                            const int32_t* faces, const int32_t* vf_off, const int32_t* vf_idx, float max_dist,
                                            float w_tangent, float* model_pts, float* normals, int* idx, float* dist, float* vw,
                                            float* vtarget, double* stats, int B, int N, int V, int F, uint64_t parents,
                                            void* stream) {
    const CloudTopo topo = {faces, vf_off, vf_idx, F, w_tangent};
    const int rc = mano_assign("scat_mano_cloud_assign_plane", &topo, blend, joint_t, joint_s, weights_t, hands_mean, p, points,
                               weights, max_dist, model_pts, normals, idx, dist, vw, vtarget, stats, B, N, V, parents, stream);
    if (rc != SCAT_OK) return rc;
    set_kernel_label("mano_cloud_assign_plane_v%d_n%d_f%d", V, N, F);
    return SCAT_OK;
}

extern "C" int scat_mesh_normals(const float* verts, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_idx,
                                 float* normals, int B, int V, int F, void* stream) {
    const char* fn = "scat_mesh_normals";
    SCAT_REQUIRE(verts && normals, SCAT_E_ARG, "%s: null pointer", fn);
    SCAT_REQUIRE((((uintptr_t)verts | (uintptr_t)normals) & 3) == 0, SCAT_E_ARG, "%s: fp32 operands must be 4-byte aligned", fn);
    const int rc = topo_check(fn, faces, vf_off, vf_idx, F);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE(B > 0, SCAT_E_SHAPE, "%s: batch %d must be positive", fn, B);
    SCAT_REQUIRE(V >= 1 && V <= kMMaxV, SCAT_E_SHAPE, "%s: %d vertices outside 1..%d", fn, V, kMMaxV);
    hipLaunchKernelGGL(mesh_normals_kernel, dim3(B), dim3(kFThreads), 0, (hipStream_t)stream, verts, faces, vf_off, vf_idx, normals,
                       V, F);
    SCAT_LAUNCH_CHECK(fn);
    set_kernel_label("mesh_normals_v%d_f%d", V, F);
    return SCAT_OK;
}

// The workspace of an ICP loop over B hands: byte offsets, every part rounded up to 16 bytes.  The normals [B,V,3] follow
// the parts every loop has only in the plane form, and the track solve's workspace only for a track; a part that is not
// there takes no bytes
struct PointsWs { int64_t stats, vtarget, vw, cost, acc, idx, dist, normals, solve, total; };

static PointsWs points_ws(int64_t B, int64_t N, int64_t V, bool plane, int64_t solve_bytes) {
    PointsWs w;
    int64_t off = 0;
    const auto take = [&off](int64_t bytes) {
        const int64_t o = off;
        off += (bytes + 15) & ~(int64_t)15;
        return o;
    };
    w.stats = take(B * 4 * (int64_t)sizeof(double));
    w.vtarget = take(B * V * 3 * (int64_t)sizeof(float));
    w.vw = take(B * V * (int64_t)sizeof(float));
    w.cost = take(B * (int64_t)sizeof(float));
    w.acc = take(B * (int64_t)sizeof(int));
    w.idx = take(B * N * (int64_t)sizeof(int));
    w.dist = take(B * N * (int64_t)sizeof(float));
    w.normals = take(plane ? B * V * 3 * (int64_t)sizeof(float) : 0);
    w.solve = take(solve_bytes);
    w.total = off;
    return w;
}

extern "C" int64_t scat_mano_fit_points_ws(int B, int N, int V) {
    if (B < 1 || N < 1 || N > kPMaxN || V < 1 || V > kMMaxV) return 0;
    return points_ws(B, N, V, false, 0).total;
}

extern "C" int64_t scat_mano_fit_points_plane_ws(int B, int N, int V, int F) {
    if (B < 1 || N < 1 || N > kPMaxN || V < 1 || V > kMMaxV || F < 1 || F > SCAT_RENDER_MAX_F) return 0;
    return points_ws(B, N, V, true, 0).total;
}

extern "C" int64_t scat_mano_fit_points_seq_ws(int S, int T, int N, int V, int F) {
    if (S < 1 || T < 1 || T > SCAT_FIT_SEQ_MAX_T || N < 1 || N > kPMaxN || V < 1 || V > kMMaxV || F < 0 || F > SCAT_RENDER_MAX_F)
        return 0;
    const int64_t B = (int64_t)S * T;
    if (B > INT32_MAX) return 0;   // S T is the assignment's batch and a grid size
    return points_ws(B, N, V, F != 0, seq_verts_ws_bytes(S, T, V)).total;
}

// What an ICP entry point packs for icp_loop
struct IcpCall {
    const float *blend, *joint_t, *joint_s, *weights_t, *hands_mean;
    const float* points;     // [B,N,3]
    const float* weights;    // [B,N] or null
    const CloudTopo* topo;   // null: nearest vertex; otherwise point-to-plane
    float* p;                // [B,62]
    float* data_cost;        // [B]
    int* accepted;           // per hand [B], of a track [S]
    int* idx;                // [B,N] or null
    float* dist;             // [B,N] or null
    void* ws;
    int64_t ws_bytes;
    int S, T;                // a track (smooth not null): B = S T; otherwise B = S hands and T is not looked at
    int N, V;
    uint64_t parents;
    int rounds, iters;
    float max_dist, lambda0, w_pose, w_beta;
    const float* smooth;     // a track: its five weights, s_rots .. s_scale
    uint64_t free_mask;
    void* stream;
};

// The parts of the workspace that the solve between two assignments reads and writes
struct IcpParts {
    const float* vtarget;    // [B,V,3]
    const float* vw;         // [B,V]
    const float* normals;    // [B,V,3], or null without a topology
    const double* stats;     // [B,4]
    float* cost;             // [B]
    int* acc;                // [B]
    void* solve;             // the track solve's own workspace
    int64_t solve_bytes;
};

// Every ICP loop: the checks, the workspace, then rounds x {assign, solve} and one last assign: 2 rounds + 1 launches of
// the mesh fit, more of the track solve.  bind(parts) points the solve at the workspace and makes the solve's own checks,
// once; solve(r) is the launches of round r, unchecked.  Per hand each assign after the first adds the accepted count of
// the fit before it to the caller's total (fold); a track's counts add up in the track kernel
template <class Bind, class Solve>
static int icp_loop(const char* fn, const IcpCall& c, Bind&& bind, Solve&& solve) {
    const bool track = c.smooth != nullptr;
    const void* ptrs[] = {c.blend, c.joint_t, c.joint_s, c.weights_t, c.hands_mean, c.points, c.p, c.data_cost, c.accepted};
    ManoArgs m = fit_model_args(c.blend, c.joint_t, c.joint_s, c.weights_t, c.hands_mean, c.V, c.parents, kNoTips);
    int rc = mano_validate(fn, ptrs, 9, c.S, c.V, c.parents, kNoTips, &m.levels);
    if (rc != SCAT_OK) return rc;
    if (track) {
        rc = seq_check_frames(fn, c.T);
        if (rc != SCAT_OK) return rc;
        SCAT_REQUIRE((int64_t)c.S * c.T <= INT32_MAX, SCAT_E_SHAPE, "%s: %d sequences of %d frames are more than %d frames in all", fn,
                     c.S, c.T, INT32_MAX);
    }
    const void* nullable[] = {c.weights, c.idx, c.dist};
    rc = cloud_check(fn, nullable, 3, nullptr, c.N, c.max_dist);
    if (rc == SCAT_OK && c.topo) rc = topo_check(fn, c.topo->faces, c.topo->vf_off, c.topo->vf_idx, c.topo->F);
    if (rc == SCAT_OK && c.topo) rc = fit_check_tau(fn, c.topo->w_tangent);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE(c.rounds >= 1 && c.rounds <= SCAT_FIT_POINTS_MAX_ROUNDS, SCAT_E_ARG, "%s: %d rounds outside 1..%d", fn, c.rounds,
                 SCAT_FIT_POINTS_MAX_ROUNDS);
    rc = fit_check_solver(fn, "none: the start is the caller's", c.iters, 0, c.lambda0, c.w_pose, c.w_beta);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE(c.rounds * c.iters <= SCAT_FIT_POINTS_MAX_STEPS, SCAT_E_ARG, "%s: %d rounds of %d iterations are more than %d steps",
                 fn, c.rounds, c.iters, SCAT_FIT_POINTS_MAX_STEPS);
    if (track) rc = seq_check_smooth(fn, c.smooth, kSeqVertsSmooth, 5);
    if (rc == SCAT_OK) rc = fit_check_mask(fn, c.free_mask);
    if (rc != SCAT_OK) return rc;
    const int B = track ? c.S * c.T : c.S;
    const PointsWs w = points_ws(B, c.N, c.V, c.topo != nullptr, track ? seq_verts_ws_bytes(c.S, c.T, c.V) : 0);
    rc = seq_check_ws(fn, c.ws, c.ws_bytes, w.total);
    if (rc != SCAT_OK) return rc;

    const auto part = [&c](int64_t off) { return static_cast<void*>(static_cast<char*>(c.ws) + off); };
    float* const vtarget = static_cast<float*>(part(w.vtarget));
    float* const vw = static_cast<float*>(part(w.vw));
    float* const normals = c.topo ? static_cast<float*>(part(w.normals)) : nullptr;
    double* const stats = static_cast<double*>(part(w.stats));
    const IcpParts parts = {vtarget, vw, normals, stats, static_cast<float*>(part(w.cost)), static_cast<int*>(part(w.acc)),
                            part(w.solve), c.ws_bytes - w.solve};
    CloudArgs a = cloud_args(m, c.p, nullptr, c.points, c.weights, c.max_dist, nullptr, c.idx ? c.idx : static_cast<int*>(part(w.idx)),
                             c.dist ? c.dist : static_cast<float*>(part(w.dist)), vw, vtarget, stats, c.N, c.V, c.topo, normals);
    if (!track) a.acc_round = parts.acc, a.acc_total = c.accepted;
    rc = bind(parts);
    if (rc != SCAT_OK) return rc;
    for (int r = 0; r <= c.rounds; ++r) {
        a.fold = track ? 0 : r == 0 ? 1 : 2;   // 1 zeroes the total, 2 adds the round before
        a.data_cost = r == c.rounds ? c.data_cost : nullptr;
        rc = c.topo ? cloud_launch<true, true>(fn, a, B, c.stream) : cloud_launch<true>(fn, a, B, c.stream);
        if (rc != SCAT_OK || r == c.rounds) return rc;
        rc = solve(r);
        if (rc != SCAT_OK) return rc;
    }
    return SCAT_OK;
}

// Both per-hand loops: icp_loop around the mesh fit, the metric one with a topology
static int hand_icp(const char* fn, const char* label, const IcpCall& c) {
    VertsCall v = {c.blend, c.joint_t, c.joint_s, c.weights_t, c.hands_mean, nullptr, nullptr, nullptr, c.p, nullptr, nullptr, c.S, c.V,
                   c.parents, c.iters, 0, c.topo != nullptr, c.topo ? c.topo->w_tangent : 1.f, c.lambda0, c.w_pose, c.w_beta,
                   c.free_mask, 0, c.stream};
    int levels = 0;
    const int rc = icp_loop(
        fn, c,
        [&](const IcpParts& w) {
            v.targets = w.vtarget, v.weights = w.vw, v.normals = w.normals, v.cost = w.cost, v.accepted = w.acc;
            return fit_verts_check(fn, v, &levels);
        },
        [&](int) { return fit_verts_launch(fn, v, levels); });
    if (rc != SCAT_OK) return rc;
    set_kernel_label(label, c.V, c.N, c.rounds, c.iters);
    return SCAT_OK;
}

extern "C" int scat_mano_fit_points(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                    const float* hands_mean, const float* points, const float* weights, float* p,
                                    float* data_cost, int* accepted, int* idx, float* dist, void* ws, int64_t ws_bytes, int B,
                                    int N, int V, uint64_t parents, int rounds, int iters, float max_dist, float lambda0,
                                    float w_pose, float w_beta, uint64_t free_mask, void* stream) {
    return hand_icp("scat_mano_fit_points", "mano_fit_points_v%d_n%d_r%d_i%d",
                    {blend, joint_t, joint_s, weights_t, hands_mean, points, weights, nullptr, p, data_cost, accepted, idx, dist, ws,
                     ws_bytes, B, 0, N, V, parents, rounds, iters, max_dist, lambda0, w_pose, w_beta, nullptr, free_mask, stream});
}

extern "C" int scat_mano_fit_points_plane(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                          const float* hands_mean, const float* points, const float* weights,
                                          const int32_t* faces, const int32_t* vf_off, const int32_t* vf_idx, float* p,
                                          float* data_cost, int* accepted, int* idx, float* dist, void* ws, int64_t ws_bytes, int B,
                                          int N, int V, int F, uint64_t parents, int rounds, int iters, float max_dist,
                                          float w_tangent, float lambda0, float w_pose, float w_beta, uint64_t free_mask,
                                          void* stream) {
    const CloudTopo topo = {faces, vf_off, vf_idx, F, w_tangent};
    return hand_icp("scat_mano_fit_points_plane", "mano_fit_points_plane_v%d_n%d_r%d_i%d",
                    {blend, joint_t, joint_s, weights_t, hands_mean, points, weights, &topo, p, data_cost, accepted, idx, dist, ws,
                     ws_bytes, B, 0, N, V, parents, rounds, iters, max_dist, lambda0, w_pose, w_beta, nullptr, free_mask, stream});
}

// ICP over a track of clouds, include/scat_mano_fit_seq_verts.h: icp_loop with the S T frames as the assignment's batch and
// mano_fit_seq_verts.hip's track solve in place of the per-hand fit.  The assignment's stats go to the solve, which bridges
// a frame where nothing matched and refuses the sequence of an unusable one
extern "C" int scat_mano_fit_points_seq(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                        const float* hands_mean, const float* points, const float* weights, const int32_t* faces,
                                        const int32_t* vf_off, const int32_t* vf_idx, float* p, float* data_cost, int* accepted,
                                        int* idx, float* dist, void* ws, int64_t ws_bytes, int S, int T, int N, int V, int F,
                                        uint64_t parents, int rounds, int iters, float max_dist, float w_tangent, float lambda0,
                                        float w_pose, float w_beta, float s_rots, float s_poses, float s_betas, float s_trans,
                                        float s_scale, uint64_t free_mask, void* stream) {
    const char* fn = "scat_mano_fit_points_seq";
    const CloudTopo topo = {faces, vf_off, vf_idx, F, w_tangent};
    const bool plane = faces || vf_off || vf_idx || F != 0;
    SeqVertsCall q = {blend, joint_t, joint_s, weights_t, hands_mean, nullptr, nullptr, nullptr, nullptr, p, nullptr, accepted,
                      nullptr, 0, S, T, V, parents, iters, 0, w_tangent, lambda0, w_pose, w_beta,
                      {s_rots, s_poses, s_betas, s_trans, s_scale}, free_mask, 0, stream};
    const IcpCall c = {blend, joint_t, joint_s, weights_t, hands_mean, points, weights, plane ? &topo : nullptr, p, data_cost, accepted,
                       idx, dist, ws, ws_bytes, S, T, N, V, parents, rounds, iters, max_dist, lambda0, w_pose, w_beta, q.smooth,
                       free_mask, stream};
    int levels = 0;
    const int rc = icp_loop(
        fn, c,
        [&](const IcpParts& w) {
            q.targets = w.vtarget, q.weights = w.vw, q.normals = w.normals, q.stats = w.stats, q.cost = w.cost;
            q.ws = w.solve, q.ws_bytes = w.solve_bytes;
            return seq_verts_check(fn, q, &levels);
        },
        [&](int r) {
            q.acc_add = r > 0;
            return seq_verts_launch(fn, q, levels);
        });
    if (rc != SCAT_OK) return rc;
    set_kernel_label(plane ? "mano_fit_points_seq_plane_v%d_n%d_t%d_r%d_i%d" : "mano_fit_points_seq_v%d_n%d_t%d_r%d_i%d", V, N, T,
                     rounds, iters);
    return SCAT_OK;
}
