// The MANO fit to a track of meshes, include/scat_mano_fit_seq_verts.h: mano_fit_verts.hip's data term in every frame and
// mano_fit_seq.hip's coupling between consecutive frames, as one Levenberg-Marquardt per sequence.  A frame has 3 V rows,
// not 63, so the solve is split where the two track kernels of 63-row frames are not:
//   frame kernel   grid S T, one workgroup of 256 threads per frame.  mano_fit_verts_kernel's tile loop (vj_setup,
//                  vj_stage, vj_cols, the 231 owners of 3 x 3 blocks, fp32 within a tile, fp64 across tiles, kMetric on the
//                  tile writers) at the point the sequence's state names, and no solver: the frame's undamped A_t (lower
//                  triangle, priors on the diagonal) and g_t (row 62) go to the workspace, with the frame's cost.  The data
//                  cost is entry (62, 62) of [J r]^T [J r], which the owner of block (20, 20) forms anyway; that one entry
//                  is added in fp64 throughout.  Its start form (init = 1) is vfit_procrustes per frame.
//   track kernel   grid S, one workgroup per sequence, no model.  Decides on the previous trial (the T frame costs and the
//                  smoothness, seq_cost_add on one thread, then seq_decide on the state kept in the workspace), then walks
//                  the frames: A_t and g_t from the workspace, smoothness, the unit rows of frozen unknowns and Marquardt's
//                  1 + lambda added in LDS, seq_eliminate forward, seq_backward into the trial buffer.  Its scan form
//                  (init = 1) is fit_start_scan; its last call only decides and writes the results.
// A_t, g_t stand undamped in two buffers, the current point's and the trial's, that swap with the unknowns' on an accepted
// step: a rejected step re-solves from what is there.  Everything a later launch needs of an earlier one is in the
// workspace; the stream orders them.  No atomics; every sum in an order fixed by the sizes.
// Host: seq_verts_check is every refusal, seq_verts_launch the 2 iters + 2 launches (mano_fit_seq_verts.h); the entry point
// runs both, the ICP loop over a track of clouds (mano_fit_points.hip) the first once and the second once per round.
#include "mano_fit_seq_common.h"
#include "mano_fit_verts_common.h"

#include "../../include/scat_mano_fit_seq_verts.h"
#include "mano_fit_seq_verts.h"
#include "mano_fit_verts.h"

namespace scat {

enum { kSVAssemble = 0, kSVStart = 1, kSVScan = 2 };
enum { kSVBad = 1, kSVHas = 2, kSVNoData = 4 };   // a frame's state

struct SVState {   // a sequence's state, 32 bytes
    float lambda, cost;
    int cur, acc, fail, refused, pad[2];
};

struct SVArgs {
    ManoArgs m;   // frame kernel; rots / poses / betas are set by the kernel (LDS)
    const float* targets;
    const float* weights;
    const float* normals;   // kMetric: [S,T,V,3]
    const double* stats;    // [S T,4] or null
    float* p;
    float* cost;
    int* accepted;
    float* walk;     // mano_fit_seq_common.h's layout: L_t, M_t^T, two buffers of the unknowns
    float* ag;       // [S][2][T][63][62]: A_t with g_t at the point of the unknowns' buffer of the same index
    float* fcost;    // [S][T]: the frame's cost at the point the frame kernel last ran at
    int* fstate;     // [S][T]
    SVState* state;  // [S]
    int T, init, mode, first, last, acc_add;
    float w_tangent, lambda0, w_pose, w_beta;
    float s_rots, s_poses, s_betas, s_trans, s_scale;
    uint64_t free_mask;
};

__device__ __forceinline__ float sv_weight(const SVArgs& a, int i) {
    return i < 3 ? a.s_rots : i < 3 + kFPose ? a.s_poses : i < kFModel ? a.s_betas : i < kFU - 1 ? a.s_trans : a.s_scale;
}

__device__ __forceinline__ float* sv_ag(const SVArgs& a, int64_t s, int buf) {
    return a.ag + (s * 2 + buf) * ((int64_t)a.T * kSeqL<kFU>);
}

// grid = S T, block = 256
template <bool kMetric>
__global__ __launch_bounds__(kFThreads) void mano_fit_seq_verts_frame_kernel(SVArgs a) {
    __shared__ JacLds m;
    __shared__ VertStage<kVTile> g;
    __shared__ alignas(8) float tile[3 * kVTile][kVCols];   // the weighted rows [J r] of a tile; the start's moments before
    __shared__ float fp[kFU];
    static_assert(sizeof(JacLds) + sizeof(VertStage<kVTile>) + sizeof(tile) + sizeof(fp) <= 64 * 1024, "static LDS");
    static_assert(sizeof(tile) >= kVWaves * kVMoments * sizeof(double), "the moments fit the tile");
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, V = a.m.V, T = a.T;
    const int64_t s = b / T;
    const int t = (int)(b - s * T);
    const int np = T * kFU;
    const float* tgt = a.targets + b * 3 * (int64_t)V;
    const float* wts = a.weights ? a.weights + b * (int64_t)V : nullptr;
    const float* nrm = nullptr;
    float ma = 1.f;
    if constexpr (kMetric) {
        nrm = a.normals + b * 3 * (int64_t)V;
        ma = sqrtf(a.w_tangent);
    }
    float* const wp = seq_ws_start<kFU>(a.walk, s, T, 0);   // the two buffers of the sequence's unknowns
    ManoArgs pc = a.m;
    pc.rots = fp, pc.poses = fp + 3, pc.betas = fp + 3 + kFPose;

    if (a.mode == kSVStart) {   // the frame's own start into the first buffer, and whether it has weight
        int bad = fit_unusable(tgt, 3 * V, wts, V), has = wts ? 0 : 1;
        if (wts) {
            for (int i = tid; i < V; i += kFThreads) has |= wts[i] > 0.f;
        }
        if (tid < kFU) fp[tid] = 0.f;
        bad = __syncthreads_or(bad);
        has = __syncthreads_or(has);
        if (!bad) {
            vj_setup(m, pc, 0, false);   // the zero pose
            vfit_procrustes(m.s, pc, tgt, wts, reinterpret_cast<double*>(&tile[0][0]), fp);
        }
        if (tid < kFU) wp[t * kFU + tid] = fp[tid];
        if (tid == 0) a.fstate[b] = (bad ? kSVBad : 0) | (has ? kSVHas : 0);
        return;
    }

    int buf = 0, nodata = 0;
    if (!a.first) {
        if (a.state[s].refused) return;   // the same for every thread of the workgroup
        buf = 1 - a.state[s].cur;         // the trial
        nodata = a.fstate[b] & kSVNoData;
    }
    const float* src = (a.first && !a.init) ? a.p + b * kFU : wp + buf * np + t * kFU;
    int bad = 0;
    if (tid < kFU) {
        const float v = src[tid];
        fp[tid] = v;
        bad = !fit_finite(v);
        if (a.first && !a.init) wp[t * kFU + tid] = v;
    }
    if (a.first) {   // usable inputs: once per solve
        if (a.stats) {
            if (a.stats[4 * b] != 0.0) bad = 1;
            else if (!(a.stats[4 * b + 1] > 0.0)) nodata = kSVNoData;   // nothing matched: its weights are a NaN row
        }
        bad |= fit_unusable(tgt, 3 * V, nodata ? nullptr : wts, V);
        if constexpr (kMetric) bad |= fit_unusable(nrm, 3 * V, nullptr, 0);
        bad = __syncthreads_or(bad);
        if (tid == 0) a.fstate[b] = (bad ? kSVBad : 0) | nodata;
        if (bad) return;   // the same for every thread of the workgroup
    }

    vj_ancestors(m, a.m.parents);
    int bi0, bj0;   // this thread's block of [J r]^T [J r]
    vfit_block(tid, bi0, bj0);
    const bool cost_owner = tid == kVOwners - 1;   // block (20, 20): entry (62, 62) is the data cost
    double tot[3][3], cst = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) tot[i][j] = 0.0;
    if (!nodata) {
        vj_setup(m, pc, 0, true);
        const float sc = expf(fp[kFU - 1]);
        float Rg[9], tr[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) Rg[e] = m.s.Rg[e];
#pragma unroll
        for (int c = 0; c < 3; ++c) tr[c] = fp[kFModel + c];
        for (int v0 = 0; v0 < V; v0 += kVTile) {
            const int nv = min(kVTile, V - v0);
            vj_stage(m.s, pc, g, v0, nv);
            for (int w = tid; w < kMJ * kVTile; w += kFThreads) {
                const int vl = w % kVTile, k = w / kVTile, v = v0 + vl;
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
                    if (cost_owner) cst += (double)ra[2] * (double)rb[2];   // the squares of the residual column, in fp64
                }
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) tot[i][j] += (double)acc[i][j];
            }
        }
    } else {
        __syncthreads();   // fp
    }
    // A_t = J^T W J + priors (lower triangle), g_t = J^T W r + the priors' gradient as row 62: undamped, nothing frozen
    if (tid < kVOwners) {
        float* A = sv_ag(a, s, buf) + (int64_t)t * kSeqL<kFU>;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int ai = 3 * bi0 + i, bi = 3 * bj0 + j;
                if (bi > ai || bi >= kFU) continue;
                float sum = (float)tot[i][j];
                if (ai == kFU) {
                    if (bi >= 3 && bi < kFModel) sum += (bi < 3 + kFPose ? a.w_pose : a.w_beta) * fp[bi];
                } else if (ai == bi) {
                    if (ai >= 3 && ai < kFModel) sum += ai < 3 + kFPose ? a.w_pose : a.w_beta;
                }
                A[ai * kFU + bi] = sum;
            }
    }
    if (cost_owner) {   // the data term, then the priors: their 55 squares in fp64, rounded once, as vfit_cost has them
        double sp = 0.0, sb = 0.0;
        for (int i = 3; i < 3 + kFPose; ++i) sp += (double)fp[i] * fp[i];
        for (int i = 3 + kFPose; i < kFModel; ++i) sb += (double)fp[i] * fp[i];
        a.fcost[b] = (float)(cst + ((double)a.w_pose * sp + (double)a.w_beta * sb));
    }
}

struct TrackLds {
    float M[kFU][kFU];       // M_t^T
    float A[kFU + 1][kFU];   // lower triangle: H_t, then L_t; row 62: g_t, then y_t
    float col[kFU + 1];
    float delta[kFU];
    float p[kFU];            // the frame's unknowns
    float pp[kFU], pn[kFU];  // the same of the frame before and of the frame after
    float yp[kFU], xn[kFU];  // y_t-1 (forward), x_t+1 (backward)
    float dc[kFU], ds[kFU];  // the smoothness weights in the cost, and in the system (zero for a frozen unknown)
    float cost, lambda;
    float cd, cs;            // the running data and smoothness sums of the decision
    int acc, fail, fin, cur, bad;
    unsigned char has[kSeqMaxT];   // the scan: the frame has weight
};

// the results of sequence s.  All threads
__device__ __forceinline__ void sv_write(const SVArgs& a, int64_t s, float cost, int acc) {
    if (threadIdx.x == 0) {
        a.cost[s] = fit_finite(cost) ? cost : INFINITY;   // also NaN
        a.accepted[s] = (a.acc_add ? a.accepted[s] : 0) + acc;
    }
}

// grid = S, block = 256
__global__ __launch_bounds__(kFThreads) void mano_fit_seq_verts_track_kernel(SVArgs a) {
    __shared__ TrackLds f;
    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x, T = a.T;
    float* const wl = seq_ws_l<kFU>(a.walk, s, T);   // L_t and y_t
    float* const wm = seq_ws_m<kFU>(wl, T);          // M_t^T, t >= 1
    float* const wp = seq_ws_p<kFU>(wm, T);          // the unknowns: two buffers of [T][62]
    const int* const fs = a.fstate + s * T;
    const float* const fc = a.fcost + s * T;
    float* const pg = a.p + s * T * kFU;
    SVState* const st = a.state + s;
    const int np = T * kFU;
    const uint64_t fm = a.free_mask;

    if (a.mode == kSVScan) {   // init = 1, after every frame's own start
        int bad = 0;
        for (int t = tid; t < T; t += kFThreads) {
            bad |= fs[t] & kSVBad;
            f.has[t] = (fs[t] & kSVHas) != 0;
        }
        bad = __syncthreads_or(bad);
        if (!bad && tid == 0) fit_start_scan<kFU>(f.has, wp, T);
        return;
    }

    if (tid >= 64 && tid < 64 + kFU) {
        const int i = tid - 64;
        const float d = sv_weight(a, i);
        f.dc[i] = d;
        f.ds[i] = ((fm >> i) & 1u) ? d : 0.f;
    }
    if (a.first) {
        int bad = 0;
        for (int t = tid; t < T; t += kFThreads) bad |= fs[t] & kSVBad;
        bad = __syncthreads_or(bad);
        if (tid == 0) {
            f.acc = 0, f.cur = 0, f.fail = 0, f.bad = bad;
            f.lambda = a.lambda0;
            f.cost = INFINITY;
        }
    } else if (tid == 0) {
        f.acc = st->acc, f.cur = st->cur, f.fail = st->fail, f.bad = st->refused;
        f.lambda = st->lambda;
        f.cost = st->cost;
    }
    __syncthreads();
    if (f.bad) {   // the same for every thread of the workgroup: the sequence is not fitted
        if (a.first && tid == 0) st->refused = 1;
        if (a.last) {
            if (a.init)
                for (int i = tid; i < np; i += kFThreads) pg[i] = 0.f;
            sv_write(a, s, INFINITY, 0);
        }
        return;
    }

    // the cost of the point the frame kernel last ran at: the start, or the trial
    {
        const float* Q = wp + (a.first ? 0 : 1 - f.cur) * np;
        if (tid == 0) {
            f.cd = 0.f, f.cs = 0.f;
            f.fin = 1;
        }
        for (int t = 0; t < T; ++t) {   // only the running sums need one thread: the finite check is the barrier's
            int fin = 1;
            if (tid < kFU) {
                const float v = Q[t * kFU + tid];
                f.p[tid] = v;
                f.pp[tid] = t > 0 ? Q[(t - 1) * kFU + tid] : 0.f;
                fin = fit_finite(v);
            }
            fin = __syncthreads_and(fin);
            if (tid == 0) {
                seq_cost_add<kFU>(f, fc[t], f.p, f.pp, t);
                f.fin &= fin;
            }
            __syncthreads();
        }
        if (tid == 0) {
            if (a.first) f.cost = f.cd + f.cs;
            else seq_decide(f);
            st->lambda = f.lambda, st->cost = f.cost;
            st->cur = f.cur, st->acc = f.acc, st->refused = 0;
            f.fail = 0;
        }
        __syncthreads();
    }
    const float* P = wp + f.cur * np;        // the current unknowns
    float* Q = wp + (1 - f.cur) * np;        // the trial's
    if (a.last) {   // a sequence without an accepted step keeps the caller's p
        if (a.init || f.acc > 0)
            for (int i = tid; i < np; i += kFThreads) pg[i] = P[i];
        sv_write(a, s, f.cost, f.acc);
        return;
    }

    // forward: H_t from the undamped A_t of the current point, eliminate the frame before, factor
    const float* AG = sv_ag(a, s, f.cur);
    for (int t = 0; t < T; ++t) {
        const float ct = (t > 0 ? 1.f : 0.f) + (t < T - 1 ? 1.f : 0.f);
        const float* At = AG + (int64_t)t * kSeqL<kFU>;
        seq_stage_unknowns<kFU>(f, P, f.p, t, T, 0);
        __syncthreads();
        for (int w = tid; w < (kFU + 1) * kFU; w += kFThreads) {
            const int ai = w / kFU, bi = w % kFU;
            const bool fb = (fm >> bi) & 1u;
            float v = 0.f;
            if (ai == kFU) {
                float gq = At[w];
                if (t > 0) gq += f.ds[bi] * (f.p[bi] - f.pp[bi]);
                if (t < T - 1) gq += f.ds[bi] * (f.p[bi] - f.pn[bi]);
                v = fb ? gq : 0.f;
            } else if (bi <= ai) {
                const bool fa = (fm >> ai) & 1u;
                float sum = At[w];
                if (ai == bi) {
                    sum += ct * f.ds[ai];
                    sum *= 1.f + f.lambda;   // Marquardt: the full diagonal, smoothness included
                }
                v = (fa && fb) ? sum : (ai == bi ? 1.f : 0.f);
            }
            (&f.A[0][0])[w] = v;
        }
        __syncthreads();
        seq_eliminate<kFU>(f, wl, wm, t, T);
    }
    // backward: x_t, and the trial unknowns
    for (int t = T - 1; t >= 0; --t) seq_backward<kFU>(f, wl, wm, P, Q, t, T, tid < kFU && ((fm >> tid) & 1u));
    if (tid == 0) st->fail = f.fail;
}

}  // namespace scat

using namespace scat;

// the workspace: byte offsets, every part rounded up to 16 bytes
struct SeqVertsWs { int64_t walk, ag, fcost, fstate, state, total; };

static SeqVertsWs seq_verts_layout(int64_t S, int64_t T) {
    SeqVertsWs w;
    int64_t off = 0;
    const auto take = [&off](int64_t bytes) {
        const int64_t o = off;
        off += (bytes + 15) & ~(int64_t)15;
        return o;
    };
    w.walk = take(S * T * kSeqFrame<kFU> * (int64_t)sizeof(float));
    w.ag = take(S * T * 2 * kSeqL<kFU> * (int64_t)sizeof(float));
    w.fcost = take(S * T * (int64_t)sizeof(float));
    w.fstate = take(S * T * (int64_t)sizeof(int));
    w.state = take(S * (int64_t)sizeof(SVState));
    w.total = off;
    return w;
}
static_assert(sizeof(SVState) == 32, "the header says 32 bytes per sequence");

int64_t seq_verts_ws_bytes(int S, int T, int V) {
    if (S < 1 || T < 1 || T > kSeqMaxT || V < 1 || V > kMMaxV || (int64_t)S * T > INT32_MAX) return 0;   // S T is a grid size
    return seq_verts_layout(S, T).total;
}

int seq_verts_check(const char* fn, const SeqVertsCall& c, int* levels) {
    const void* ptrs[] = {c.blend, c.joint_t, c.joint_s, c.weights_t, c.hands_mean, c.targets, c.p, c.cost, c.accepted};
    int rc = mano_validate(fn, ptrs, 9, c.S, c.V, c.parents, kNoTips, levels);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE((((uintptr_t)c.weights | (uintptr_t)c.normals) & 3) == 0, SCAT_E_ARG, "%s: fp32 operands must be 4-byte aligned", fn);
    SCAT_REQUIRE(((uintptr_t)c.stats & 7) == 0, SCAT_E_ARG, "%s: stats must be 8-byte aligned", fn);
    rc = seq_check_frames(fn, c.T);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE((int64_t)c.S * c.T <= INT32_MAX, SCAT_E_SHAPE, "%s: %d sequences of %d frames are more than %d frames in all", fn,
                 c.S, c.T, INT32_MAX);
    rc = fit_check_solver(fn, "Procrustes over the vertices, frame by frame", c.iters, c.init, c.lambda0, c.w_pose, c.w_beta);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE(!(c.init && c.normals), SCAT_E_ARG, "%s: init 1 is the Euclidean fit's: with normals the start is the caller's", fn);
    if (c.normals) rc = fit_check_tau(fn, c.w_tangent);
    if (rc == SCAT_OK) rc = seq_check_smooth(fn, c.smooth, kSeqVertsSmooth, 5);
    if (rc == SCAT_OK) rc = fit_check_mask(fn, c.free_mask);
    if (rc == SCAT_OK) rc = seq_check_ws(fn, c.ws, c.ws_bytes, seq_verts_ws_bytes(c.S, c.T, c.V));
    return rc;
}

int seq_verts_launch(const char* fn, const SeqVertsCall& c, int levels) {
    SVArgs a = {};
    a.m = fit_model_args(c.blend, c.joint_t, c.joint_s, c.weights_t, c.hands_mean, c.V, c.parents, kNoTips);
    a.m.levels = levels;
    const SeqVertsWs w = seq_verts_layout(c.S, c.T);
    char* base = static_cast<char*>(c.ws);
    a.targets = c.targets, a.weights = c.weights, a.normals = c.normals, a.stats = c.stats;
    a.p = c.p, a.cost = c.cost, a.accepted = c.accepted;
    a.walk = reinterpret_cast<float*>(base + w.walk), a.ag = reinterpret_cast<float*>(base + w.ag);
    a.fcost = reinterpret_cast<float*>(base + w.fcost), a.fstate = reinterpret_cast<int*>(base + w.fstate);
    a.state = reinterpret_cast<SVState*>(base + w.state);
    a.T = c.T, a.init = c.init, a.acc_add = c.acc_add;
    a.w_tangent = c.w_tangent, a.lambda0 = c.lambda0, a.w_pose = c.w_pose, a.w_beta = c.w_beta;
    a.s_rots = c.smooth[0], a.s_poses = c.smooth[1], a.s_betas = c.smooth[2], a.s_trans = c.smooth[3], a.s_scale = c.smooth[4];
    a.free_mask = c.free_mask;
    const dim3 frames(c.S * c.T), tracks(c.S), block(kFThreads);
    hipStream_t stream = (hipStream_t)c.stream;
    const bool metric = c.normals != nullptr;
    const auto frame = [&](int mode, int first) {
        a.mode = mode, a.first = first, a.last = 0;
        if (metric) hipLaunchKernelGGL((mano_fit_seq_verts_frame_kernel<true>), frames, block, 0, stream, a);
        else hipLaunchKernelGGL((mano_fit_seq_verts_frame_kernel<false>), frames, block, 0, stream, a);
    };
    const auto track = [&](int mode, int first, int last) {
        a.mode = mode, a.first = first, a.last = last;
        hipLaunchKernelGGL(mano_fit_seq_verts_track_kernel, tracks, block, 0, stream, a);
    };
    if (c.init) {
        frame(kSVStart, 0);
        SCAT_LAUNCH_CHECK(fn);
        track(kSVScan, 0, 0);
        SCAT_LAUNCH_CHECK(fn);
    }
    frame(kSVAssemble, 1);
    SCAT_LAUNCH_CHECK(fn);
    for (int it = 0; it < c.iters; ++it) {
        track(kSVAssemble, it == 0, 0);
        SCAT_LAUNCH_CHECK(fn);
        frame(kSVAssemble, 0);
        SCAT_LAUNCH_CHECK(fn);
    }
    track(kSVAssemble, 0, 1);
    SCAT_LAUNCH_CHECK(fn);
    return SCAT_OK;
}

extern "C" int64_t scat_mano_fit_seq_verts_ws(int S, int T, int V) {
    return seq_verts_ws_bytes(S, T, V);
}

extern "C" int scat_mano_fit_seq_verts(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                       const float* hands_mean, const float* targets, const float* weights, const float* normals,
                                       float* p, float* cost, int* accepted, void* ws, int64_t ws_bytes, int S, int T, int V,
                                       uint64_t parents, int iters, int init, float w_tangent, float lambda0, float w_pose,
                                       float w_beta, float s_rots, float s_poses, float s_betas, float s_trans, float s_scale,
                                       uint64_t free_mask, void* stream) {
    const SeqVertsCall c = {blend, joint_t, joint_s, weights_t, hands_mean, targets, weights, normals, nullptr, p, cost, accepted,
                            ws, ws_bytes, S, T, V, parents, iters, init, w_tangent, lambda0, w_pose, w_beta,
                            {s_rots, s_poses, s_betas, s_trans, s_scale}, free_mask, 0, stream};
    const char* fn = "scat_mano_fit_seq_verts";
    int levels = 0;
    int rc = seq_verts_check(fn, c, &levels);
    if (rc == SCAT_OK) rc = seq_verts_launch(fn, c, levels);
    if (rc != SCAT_OK) return rc;
    set_kernel_label(normals ? "mano_fit_seq_verts_metric_v%d_t%d_i%d" : "mano_fit_seq_verts_v%d_t%d_i%d", V, T, iters);
    return SCAT_OK;
}
