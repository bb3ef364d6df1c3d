// The MANO fit to a track of frames, include/scat_mano_fit_seq.h: mano_fit.hip's problem over T frames of one sequence,
// coupled by a quadratic penalty on consecutive unknowns, as one Levenberg-Marquardt.  One workgroup of 256 threads per
// sequence walks the frames in order, all iterations in one launch.  The frame's residuals and cost (fit_residual,
// fit_cost), the two halves of the solve (lm_factor, lm_backsub), the accept step's decision (lm_decide) and the
// usable-inputs scan (fit_unusable, each thread's share) and the scan over the frames' starts (fit_start_scan) are
// mano_fit_common.h's; the block-tridiagonal elimination is this kernel's.
//
// The damped normal matrix is block-tridiagonal: H_t (62 x 62) on the diagonal, -D beside it.  It is factored exactly,
// frame by frame (the header has the recurrences).  Per frame, J, A_t and g_t are built in LDS by mano_fit.hip's walk,
// with the smoothness on the diagonal and in g.  Then
//   rank update   M_t^T, which the frame before left in the workspace, is read into the LDS that J occupied (J is dead
//                 once A_t and g_t stand); H_t -= M_t M_t^T over the lower triangle with all threads, g_t -= M_t y_t-1
//   factor        lm_factor: the left-looking Cholesky of lm_solve, g riding along as row 62 and ending as y_t
//   M_t+1^T       = -L_t^-1 D: 62 forward substitutions, one thread per column, the column written to and read back from
//                 LDS by its own thread only, so no barrier.  It is lower triangular (L^-1 is), which the rank update
//                 and the backward pass use.
// L_t with y_t and M_t+1^T go to the workspace.  The backward pass reads L_t back, x_t = L_t^-T (y_t - M_t+1^T x_t+1) by
// lm_backsub, and writes the trial unknowns to the workspace; a third walk evaluates the trial's cost.  The current and
// the trial unknowns are two buffers of the workspace that swap roles on an accepted step.  The workspace of a sequence
// is touched by its own workgroup only, so __syncthreads() between a write and its read is all the ordering there is.
#include "mano_fit_common.h"

#include "../../include/scat_mano_fit_seq.h"

namespace scat {

constexpr int kSL = (kFU + 1) * kFU;            // 3906 floats: L_t, y_t as row 62
constexpr int kSM = kFU * kFU;                  // 3844 floats: M_t^T
constexpr int kSFrame = kSL + kSM + 2 * kFU;    // 7874 floats of workspace per frame
constexpr int kSMaxT = SCAT_FIT_SEQ_MAX_T;
static_assert(kSMaxT <= kFThreads, "the start gives every frame a thread");

struct SeqArgs {
    ManoArgs m;   // rots / poses / betas are set by the kernel (LDS)
    const float* targets;
    const float* weights;
    const int* joint_map;
    float* p;
    float* cost;
    int* accepted;
    float* ws;
    int T, iters, init;
    float lambda0, w_pose, w_beta;
    float s_rots, s_poses, s_betas, s_trans, s_scale;
    uint64_t free_mask;
};

struct SeqLds {
    float J[kFRows][kFU];    // the Jacobian of the frame; M_t^T (62 x 62) overlays it once A and g are built
    float A[kFU + 1][kFU];   // lower triangle: H_t, then L_t; row 62: g_t, then y_t
    float col[kFU + 1];
    float delta[kFU];
    float p[kFU], pt[kFU];   // the frame's current and trial unknowns
    float pp[kFU], pn[kFU];  // the same of the frame before and of the frame after
    float yp[kFU], xn[kFU];  // y_t-1 (forward), x_t+1 (backward)
    float dc[kFU], ds[kFU];  // the smoothness weights in the cost, and in the system (zero for a frozen unknown)
    float tgt[kFRows], w[kFJoints], r[kFRows];
    float cost, lambda;
    float cd, cs;            // the running data and smoothness sums of the walk in progress
    int acc, bad, fail, fin, cur;
    unsigned char has[kSMaxT];   // init = 1: the frame has weight
};

__device__ __forceinline__ float seq_weight(const SeqArgs& a, int i) {
    return i < 3 ? a.s_rots : i < 3 + kFPose ? a.s_poses : i < kFModel ? a.s_betas : i < kFU - 1 ? a.s_trans : a.s_scale;
}

// one thread: frame t's terms of the cost onto the running sums, q the frame's unknowns and qp those of the frame before
__device__ __forceinline__ void seq_cost_add(SeqLds& f, const float* q, const float* qp, int t, float w_pose, float w_beta) {
    f.cd += fit_cost(f, q, w_pose, w_beta);
    if (t > 0) {
        float cs = f.cs;
        for (int i = 0; i < kFU; ++i) {
            const float e = q[i] - qp[i];
            cs += f.dc[i] * (e * e);
        }
        f.cs = cs;
    }
}

// the targets and weights of frame t, and from the buffer P the unknowns of frames t - 1, t, t + 1 into pp, q, pn
__device__ __forceinline__ void seq_stage(SeqLds& f, const float* tg, const float* wt, const float* P, float* q, int t, int T) {
    const int tid = threadIdx.x;
    if (tid < kFRows) {   // a joint without weight is staged as zero: its target, however large, never meets a square
        const float w = wt ? wt[(int64_t)t * kFJoints + tid / 3] : 1.f;
        f.tgt[tid] = w == 0.f ? 0.f : tg[(int64_t)t * kFRows + tid];
    } else if (tid >= 64 && tid < 64 + kFJoints) {
        f.w[tid - 64] = wt ? wt[(int64_t)t * kFJoints + (tid - 64)] : 1.f;
    } else if (tid >= 128 && tid < 128 + kFU) {
        const int i = tid - 128;
        q[i] = P[t * kFU + i];
        f.pp[i] = t > 0 ? P[(t - 1) * kFU + i] : 0.f;
        f.pn[i] = t < T - 1 ? P[(t + 1) * kFU + i] : 0.f;
    }
}

// grid = S, block = 256
__global__ __launch_bounds__(kFThreads) void mano_fit_seq_kernel(SeqArgs a) {
    __shared__ JacLds m;
    __shared__ SeqLds f;
    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x, T = a.T;
    float* const wl = a.ws + s * ((int64_t)T * kSFrame);   // L_t and y_t
    float* const wm = wl + (int64_t)T * kSL;               // M_t^T, t >= 1
    float* const wp = wm + (int64_t)T * kSM;               // the unknowns: two buffers of [T][62]
    const float* const tg = a.targets + s * T * kFRows;
    const float* const wt = a.weights ? a.weights + s * T * kFJoints : nullptr;
    float* const pg = a.p + s * T * kFU;
    float(*const M)[kFU] = reinterpret_cast<float(*)[kFU]>(&f.J[0][0]);
    const int np = T * kFU;
    const uint64_t fm = a.free_mask;

    jac_load_model(m, a.m);
    if (tid < kFJoints) {
        const int v = a.joint_map[tid];
        m.map[tid] = v < 0 ? 0 : (v > kFJoints - 1 ? kFJoints - 1 : v);
    } else if (tid >= 64 && tid < 64 + kFU) {
        const int i = tid - 64;
        const float d = seq_weight(a, i);
        f.dc[i] = d;
        f.ds[i] = ((fm >> i) & 1u) ? d : 0.f;
    }
    if (tid == 0) {
        f.bad = 0;
        f.acc = 0;
        f.cur = 0;
        f.lambda = a.lambda0;
        f.cost = INFINITY;
    }
    __syncthreads();
    if (fit_unusable(tg, T * kFRows, wt, T * kFJoints)) f.bad = 1;   // usable inputs: every target and weight of every frame
    __syncthreads();
    if (f.bad) {   // the same for every thread of the workgroup
        if (a.init)
            for (int i = tid; i < np; i += kFThreads) pg[i] = 0.f;
        if (tid == 0) {
            a.cost[s] = INFINITY;
            a.accepted[s] = 0;
        }
        return;
    }
    ManoArgs pc = a.m, pt = a.m;
    pc.rots = f.p, pc.poses = f.p + 3, pc.betas = f.p + 3 + kFPose;
    pt.rots = f.pt, pt.poses = f.pt + 3, pt.betas = f.pt + 3 + kFPose;
    if (a.init) {
        if (tid < kFU) f.p[tid] = 0.f;
        if (tid < kFJoints) f.w[tid] = 1.f;
        jac_eval(m, pc, 0, false, 1.f, nullptr, 0);   // the zero pose, the same for every frame
        if (tid < T) {   // one frame per thread
            float* q = wp + tid * kFU;
            for (int i = 0; i < kFU; ++i) q[i] = 0.f;
            const float* w = wt ? wt + tid * kFJoints : f.w;
            double W = 0.0;
            for (int j = 0; j < kFJoints; ++j) W += w[j];
            f.has[tid] = W > 0.0;
            fit_procrustes(m.x, tg + tid * kFRows, w, q);
        }
        __syncthreads();
        if (tid == 0) fit_start_scan<kFU>(f.has, wp, T);
    } else {
        for (int i = tid; i < np; i += kFThreads) wp[i] = pg[i];
    }
    for (int it = 0; it < a.iters; ++it) {
        __syncthreads();
        const float* P = wp + f.cur * np;        // the current unknowns
        float* Q = wp + (1 - f.cur) * np;        // the trial's
        if (tid == 0) {
            f.cd = 0.f, f.cs = 0.f;
            f.fail = 0;
        }
        // forward: assemble, eliminate the frame before, factor
        for (int t = 0; t < T; ++t) {
            const float ct = (t > 0 ? 1.f : 0.f) + (t < T - 1 ? 1.f : 0.f);
            seq_stage(f, tg, wt, P, f.p, t, T);
            __syncthreads();
            jac_eval(m, pc, 0, true, expf(f.p[kFU - 1]), &f.J[0][0], kFU);
            fit_residual(m, f, f.p, true);
            __syncthreads();
            if (tid == 0) seq_cost_add(f, f.p, f.pp, t, a.w_pose, a.w_beta);
            // A_t = J^T W J + priors + c_t D (lower triangle), g_t as row 62; a frozen unknown is a unit row
            for (int w = tid; w < (kFU + 1) * kFU; w += kFThreads) {
                const int ai = w / kFU, bi = w % kFU;
                const bool fb = (fm >> bi) & 1u;
                if (ai == kFU) {
                    float g = 0.f;
                    for (int row = 0; row < kFRows; ++row) g += f.w[row / 3] * f.J[row][bi] * f.r[row];
                    if (bi >= 3 && bi < kFModel) g += (bi < 3 + kFPose ? a.w_pose : a.w_beta) * f.p[bi];
                    if (t > 0) g += f.ds[bi] * (f.p[bi] - f.pp[bi]);
                    if (t < T - 1) g += f.ds[bi] * (f.p[bi] - f.pn[bi]);
                    f.A[kFU][bi] = fb ? g : 0.f;
                } else if (bi <= ai) {
                    const bool fa = (fm >> ai) & 1u;
                    float sum = 0.f;
                    for (int row = 0; row < kFRows; ++row) sum += f.w[row / 3] * f.J[row][ai] * f.J[row][bi];
                    if (ai == bi) {
                        if (ai >= 3 && ai < kFModel) sum += ai < 3 + kFPose ? a.w_pose : a.w_beta;
                        sum += ct * f.ds[ai];
                        sum *= 1.f + f.lambda;   // Marquardt: the full diagonal, smoothness included
                    }
                    f.A[ai][bi] = (fa && fb) ? sum : (ai == bi ? 1.f : 0.f);
                }
            }
            __syncthreads();
            if (t > 0) {
                const float* mt = wm + (int64_t)t * kSM;
                for (int i = tid; i < kSM; i += kFThreads) (&M[0][0])[i] = mt[i];
                __syncthreads();
                // H_t -= M_t M_t^T and g_t -= M_t y_t-1; M^T[k][i] = 0 for i > k
                for (int w = tid; w < (kFU + 1) * kFU; w += kFThreads) {
                    const int ai = w / kFU, bi = w % kFU;
                    if (ai == kFU) {
                        float sum = 0.f;
                        for (int k = bi; k < kFU; ++k) sum += M[k][bi] * f.yp[k];
                        f.A[kFU][bi] -= sum;
                    } else if (bi <= ai) {
                        float sum = 0.f;
                        for (int k = ai; k < kFU; ++k) sum += M[k][ai] * M[k][bi];
                        f.A[ai][bi] -= sum;
                    }
                }
                __syncthreads();
            }
            lm_factor<kFU>(f);
            {
                float* lt = wl + (int64_t)t * kSL;
                for (int i = tid; i < kSL; i += kFThreads) lt[i] = (&f.A[0][0])[i];
            }
            if (tid < kFU) f.yp[tid] = f.A[kFU][tid];
            if (t < T - 1) {
                if (tid < kFU) {   // column tid of M_t+1^T = -L_t^-1 D
                    const float d = f.ds[tid];
                    for (int k = 0; k < kFU; ++k) {
                        float sum = k == tid ? -d : 0.f;
                        for (int j = 0; j < k; ++j) sum -= f.A[k][j] * M[j][tid];
                        M[k][tid] = sum / f.A[k][k];
                    }
                }
                __syncthreads();
                float* mt = wm + (int64_t)(t + 1) * kSM;
                for (int i = tid; i < kSM; i += kFThreads) mt[i] = (&M[0][0])[i];
            }
            __syncthreads();
        }
        if (tid == 0) f.cost = f.cd + f.cs;
        // backward: x_t, and the trial unknowns
        for (int t = T - 1; t >= 0; --t) {
            const float* lt = wl + (int64_t)t * kSL;
            for (int i = tid; i < kSL; i += kFThreads) (&f.A[0][0])[i] = lt[i];
            if (tid < kFU) f.p[tid] = P[t * kFU + tid];
            __syncthreads();
            if (t < T - 1 && tid < kFU) {
                const float* mt = wm + (int64_t)(t + 1) * kSM + tid * kFU;
                float sum = 0.f;
                for (int i = 0; i <= tid; ++i) sum += mt[i] * f.xn[i];
                f.A[kFU][tid] -= sum;
            }
            __syncthreads();
            lm_backsub<kFU>(f);
            if (tid < kFU) {
                f.xn[tid] = -f.delta[tid];
                Q[t * kFU + tid] = ((fm >> tid) & 1u) ? f.p[tid] + f.delta[tid] : f.p[tid];
            }
            __syncthreads();
        }
        // the trial's cost
        if (tid == 0) {
            f.cd = 0.f, f.cs = 0.f;
            f.fin = 1;
        }
        for (int t = 0; t < T; ++t) {
            seq_stage(f, tg, wt, Q, f.pt, t, T);
            __syncthreads();
            jac_eval(m, pt, 0, false, 1.f, nullptr, 0);
            fit_residual(m, f, f.pt, false);
            __syncthreads();
            if (tid == 0) {
                seq_cost_add(f, f.pt, f.pp, t, a.w_pose, a.w_beta);
                int fin = f.fin;
                for (int i = 0; i < kFU; ++i) fin &= fit_finite(f.pt[i]);
                f.fin = fin;
            }
            __syncthreads();
        }
        if (tid == 0) {   // taken if every pivot was positive, every trial unknown is finite and the cost drops
            const float c = f.cd + f.cs;
            const bool ok = !f.fail && f.fin && c < f.cost;
            lm_decide(f, ok, c);
            if (ok) f.cur ^= 1;   // the buffers swap roles, where lm_commit copies pt
        }
    }
    __syncthreads();
    if (a.init || f.acc > 0) {
        const float* P = wp + f.cur * np;
        for (int i = tid; i < np; i += kFThreads) pg[i] = P[i];
    }
    if (tid == 0) {
        a.cost[s] = fit_finite(f.cost) ? f.cost : INFINITY;   // also NaN: a start that is not finite
        a.accepted[s] = f.acc;
    }
}

}  // namespace scat

using namespace scat;

extern "C" int64_t scat_mano_fit_seq_ws(int S, int T) {
    if (S < 1 || T < 1 || T > kSMaxT) return 0;
    return (int64_t)S * T * kSFrame * (int64_t)sizeof(float);
}

extern "C" int scat_mano_fit_seq(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                 const float* hands_mean, const float* targets, const float* weights, const int* joint_map,
                                 float* p, float* cost, int* accepted, void* ws, int64_t ws_bytes, int S, int T, int V,
                                 uint64_t parents, int tip0, int tip1, int tip2, int tip3, int tip4, int iters, int init,
                                 float lambda0, float w_pose, float w_beta, float s_rots, float s_poses, float s_betas,
                                 float s_trans, float s_scale, uint64_t free_mask, void* stream) {
    const char* fn = "scat_mano_fit_seq";
    const void* ptrs[] = {blend, joint_t, joint_s, weights_t, hands_mean, targets, joint_map, p, cost, accepted};
    const int tips[kMTips] = {tip0, tip1, tip2, tip3, tip4};
    SeqArgs a = {fit_model_args(blend, joint_t, joint_s, weights_t, hands_mean, V, parents, tips),
                 targets, weights, joint_map, p, cost, accepted, (float*)ws, T, iters, init, lambda0, w_pose, w_beta,
                 s_rots, s_poses, s_betas, s_trans, s_scale, free_mask};
    int rc = mano_validate(fn, ptrs, 10, S, V, parents, tips, &a.m.levels);
    if (rc != SCAT_OK) return rc;
    rc = fit_check_weights(fn, weights);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE(T >= 1 && T <= kSMaxT, SCAT_E_SHAPE, "%s: %d frames outside 1..%d", fn, T, kSMaxT);
    rc = fit_check_solver(fn, "Procrustes, frame by frame", iters, init, lambda0, w_pose, w_beta);
    if (rc != SCAT_OK) return rc;
    const float sw[5] = {s_rots, s_poses, s_betas, s_trans, s_scale};
    const char* const sn[5] = {"s_rots", "s_poses", "s_betas", "s_trans", "s_scale"};
    for (int i = 0; i < 5; ++i)
        SCAT_REQUIRE(sw[i] >= 0.f && sw[i] < INFINITY, SCAT_E_ARG, "%s: %s %g must be finite and not negative", fn, sn[i],
                     (double)sw[i]);
    rc = fit_check_mask(fn, free_mask);
    if (rc != SCAT_OK) return rc;
    const int64_t need = scat_mano_fit_seq_ws(S, T);
    SCAT_REQUIRE(ws && ((uintptr_t)ws & 15) == 0, SCAT_E_WORKSPACE, "%s: the workspace must be a 16-byte-aligned pointer", fn);
    SCAT_REQUIRE(ws_bytes >= need, SCAT_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn, (long long)ws_bytes,
                 (long long)need);
    hipLaunchKernelGGL(mano_fit_seq_kernel, dim3(S), dim3(kFThreads), 0, (hipStream_t)stream, a);
    SCAT_LAUNCH_CHECK(fn);
    set_kernel_label("mano_fit_seq_v%d_t%d_i%d", V, T, iters);
    return SCAT_OK;
}
