// The MANO fit to a track of frames, include/scat_mano_fit_seq.h: mano_fit.hip's problem over T frames of one sequence,
// coupled by a quadratic penalty on consecutive unknowns, as one Levenberg-Marquardt.  One workgroup of 256 threads per
// sequence walks the frames in order, all iterations in one launch.  The frame's residuals and cost (fit_residual,
// fit_cost), the usable-inputs scan (fit_unusable) and the scan over the frames' starts (fit_start_scan) are
// mano_fit_common.h's.  What a track is (the workspace, the block-tridiagonal elimination forward and backward, the
// smoothness sum, the accept step, the refusal and the write-out) is mano_fit_seq_common.h's, shared with
// mano_fit_seq_kp.hip; here it runs at 62 unknowns.  This file keeps the frame: staging of targets and weights, the
// Procrustes start, and the loop that assembles A_t and g_t.  Three passes per iteration:
//   forward    per frame, J, A_t and g_t in LDS by mano_fit.hip's walk, with the smoothness on the diagonal and in g;
//              seq_eliminate: H_t -= M_t M_t^T, g_t -= M_t y_t-1, lm_factor, M_t+1^T = -L_t^-1 D
//   backward   seq_backward: x_t = L_t^-T (y_t - M_t+1^T x_t+1) by lm_backsub, the trial unknowns to the workspace
//   cost       a third walk evaluates the trial's cost
#include "mano_fit_seq_common.h"

namespace scat {

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
    union {
        float J[kFRows][kFU];   // the Jacobian of the frame ...
        float M[kFU][kFU];      // ... and, once A and g are built, M_t^T
    };
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
    unsigned char has[kSeqMaxT];   // init = 1: the frame has weight
};

__device__ __forceinline__ float seq_weight(const SeqArgs& a, int i) {
    return i < 3 ? a.s_rots : i < 3 + kFPose ? a.s_poses : i < kFModel ? a.s_betas : i < kFU - 1 ? a.s_trans : a.s_scale;
}

// the targets and weights of frame t, and from the buffer P the unknowns of frames t - 1, t, t + 1 into pp, q, pn
__device__ __forceinline__ void seq_stage(SeqLds& f, const float* tg, const float* wt, const float* P, float* q, int t, int T) {
    const int tid = threadIdx.x;
    if (tid < kFRows) {   // a joint without weight is staged as zero: its target, however large, never meets a square
        const float w = wt ? wt[(int64_t)t * kFJoints + tid / 3] : 1.f;
        f.tgt[tid] = w == 0.f ? 0.f : tg[(int64_t)t * kFRows + tid];
    } else if (tid >= 64 && tid < 64 + kFJoints) {
        f.w[tid - 64] = wt ? wt[(int64_t)t * kFJoints + (tid - 64)] : 1.f;
    }
    seq_stage_unknowns<kFU>(f, P, q, t, T, 128);
}

// grid = S, block = 256
__global__ __launch_bounds__(kFThreads) void mano_fit_seq_kernel(SeqArgs a) {
    __shared__ JacLds m;
    __shared__ SeqLds f;
    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x, T = a.T;
    float* const wl = seq_ws_l<kFU>(a.ws, s, T);   // L_t and y_t
    float* const wm = seq_ws_m<kFU>(wl, T);        // M_t^T, t >= 1
    float* const wp = seq_ws_p<kFU>(wm, T);        // the unknowns: two buffers of [T][62]
    const float* const tg = a.targets + s * T * kFRows;
    const float* const wt = a.weights ? a.weights + s * T * kFJoints : nullptr;
    float* const pg = a.p + s * T * kFU;
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
        seq_refuse<kFU>(a, s, pg, np, -1);
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
            if (tid == 0) seq_cost_add<kFU>(f, fit_cost(f, f.p, a.w_pose, a.w_beta), f.p, f.pp, t);
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
            seq_eliminate<kFU>(f, wl, wm, t, T);
        }
        if (tid == 0) f.cost = f.cd + f.cs;
        // backward: x_t, and the trial unknowns
        for (int t = T - 1; t >= 0; --t) seq_backward<kFU>(f, wl, wm, P, Q, t, T, tid < kFU && ((fm >> tid) & 1u));
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
                seq_cost_add<kFU>(f, fit_cost(f, f.pt, a.w_pose, a.w_beta), f.pt, f.pp, t);
                int fin = f.fin;   // written out in both kernels: DESIGN.md 18 has what lifting it did
                for (int i = 0; i < kFU; ++i) fin &= fit_finite(f.pt[i]);
                f.fin = fin;
            }
            __syncthreads();
        }
        if (tid == 0) seq_decide(f);
    }
    __syncthreads();
    seq_write(f, a, s, wp, pg, np);
}

}  // namespace scat

using namespace scat;

extern "C" int64_t scat_mano_fit_seq_ws(int S, int T) {
    return seq_ws_bytes<kFU>(S, T);
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
    rc = seq_check_frames(fn, T);
    if (rc != SCAT_OK) return rc;
    rc = fit_check_solver(fn, "Procrustes, frame by frame", iters, init, lambda0, w_pose, w_beta);
    if (rc != SCAT_OK) return rc;
    const float sw[5] = {s_rots, s_poses, s_betas, s_trans, s_scale};
    const char* const sn[5] = {"s_rots", "s_poses", "s_betas", "s_trans", "s_scale"};
    rc = seq_check_smooth(fn, sw, sn, 5);
    if (rc != SCAT_OK) return rc;
    rc = fit_check_mask(fn, free_mask);
    if (rc != SCAT_OK) return rc;
    rc = seq_check_ws(fn, ws, ws_bytes, scat_mano_fit_seq_ws(S, T));
    if (rc != SCAT_OK) return rc;
    hipLaunchKernelGGL(mano_fit_seq_kernel, dim3(S), dim3(kFThreads), 0, (hipStream_t)stream, a);
    SCAT_LAUNCH_CHECK(fn);
    set_kernel_label("mano_fit_seq_v%d_t%d_i%d", V, T, iters);
    return SCAT_OK;
}
