// The MANO fit to a track of multi-view keypoints, include_ext/scat_mano_fit_seq_views.h: mano_fit_views.hip's problem
// (2-D keypoints through C calibrated pinhole cameras, Geman-McClure weights, joint limits; scat_mano_fit's 62 unknowns)
// over the T frames of one sequence, coupled and solved as mano_fit_seq.hip couples and solves its own.  One workgroup of
// 256 threads per sequence walks the frames in order, all iterations in one launch.  With init = 1 a launch before it
// computes every frame's own triangulated start, one workgroup per frame (mano_fit_seq_views_start.hip: a second
// translation unit for the reason mano_fit_seq_kp.hip records).
//
// What a frame is comes from mano_fit_views_common.h, one copy shared with mano_fit_views.hip: the per-joint metric M_j,
// h_j and the robust terms (views_residual, not inlined), the plane MG = blockdiag(M_j) J (views_form_mg), the
// behind-the-camera flag (views_behind), the frame's cost (views_cost) and the usable-inputs scan.  What a track is comes
// from mano_fit_seq_common.h at 62 unknowns.  This kernel is that walk with that frame inside:
//   forward    stage the frame's keypoints and weights (the cameras are staged once per sequence), J, M_j and h_j, MG,
//              A_t = J^T MG and g_t = J^T h with the priors, the limits and the smoothness; seq_eliminate
//   backward   seq_backward: x_t = L_t^-T (y_t - M_t+1^T x_t+1), the trial unknowns to the workspace
//   cost       a third walk evaluates the trial's robust cost; a frame behind a camera rejects the trial
// Inside a launch the workspace of a sequence is touched by its own workgroup only, so __syncthreads() between a write and
// its read is all the ordering there is; the start kernel's writes are ordered before the walk by the stream.
#include "mano_fit_seq_views.h"

namespace scat {

struct SeqViewsLds {
    union {
        float J[kFRows][kFU];   // the frame's Jacobian ...
        float M[kFU][kFU];      // ... and, once A and g are built, M_t^T
    };
    float MG[kFRows][kFU];      // row 3 j + c: row c of M_j times G_j
    float A[kFU + 1][kFU];      // lower triangle: H_t, then L_t; row 62: g_t, then y_t
    float col[kFU + 1];
    float delta[kFU];
    float p[kFU], pt[kFU];      // the frame's current and trial unknowns
    float pp[kFU], pn[kFU];     // the same of the frame before and of the frame after
    float yp[kFU], xn[kFU];     // y_t-1 (forward), x_t+1 (backward)
    float dc[kFU], ds[kFU];     // the smoothness weights in the cost, and in the system (zero for a frozen unknown)
    float cam[kVMaxC][kVCam];   // staged once per sequence
    float tgt[kVMaxC][kKRows2], w[kVMaxC][kFJoints];   // staged per frame
    float lo[kFPose], hi[kFPose];
    float Mj[kFJoints][6];      // M_j: xx, xy, xz, yy, yz, zz
    float h[kFRows];
    float rho[kFJoints];
    int behind[kFJoints];
    float cost, lambda;
    float cd, cs;               // the running data and smoothness sums of the walk in progress
    int acc, bad, fail, fin, cur;
    unsigned char has[kSeqMaxT];   // init = 1: the frame has a triangulated start
};
static_assert(sizeof(JacLds) + sizeof(SeqViewsLds) <= 80 * 1024, "static LDS of mano_fit_seq_views_kernel: two workgroups per CU");

__device__ __forceinline__ float seq_views_weight(const SeqViewsArgs& a, int i) {
    return i < 3 ? a.s_rots : i < 3 + kFPose ? a.s_poses : i < kFModel ? a.s_betas : i < kFU - 1 ? a.s_trans : a.s_scale;
}

// the keypoints and weights of frame t, and from the buffer P the unknowns of frames t - 1, t, t + 1 into pp, q, pn
__device__ __forceinline__ void seq_views_stage(SeqViewsLds& f, const float* tg, const float* wt, int C, const float* P,
                                                float* q, int t, int T) {
    const int tid = threadIdx.x;
    const float* tgt = tg + (int64_t)t * C * kKRows2;
    for (int i = tid; i < C * kKRows2; i += kFThreads) f.tgt[i / kKRows2][i % kKRows2] = tgt[i];
    for (int i = tid; i < C * kFJoints; i += kFThreads)
        f.w[i / kFJoints][i % kFJoints] = wt ? wt[(int64_t)t * C * kFJoints + i] : 1.f;
    seq_stage_unknowns<kFU>(f, P, q, t, T, 128);
}

// grid = S, block = 256
__global__ __launch_bounds__(kFThreads) void mano_fit_seq_views_kernel(SeqViewsArgs a) {
    __shared__ JacLds m;
    __shared__ SeqViewsLds f;
    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x, T = a.T, C = a.C;
    float* const wl = seq_ws_l<kFU>(a.ws, s, T);   // L_t and y_t
    float* const wm = seq_ws_m<kFU>(wl, T);        // M_t^T, t >= 1
    float* const wp = seq_ws_p<kFU>(wm, T);        // the unknowns: two buffers of [T][62]
    const float* const cams = a.cams + s * a.cam_stride;
    const float* const tg = a.targets2 + s * T * C * kKRows2;
    const float* const wt = a.weights2 ? a.weights2 + s * T * C * kFJoints : nullptr;
    float* const pg = a.p + s * T * kFU;
    const int np = T * kFU;
    const uint64_t fm = a.free_mask;

    jac_load_model(m, a.m);
    if (tid < kFJoints) {
        const int v = a.joint_map[tid];
        m.map[tid] = v < 0 ? 0 : (v > kFJoints - 1 ? kFJoints - 1 : v);
    } else if (tid >= 64 && tid < 64 + kFU) {
        const int i = tid - 64;
        const float d = seq_views_weight(a, i);
        f.dc[i] = d;
        f.ds[i] = ((fm >> i) & 1u) ? d : 0.f;
    } else if (tid >= 128 && tid < 128 + kFPose) {
        f.lo[tid - 128] = a.lo ? a.lo[tid - 128] : -INFINITY;
        f.hi[tid - 128] = a.hi ? a.hi[tid - 128] : INFINITY;
    }
    for (int i = tid; i < C * kVCam; i += kFThreads) f.cam[0][i] = cams[i];
    if (tid == 0) {
        f.bad = 0;
        f.acc = 0;
        f.cur = 0;
        f.lambda = a.lambda0;
        f.cost = INFINITY;
    }
    __syncthreads();
    {   // usable inputs: the cameras, and every keypoint and weight of every frame
        int bad = fit_unusable(tg, T * C * kKRows2, wt, T * C * kFJoints);
        bad |= fit_unusable(cams, C * kVCam, nullptr, 0);
        if (bad) f.bad = 1;
    }
    __syncthreads();
    if (f.bad) {   // the same for every thread of the workgroup
        seq_refuse<kFU>(a, s, pg, np, -1);
        return;
    }
    ManoArgs pc = a.m, pt = a.m;
    pc.rots = f.p, pc.poses = f.p + 3, pc.betas = f.p + 3 + kFPose;
    pt.rots = f.pt, pt.poses = f.pt + 3, pt.betas = f.pt + 3 + kFPose;
    if (a.init) {   // the start kernel left every frame's own start in the first buffer, and whether it has one
        if (tid < T) f.has[tid] = *seq_views_flag(a.ws, s, T, tid) != 0.f;
        __syncthreads();
        if (tid == 0) {
            int any = 0;
            for (int t = 0; t < T; ++t) any |= f.has[t];
            if (any) fit_start_scan<kFU>(f.has, wp, T);
            else f.bad = 1;
        }
        __syncthreads();
        if (f.bad) {   // no frame has a start: zeros
            seq_refuse<kFU>(a, s, pg, np, -1);
            return;
        }
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
            seq_views_stage(f, tg, wt, C, P, f.p, t, T);
            __syncthreads();
            [[clang::always_inline]] jac_eval(m, pc, 0, true, expf(f.p[kFU - 1]), &f.J[0][0], kFU);
            views_residual(m, f, a, f.p);
            __syncthreads();
            if (tid == 0) {
                if (views_behind(f)) f.bad = 1;   // only the start can be: a trial behind a camera is never taken
                seq_cost_add<kFU>(f, views_cost(f, a, f.p), f.p, f.pp, t);
            }
            views_form_mg(f);
            __syncthreads();
            if (f.bad) break;   // the same for every thread: cost is +inf and acc 0, as seq_write wants them
            // A_t = J^T MG + priors + active limits + c_t D (lower triangle), g_t as row 62; a frozen unknown is a unit row
            for (int w = tid; w < (kFU + 1) * kFU; w += kFThreads) {
                const int ai = w / kFU, bi = w % kFU;
                const bool fb = (fm >> bi) & 1u;
                if (ai == kFU) {
                    float g = 0.f;
                    for (int row = 0; row < kFRows; ++row) g += f.J[row][bi] * f.h[row];
                    if (bi >= 3 && bi < kFModel) g += (bi < 3 + kFPose ? a.w_pose : a.w_beta) * f.p[bi];
                    if (bi >= 3 && bi < 3 + kFPose) g += a.w_limit * kp_excess(f, f.p, bi - 3);
                    if (t > 0) g += f.ds[bi] * (f.p[bi] - f.pp[bi]);
                    if (t < T - 1) g += f.ds[bi] * (f.p[bi] - f.pn[bi]);
                    f.A[kFU][bi] = fb ? g : 0.f;
                } else if (bi <= ai) {
                    const bool fa = (fm >> ai) & 1u;
                    float sum = 0.f;
                    for (int row = 0; row < kFRows; ++row) sum += f.J[row][ai] * f.MG[row][bi];
                    if (ai == bi) {
                        if (ai >= 3 && ai < kFModel) sum += ai < 3 + kFPose ? a.w_pose : a.w_beta;
                        if (ai >= 3 && ai < 3 + kFPose && kp_excess(f, f.p, ai - 3) != 0.f) sum += a.w_limit;
                        sum += ct * f.ds[ai];
                        sum *= 1.f + f.lambda;   // Marquardt: the full diagonal, smoothness included
                    }
                    f.A[ai][bi] = (fa && fb) ? sum : (ai == bi ? 1.f : 0.f);
                }
            }
            __syncthreads();
            seq_eliminate<kFU>(f, wl, wm, t, T);
        }
        if (f.bad) break;   // a frame of the start is behind a camera: the sequence is not fitted
        if (tid == 0) f.cost = f.cd + f.cs;
        // backward: x_t, and the trial unknowns
        for (int t = T - 1; t >= 0; --t) seq_backward<kFU>(f, wl, wm, P, Q, t, T, tid < kFU && ((fm >> tid) & 1u));
        // the trial's cost
        if (tid == 0) {
            f.cd = 0.f, f.cs = 0.f;
            f.fin = 1;
        }
        for (int t = 0; t < T; ++t) {
            seq_views_stage(f, tg, wt, C, Q, f.pt, t, T);
            __syncthreads();
            [[clang::always_inline]] jac_eval(m, pt, 0, false, 1.f, nullptr, 0);
            views_residual(m, f, a, f.pt);
            __syncthreads();
            if (tid == 0) {
                if (views_behind(f)) f.fail = 1;   // rejected, like a failed pivot
                seq_cost_add<kFU>(f, views_cost(f, a, f.pt), f.pt, f.pp, t);
                int fin = f.fin;   // written out in every track kernel: DESIGN.md 18 has what lifting it did
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

extern "C" int64_t scat_mano_fit_seq_views_ws(int S, int T) {
    return seq_ws_bytes<kFU>(S, T);
}

extern "C" int scat_mano_fit_seq_views(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                       const float* hands_mean, const float* cams, int cam_batch, const float* targets2,
                                       const float* weights2, const int* joint_map, const float* pose_lo, const float* pose_hi,
                                       float* p, float* cost, int* accepted, void* ws, int64_t ws_bytes, int S, int T, int C,
                                       int V, uint64_t parents, int tip0, int tip1, int tip2, int tip3, int tip4, int iters,
                                       int init, float lambda0, float w_pose, float w_beta, float w_limit, float sigma2,
                                       float z_near, float s_rots, float s_poses, float s_betas, float s_trans, float s_scale,
                                       uint64_t free_mask, void* stream) {
    const char* fn = "scat_mano_fit_seq_views";
    const void* ptrs[] = {blend, joint_t, joint_s, weights_t, hands_mean, cams, targets2, joint_map, p, cost, accepted};
    const int tips[kMTips] = {tip0, tip1, tip2, tip3, tip4};
    SeqViewsArgs a = {fit_model_args(blend, joint_t, joint_s, weights_t, hands_mean, V, parents, tips),
                      cams, targets2, weights2, joint_map, pose_lo, pose_hi, p, cost, accepted, (float*)ws, T, C,
                      cam_batch == 1 ? 0 : C * kVCam, iters, init, lambda0, w_pose, w_beta, w_limit, sigma2, z_near,
                      s_rots, s_poses, s_betas, s_trans, s_scale, free_mask};
    int rc = mano_validate(fn, ptrs, 11, S, V, parents, tips, &a.m.levels);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE((((uintptr_t)pose_lo | (uintptr_t)pose_hi) & 3) == 0, SCAT_E_ARG, "%s: fp32 operands must be 4-byte aligned", fn);
    SCAT_REQUIRE(!pose_lo == !pose_hi, SCAT_E_ARG, "%s: pose_lo and pose_hi must both be given or both be null", fn);
    rc = views_check(fn, weights2, cam_batch, S, C, z_near);
    if (rc != SCAT_OK) return rc;
    rc = seq_check_frames(fn, T);
    if (rc != SCAT_OK) return rc;
    rc = fit_check_solver(fn, "triangulation, then Procrustes, frame by frame", iters, init, lambda0, w_pose, w_beta);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE(!(init == 1 && C == 1), SCAT_E_ARG, "%s: init 1 needs C >= 2 views: nothing can be triangulated from one", fn);
    SCAT_REQUIRE(kp_weight_ok(w_limit), SCAT_E_ARG, "%s: w_limit %g must be finite and not negative", fn, (double)w_limit);
    SCAT_REQUIRE(kp_weight_ok(sigma2), SCAT_E_ARG, "%s: sigma2 %g must be finite and not negative", fn, (double)sigma2);
    const float sw[5] = {s_rots, s_poses, s_betas, s_trans, s_scale};
    const char* const sn[5] = {"s_rots", "s_poses", "s_betas", "s_trans", "s_scale"};
    rc = seq_check_smooth(fn, sw, sn, 5);
    if (rc != SCAT_OK) return rc;
    rc = fit_check_mask(fn, free_mask);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE((int64_t)S * T <= INT32_MAX, SCAT_E_SHAPE, "%s: %d sequences of %d frames: more than %d frames", fn, S, T, INT32_MAX);
    rc = seq_check_ws(fn, ws, ws_bytes, scat_mano_fit_seq_views_ws(S, T));
    if (rc != SCAT_OK) return rc;
    if (init) {
        seq_views_launch_start(a, S, (hipStream_t)stream);
        SCAT_LAUNCH_CHECK(fn);
    }
    hipLaunchKernelGGL(mano_fit_seq_views_kernel, dim3(S), dim3(kFThreads), 0, (hipStream_t)stream, a);
    SCAT_LAUNCH_CHECK(fn);
    set_kernel_label("mano_fit_seq_views_t%d_c%d_i%d", T, C, iters);
    return SCAT_OK;
}
