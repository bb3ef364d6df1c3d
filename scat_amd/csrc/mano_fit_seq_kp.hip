// The MANO fit to a track of keypoints, include/scat_mano_fit_seq_kp.h: mano_fit_kp.hip's problem (3-D joints, 2-D
// keypoints through a weak-perspective camera, Geman-McClure weights, joint limits; 65 unknowns) over the T frames of one
// sequence, coupled and solved as mano_fit_seq.hip couples and solves its own.  One workgroup of 256 threads per sequence
// walks the frames in order, all iterations in one launch.  With init = 1 a launch before it computes every frame's own
// closed-form start, one workgroup per frame (mano_fit_seq_kp_start.hip).  REGISTERS: this kernel is at the edge of the
// register file (256 VGPRs and 198 AGPRs, no scratch), and hipcc's inliner decides on which side: with the fp64 start
// inside the walk it spilled 26 VGPRs (208 bytes of scratch per lane); with the start kernel in this translation unit,
// 307 (816 bytes); with jac_eval left to the inliner's own choice one call stayed out of line and ManoArgs went to the
// stack (112 bytes).  Hence the second file and the two [[clang::always_inline]] calls below.
//
// What a frame is comes from mano_fit_kp_common.h: residuals and IRLS weights (kp_residual), the sums over the 105 rows
// from the stored 63 x 62 Jacobian (kp_gram, kp_grad; the 42 2-D rows are never stored), the limits (kp_excess), the
// frame's cost (kp_cost) and the closed-form start (kp_start).  What a track is comes from mano_fit_seq_common.h, shared
// with mano_fit_seq.hip (the workspace's layout, the elimination forward and backward, the smoothness sum, the accept step
// with the buffer swap, the refusal and the write-out), on mano_fit_common.h's lm_factor, lm_backsub, lm_decide,
// fit_unusable and fit_start_scan.  This kernel is that walk at 65 unknowns with that frame inside:
//   forward    stage the frame, J and the residuals, A_t and g_t with the smoothness on the diagonal and in g;
//              seq_eliminate: H_t -= M_t M_t^T, g_t -= M_t y_t-1; lm_factor; M_t+1^T = -L_t^-1 D
//   backward   seq_backward: x_t = L_t^-T (y_t - M_t+1^T x_t+1) by lm_backsub, the trial unknowns to the workspace
//   cost       a third walk evaluates the trial's robust cost
// Inside a launch the workspace of a sequence is touched by its own workgroup only, so __syncthreads() between a write and
// its read is all the ordering there is; the start kernel's writes are ordered before the walk by the stream.
#include "mano_fit_seq_kp.h"

namespace scat {

struct SeqKpLds {
    union {
        float J[kFRows][kFU];   // the 3-D rows of the frame's Jacobian ...
        float M[kKU][kKU];      // ... and, once A and g are built, M_t^T
    };
    float A[kKU + 1][kKU];      // lower triangle: H_t, then L_t; row 65: g_t, then y_t
    float col[kKU + 1];
    float delta[kKU];
    float p[kKU], pt[kKU];      // the frame's current and trial unknowns
    float pp[kKU], pn[kKU];     // the same of the frame before and of the frame after
    float yp[kKU], xn[kKU];     // y_t-1 (forward), x_t+1 (backward)
    float dc[kKU], ds[kKU];     // the smoothness weights in the cost, and in the system (zero for a frozen unknown)
    float tgt3[kFRows], tgt2[kKRows2], w3[kFJoints], w2[kFJoints];
    float lo[kFPose], hi[kFPose];
    float r[kKRows], wrow[kKRows], wr[kKRows];   // mano_fit_kp.hip's: residuals, IRLS row weights, their product
    float rho[2 * kFJoints];
    float dcs[kKRows2];
    float k2[2];
    float cost, lambda;
    float cd, cs;               // the running data and smoothness sums of the walk in progress
    int acc, bad, fail, fin, cur;
    unsigned char has[kSeqMaxT];  // init = 1: the frame has weight
};
static_assert(sizeof(JacLds) + sizeof(SeqKpLds) <= 64 * 1024, "static LDS of mano_fit_seq_kp_kernel must stay under 64 KiB");

__device__ __forceinline__ float seq_kp_weight(const SeqKpArgs& a, int i) {
    return i < 3 ? a.s_rots : i < 3 + kFPose ? a.s_poses : i < kFModel ? a.s_betas : i < kFU - 1 ? a.s_trans
         : i < kFU ? a.s_scale : i == kKCam ? a.s_cs : a.s_ct;
}

// the targets and weights of frame t (an absent term: zeros; a joint without weight is staged with a zero target), and
// from the buffer P the unknowns of frames t - 1, t, t + 1 into pp, q, pn
__device__ __forceinline__ void seq_kp_stage(SeqKpLds& f, const float* tg3, const float* wt3, const float* tg2, const float* wt2,
                                             const float* P, float* q, int t, int T) {
    const int tid = threadIdx.x;
    if (tid < kFRows) {
        const float w = tg3 ? (wt3 ? wt3[(int64_t)t * kFJoints + tid / 3] : 1.f) : 0.f;
        f.tgt3[tid] = w == 0.f ? 0.f : tg3[(int64_t)t * kFRows + tid];
    } else if (tid >= 64 && tid < 64 + kFJoints) {
        const int j = tid - 64;
        f.w3[j] = tg3 ? (wt3 ? wt3[(int64_t)t * kFJoints + j] : 1.f) : 0.f;
        f.w2[j] = tg2 ? (wt2 ? wt2[(int64_t)t * kFJoints + j] : 1.f) : 0.f;
    } else if (tid >= 96 && tid < 96 + kKRows2) {
        const int i = tid - 96;
        const float w = tg2 ? (wt2 ? wt2[(int64_t)t * kFJoints + i / 2] : 1.f) : 0.f;
        f.tgt2[i] = w == 0.f ? 0.f : tg2[(int64_t)t * kKRows2 + i];
    }
    seq_stage_unknowns<kKU>(f, P, q, t, T, 160);
}

// the frame has weight: sum w3 + sum w2 > 0, a null weights pointer of a present term being all ones
__device__ __forceinline__ bool seq_kp_has(const float* wt3, const float* wt2, bool has3, bool has2, int t) {
    float W = 0.f;
    if (has3)
        for (int j = 0; j < kFJoints; ++j) W += wt3 ? wt3[(int64_t)t * kFJoints + j] : 1.f;
    if (has2)
        for (int j = 0; j < kFJoints; ++j) W += wt2 ? wt2[(int64_t)t * kFJoints + j] : 1.f;
    return W > 0.f;
}

// grid = S, block = 256
__global__ __launch_bounds__(kFThreads) void mano_fit_seq_kp_kernel(SeqKpArgs a) {
    __shared__ JacLds m;
    __shared__ SeqKpLds f;
    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x, T = a.T;
    const bool has3 = a.targets3 != nullptr, has2 = a.targets2 != nullptr;
    float* const wl = seq_ws_l<kKU>(a.ws, s, T);   // L_t and y_t
    float* const wm = seq_ws_m<kKU>(wl, T);        // M_t^T, t >= 1
    float* const wp = seq_ws_p<kKU>(wm, T);        // the unknowns: two buffers of [T][65]
    const float* const tg3 = has3 ? a.targets3 + s * T * kFRows : nullptr;
    const float* const wt3 = a.weights3 ? a.weights3 + s * T * kFJoints : nullptr;
    const float* const tg2 = has2 ? a.targets2 + s * T * kKRows2 : nullptr;
    const float* const wt2 = a.weights2 ? a.weights2 + s * T * kFJoints : nullptr;
    float* const pg = a.p + s * T * kKU;
    const int np = T * kKU;

    jac_load_model(m, a.m);
    if (tid < kFJoints) {
        const int v = a.joint_map[tid];
        m.map[tid] = v < 0 ? 0 : (v > kFJoints - 1 ? kFJoints - 1 : v);
    } else if (tid >= 64 && tid < 64 + kKU) {
        const int i = tid - 64;
        const float d = seq_kp_weight(a, i);
        f.dc[i] = d;
        f.ds[i] = kp_free(a, i) ? d : 0.f;
    } else if (tid >= 160 && tid < 160 + kFPose) {
        const int i = tid - 160;
        f.lo[i] = a.lo ? a.lo[i] : -INFINITY;
        f.hi[i] = a.hi ? a.hi[i] : INFINITY;
    }
    if (tid == 0) {
        f.bad = 0;
        f.acc = 0;
        f.cur = 0;
        f.lambda = a.lambda0;
        f.cost = INFINITY;
    }
    __syncthreads();
    {   // usable inputs: every target and weight of every frame of the terms that are present
        int bad = has3 ? fit_unusable(tg3, T * kFRows, wt3, T * kFJoints) : 0;
        if (has2) bad |= fit_unusable(tg2, T * kKRows2, wt2, T * kFJoints);
        if (bad) f.bad = 1;
    }
    __syncthreads();
    if (f.bad) {   // the same for every thread of the workgroup
        seq_refuse<kKU>(a, s, pg, np, kKCam);   // the camera (1, 0, 0)
        return;
    }
    ManoArgs pc = a.m, pt = a.m;
    pc.rots = f.p, pc.poses = f.p + 3, pc.betas = f.p + 3 + kFPose;
    pt.rots = f.pt, pt.poses = f.pt + 3, pt.betas = f.pt + 3 + kFPose;
    if (a.init) {   // the start kernel left every frame's own start in the first buffer
        if (tid < T) f.has[tid] = seq_kp_has(wt3, wt2, has3, has2, tid);
        __syncthreads();
        if (tid == 0) fit_start_scan<kKU>(f.has, wp, T);
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
            seq_kp_stage(f, tg3, wt3, tg2, wt2, P, f.p, t, T);
            __syncthreads();
            [[clang::always_inline]] jac_eval(m, pc, 0, true, expf(f.p[kFU - 1]), &f.J[0][0], kFU);
            kp_residual(m, f, a, f.p, true);
            __syncthreads();
            if (tid == 0) seq_cost_add<kKU>(f, kp_cost(f, a, f.p), f.p, f.pp, t);
            // A_t = J^T W J + priors + active limits + c_t D (lower triangle), g_t as row 65; a frozen unknown is a unit row
            for (int w = tid; w < (kKU + 1) * kKU; w += kFThreads) {
                const int ai = w / kKU, bi = w % kKU;
                const bool fb = kp_free(a, bi);
                if (ai == kKU) {
                    float g = kp_grad(f, bi, has3, has2);
                    if (bi >= 3 && bi < kFModel) g += (bi < 3 + kFPose ? a.w_pose : a.w_beta) * f.p[bi];
                    if (bi >= 3 && bi < 3 + kFPose) g += a.w_limit * kp_excess(f, f.p, bi - 3);
                    if (t > 0) g += f.ds[bi] * (f.p[bi] - f.pp[bi]);
                    if (t < T - 1) g += f.ds[bi] * (f.p[bi] - f.pn[bi]);
                    f.A[kKU][bi] = fb ? g : 0.f;
                } else if (bi <= ai) {
                    const bool fa = kp_free(a, ai);
                    float sum = kp_gram(f, ai, bi, has3, has2);
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
            seq_eliminate<kKU>(f, wl, wm, t, T);
        }
        if (tid == 0) f.cost = f.cd + f.cs;
        // backward: x_t, and the trial unknowns
        for (int t = T - 1; t >= 0; --t) seq_backward<kKU>(f, wl, wm, P, Q, t, T, tid < kKU && kp_free(a, tid));
        // the trial's cost
        if (tid == 0) {
            f.cd = 0.f, f.cs = 0.f;
            f.fin = 1;
        }
        for (int t = 0; t < T; ++t) {
            seq_kp_stage(f, tg3, wt3, tg2, wt2, Q, f.pt, t, T);
            __syncthreads();
            [[clang::always_inline]] jac_eval(m, pt, 0, false, 1.f, nullptr, 0);
            kp_residual(m, f, a, f.pt, false);
            __syncthreads();
            if (tid == 0) {
                seq_cost_add<kKU>(f, kp_cost(f, a, f.pt), f.pt, f.pp, t);
                int fin = f.fin;   // written out in both kernels: DESIGN.md 18 has what lifting it did
                for (int i = 0; i < kKU; ++i) fin &= fit_finite(f.pt[i]);
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

extern "C" int64_t scat_mano_fit_seq_kp_ws(int S, int T) {
    return seq_ws_bytes<kKU>(S, T);
}

extern "C" int scat_mano_fit_seq_kp(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                    const float* hands_mean, const float* targets3, const float* weights3,
                                    const float* targets2, const float* weights2, const int* joint_map, const float* pose_lo,
                                    const float* pose_hi, float* p, float* cost, int* accepted, void* ws, int64_t ws_bytes,
                                    int S, int T, int V, uint64_t parents, int tip0, int tip1, int tip2, int tip3, int tip4,
                                    int iters, int init, float lambda0, float w_pose, float w_beta, float w_limit, float sigma3,
                                    float sigma2, float half_w, float half_h, float s_rots, float s_poses, float s_betas,
                                    float s_trans, float s_scale, float s_cs, float s_ct, uint64_t free_mask, int free_cam,
                                    void* stream) {
    const char* fn = "scat_mano_fit_seq_kp";
    const void* ptrs[] = {blend, joint_t, joint_s, weights_t, hands_mean, joint_map, p, cost, accepted};
    const int tips[kMTips] = {tip0, tip1, tip2, tip3, tip4};
    SeqKpArgs a = {fit_model_args(blend, joint_t, joint_s, weights_t, hands_mean, V, parents, tips),
                   targets3, weights3, targets2, weights2, joint_map, pose_lo, pose_hi, p, cost, accepted, (float*)ws, T, iters,
                   init, lambda0, w_pose, w_beta, w_limit, sigma3, sigma2, {half_w, half_h}, s_rots, s_poses, s_betas, s_trans,
                   s_scale, s_cs, s_ct, free_mask, free_cam};
    int rc = mano_validate(fn, ptrs, 9, S, V, parents, tips, &a.m.levels);
    if (rc != SCAT_OK) return rc;
    rc = kp_check_terms(fn, targets3, weights3, targets2, weights2, pose_lo, pose_hi);
    if (rc != SCAT_OK) return rc;
    rc = seq_check_frames(fn, T);
    if (rc != SCAT_OK) return rc;
    rc = fit_check_solver(fn, "the closed-form start, frame by frame", iters, init, lambda0, w_pose, w_beta);
    if (rc != SCAT_OK) return rc;
    rc = kp_check_loss(fn, w_limit, sigma3, sigma2, half_w, half_h);
    if (rc != SCAT_OK) return rc;
    const float sw[7] = {s_rots, s_poses, s_betas, s_trans, s_scale, s_cs, s_ct};
    const char* const sn[7] = {"s_rots", "s_poses", "s_betas", "s_trans", "s_scale", "s_cs", "s_ct"};
    rc = seq_check_smooth(fn, sw, sn, 7);
    if (rc != SCAT_OK) return rc;
    rc = fit_check_mask(fn, free_mask);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE(free_cam >= 0 && free_cam <= 7, SCAT_E_ARG, "%s: free_cam %d outside 0..7", fn, free_cam);
    SCAT_REQUIRE((int64_t)S * T <= INT32_MAX, SCAT_E_SHAPE, "%s: %d sequences of %d frames: more than %d frames", fn, S, T, INT32_MAX);
    rc = seq_check_ws(fn, ws, ws_bytes, scat_mano_fit_seq_kp_ws(S, T));
    if (rc != SCAT_OK) return rc;
    if (init) {
        seq_kp_launch_start(a, S, (hipStream_t)stream);
        SCAT_LAUNCH_CHECK(fn);
    }
    hipLaunchKernelGGL(mano_fit_seq_kp_kernel, dim3(S), dim3(kFThreads), 0, (hipStream_t)stream, a);
    SCAT_LAUNCH_CHECK(fn);
    set_kernel_label("mano_fit_seq_kp_t%d_i%d", T, iters);
    return SCAT_OK;
}
