// The MANO fit to keypoints seen by C calibrated pinhole cameras, include_ext/scat_mano_fit_views.h: mano_fit_kernel's
// Levenberg-Marquardt on scat_mano_fit's 62 unknowns with a perspective reprojection term per view, Geman-McClure
// weights (IRLS) and joint limits, and the triangulation that makes its start.  One workgroup of 256 threads per hand,
// all iterations in one launch, everything in LDS; jac_eval, the Procrustes start and the solver's steps (lm_solve,
// lm_accept, lm_commit, lm_write) are mano_fit_common.h's, kp_robust and kp_excess mano_fit_kp_common.h's.  What a views
// frame is (views_triangulate, views_start, views_unusable, views_residual, views_behind, views_cost, views_form_mg) is
// mano_fit_views_common.h's, one copy shared with the track kernel mano_fit_seq_views.hip.
//
// The 42 C rows are not stored.  A view-joint's two rows are P G_j with P = D R_c (2 x 3) and G_j rows 3 j .. 3 j + 2 of
// the stored 63 x 62 Jacobian, so one thread per joint sums its views into M_j = sum_c wi P^T P and h_j = sum_c wi P^T r
// (views_residual), all threads form the plane MG = blockdiag(M_j) J once, and the walk over the normal equations is
// mano_fit_kernel's with MG in the place of W J: A = J^T MG, g = J^T h.  Neither the walk nor LDS grow with C.  Every sum
// is a sequential loop: views ascending inside a joint, joints ascending, then the priors, then the limits.
#include "mano_fit_views_common.h"

namespace scat {

struct ViewsArgs {
    ManoArgs m;   // rots / poses / betas are set by the kernel (LDS)
    const float* cams;
    const float *targets2, *weights2;
    const int* joint_map;
    const float *lo, *hi;
    float* p;
    float* cost;
    int* accepted;
    int C, cam_stride, iters, init;   // cam_stride: C * 16 floats with a rig per sample, 0 with one for the batch
    float lambda0, w_pose, w_beta, w_limit, sigma2, z_near;
    uint64_t free_mask;
};

struct ViewsLds {
    float J[kFRows][kFU];      // scat_mano_fit's
    float MG[kFRows][kFU];     // row 3 j + c: row c of M_j times G_j
    float A[kFU + 1][kFU];     // lower triangle: the damped normal matrix, then its factor; row 62: g, then L^-1 g
    float col[kFU + 1];
    float delta[kFU];
    float p[kFU], pt[kFU];
    float cam[kVMaxC][kVCam];
    float tgt[kVMaxC][kKRows2], w[kVMaxC][kFJoints];
    float lo[kFPose], hi[kFPose];
    float Mj[kFJoints][6];     // M_j: xx, xy, xz, yy, yz, zz
    float h[kFRows];           // h_j; before the iterations the triangulated joints
    float rho[kFJoints];       // sum_c w rho(e) of a joint; before the iterations 1 for a triangulated joint, else 0
    int behind[kFJoints];      // a view of positive weight has the joint at q.z <= z_near
    float cost, lambda;
    int acc, bad, fail, take;
};

// grid = B, block = 256
__global__ __launch_bounds__(kFThreads) void mano_fit_views_kernel(ViewsArgs a) {
    __shared__ JacLds m;
    __shared__ ViewsLds f;
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, C = a.C;
    jac_load_model(m, a.m);
    const float* cams = a.cams + b * a.cam_stride;
    const float* tgt = a.targets2 + b * C * kKRows2;
    const float* wts = a.weights2 ? a.weights2 + b * C * kFJoints : nullptr;
    if (tid < kFJoints) {
        const int v = a.joint_map[tid];
        m.map[tid] = v < 0 ? 0 : (v > kFJoints - 1 ? kFJoints - 1 : v);
    } else if (tid >= 64 && tid < 64 + kFU) {
        f.p[tid - 64] = a.init ? 0.f : a.p[b * kFU + (tid - 64)];
    } else if (tid >= 128 && tid < 128 + kFPose) {
        f.lo[tid - 128] = a.lo ? a.lo[tid - 128] : -INFINITY;
        f.hi[tid - 128] = a.hi ? a.hi[tid - 128] : INFINITY;
    }
    for (int i = tid; i < C * kVCam; i += kFThreads) f.cam[0][i] = cams[i];
    for (int i = tid; i < C * kKRows2; i += kFThreads) f.tgt[i / kKRows2][i % kKRows2] = tgt[i];
    for (int i = tid; i < C * kFJoints; i += kFThreads) f.w[i / kFJoints][i % kFJoints] = wts ? wts[i] : 1.f;
    if (tid == 0) {
        f.acc = 0;
        f.lambda = a.lambda0;
        f.cost = INFINITY;
    }
    if (__syncthreads_or(views_unusable(cams, tgt, wts, C, kFThreads))) {   // acc and cost are as lm_write wants them
        lm_write<kFU>(f, a, b);
        return;
    }
    ManoArgs pc = a.m, pt = a.m;
    pc.rots = f.p, pc.poses = f.p + 3, pc.betas = f.p + 3 + kFPose;
    pt.rots = f.pt, pt.poses = f.pt + 3, pt.betas = f.pt + 3 + kFPose;
    if (a.init) {
        jac_eval(m, pc, 0, false, 1.f, nullptr, 0);   // the zero pose
        views_start(m, f, C, a.z_near, f.p, &f.bad);
        if (f.bad) {   // too few joints triangulated: p is zeros
            lm_write<kFU>(f, a, b);
            return;
        }
    }
    const uint64_t fm = a.free_mask;
    for (int it = 0; it < a.iters; ++it) {
        jac_eval(m, pc, 0, true, expf(f.p[kFU - 1]), &f.J[0][0], kFU);
        views_residual(m, f, a, f.p);
        __syncthreads();
        if (tid == 0) {
            f.bad = views_behind(f);   // only the start can be: a trial behind a camera is never taken
            if (!f.bad) f.cost = views_cost(f, a, f.p);
            f.fail = 0;
        }
        views_form_mg(f);
        __syncthreads();
        if (f.bad) break;   // the same for every thread: cost is +inf and acc 0, as lm_write wants them
        // A = J^T MG + priors + active limits (lower triangle), g = J^T h + their gradients as row 62; a frozen unknown
        // is a unit row
        for (int w = tid; w < (kFU + 1) * kFU; w += kFThreads) {
            const int ai = w / kFU, bi = w % kFU;
            const bool fb = (fm >> bi) & 1u;
            if (ai == kFU) {
                float g = 0.f;
                for (int row = 0; row < kFRows; ++row) g += f.J[row][bi] * f.h[row];
                if (bi >= 3 && bi < kFModel) g += (bi < 3 + kFPose ? a.w_pose : a.w_beta) * f.p[bi];
                if (bi >= 3 && bi < 3 + kFPose) g += a.w_limit * kp_excess(f, f.p, bi - 3);
                f.A[kFU][bi] = fb ? g : 0.f;
            } else if (bi <= ai) {
                const bool fa = (fm >> ai) & 1u;
                float s = 0.f;
                for (int row = 0; row < kFRows; ++row) s += f.J[row][ai] * f.MG[row][bi];
                if (ai == bi) {
                    if (ai >= 3 && ai < kFModel) s += ai < 3 + kFPose ? a.w_pose : a.w_beta;
                    if (ai >= 3 && ai < 3 + kFPose && kp_excess(f, f.p, ai - 3) != 0.f) s += a.w_limit;
                    s *= 1.f + f.lambda;   // Marquardt: A + lambda diag(A)
                }
                f.A[ai][bi] = (fa && fb) ? s : (ai == bi ? 1.f : 0.f);
            }
        }
        __syncthreads();
        lm_solve<kFU>(f);
        if (tid < kFU) f.pt[tid] = ((fm >> tid) & 1u) ? f.p[tid] + f.delta[tid] : f.p[tid];
        jac_eval(m, pt, 0, false, 1.f, nullptr, 0);
        views_residual(m, f, a, f.pt);
        __syncthreads();
        if (tid == 0) {
            const int behind = views_behind(f);
            if (behind) f.fail = 1;   // rejected, like a failed factorisation
            lm_accept<kFU>(f, behind ? INFINITY : views_cost(f, a, f.pt));
        }
        lm_commit<kFU>(f);
    }
    lm_write<kFU>(f, a, b);
}

// grid = B, block = 64
__global__ __launch_bounds__(64) void triangulate_kernel(const float* __restrict__ cams, int cam_stride,
                                                         const float* __restrict__ targets2, const float* __restrict__ weights2,
                                                         float* __restrict__ points, int* __restrict__ valid, int C, float z_near) {
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const float* cam = cams + b * cam_stride;
    const float* tgt = targets2 + b * C * kKRows2;
    const float* wts = weights2 ? weights2 + b * C * kFJoints : nullptr;
    const int bad = __syncthreads_or(views_unusable(cam, tgt, wts, C, 64));
    if (tid >= kFJoints) return;
    double X[3];
    const bool ok = !bad && views_triangulate(cam, tgt + 2 * tid, kKRows2, wts ? wts + tid : nullptr, kFJoints, C, z_near, X);
#pragma unroll
    for (int c = 0; c < 3; ++c) points[b * kFRows + 3 * tid + c] = ok ? (float)X[c] : 0.f;
    valid[b * kFJoints + tid] = ok ? 1 : 0;
}

}  // namespace scat

using namespace scat;

extern "C" int scat_mano_fit_views(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                   const float* hands_mean, const float* cams, int cam_batch, const float* targets2,
                                   const float* weights2, const int* joint_map, const float* pose_lo, const float* pose_hi,
                                   float* p, float* cost, int* accepted, int B, int C, int V, uint64_t parents, int tip0,
                                   int tip1, int tip2, int tip3, int tip4, int iters, int init, float lambda0, float w_pose,
                                   float w_beta, float w_limit, float sigma2, float z_near, uint64_t free_mask, void* stream) {
    const char* fn = "scat_mano_fit_views";
    const void* ptrs[] = {blend, joint_t, joint_s, weights_t, hands_mean, cams, targets2, joint_map, p, cost, accepted};
    const int tips[kMTips] = {tip0, tip1, tip2, tip3, tip4};
    ViewsArgs a = {fit_model_args(blend, joint_t, joint_s, weights_t, hands_mean, V, parents, tips),
                   cams, targets2, weights2, joint_map, pose_lo, pose_hi, p, cost, accepted, C,
                   cam_batch == 1 ? 0 : C * kVCam, iters, init, lambda0, w_pose, w_beta, w_limit, sigma2, z_near, free_mask};
    int rc = mano_validate(fn, ptrs, 11, B, V, parents, tips, &a.m.levels);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE((((uintptr_t)pose_lo | (uintptr_t)pose_hi) & 3) == 0, SCAT_E_ARG, "%s: fp32 operands must be 4-byte aligned", fn);
    SCAT_REQUIRE(!pose_lo == !pose_hi, SCAT_E_ARG, "%s: pose_lo and pose_hi must both be given or both be null", fn);
    rc = views_check(fn, weights2, cam_batch, B, C, z_near);
    if (rc != SCAT_OK) return rc;
    rc = fit_check_solver(fn, "triangulation, then Procrustes", iters, init, lambda0, w_pose, w_beta);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE(kp_weight_ok(w_limit), SCAT_E_ARG, "%s: w_limit %g must be finite and not negative", fn, (double)w_limit);
    SCAT_REQUIRE(kp_weight_ok(sigma2), SCAT_E_ARG, "%s: sigma2 %g must be finite and not negative", fn, (double)sigma2);
    rc = fit_check_mask(fn, free_mask);
    if (rc != SCAT_OK) return rc;
    hipLaunchKernelGGL(mano_fit_views_kernel, dim3(B), dim3(kFThreads), 0, (hipStream_t)stream, a);
    SCAT_LAUNCH_CHECK(fn);
    set_kernel_label("mano_fit_views_v%d_c%d_i%d", V, C, iters);
    return SCAT_OK;
}

extern "C" int scat_triangulate(const float* cams, int cam_batch, const float* targets2, const float* weights2, float* points,
                                int* valid, int B, int C, float z_near, void* stream) {
    const char* fn = "scat_triangulate";
    const void* ptrs[] = {cams, targets2, points, valid};
    uintptr_t all = 0;
    for (const void* q : ptrs) {
        SCAT_REQUIRE(q, SCAT_E_ARG, "%s: null pointer", fn);
        all |= (uintptr_t)q;
    }
    SCAT_REQUIRE((all & 3) == 0, SCAT_E_ARG, "%s: fp32 operands must be 4-byte aligned", fn);
    SCAT_REQUIRE(B > 0, SCAT_E_SHAPE, "%s: batch %d must be positive", fn, B);
    const int rc = views_check(fn, weights2, cam_batch, B, C, z_near);
    if (rc != SCAT_OK) return rc;
    hipLaunchKernelGGL(triangulate_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, cams, cam_batch == 1 ? 0 : C * kVCam,
                       targets2, weights2, points, valid, C, z_near);
    SCAT_LAUNCH_CHECK(fn);
    set_kernel_label("triangulate_c%d", C);
    return SCAT_OK;
}
