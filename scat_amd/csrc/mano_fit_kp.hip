// The MANO fit to keypoints, include/scat_mano_fit_kp.h: mano_fit_kernel's Levenberg-Marquardt with a 2-D reprojection
// term through a weak-perspective camera, Geman-McClure weights (IRLS) and joint limits.  One workgroup of 256 threads per
// sample, all iterations in one launch, everything in LDS; jac_eval, the Procrustes start, the constants and the solver's
// steps that do not depend on the problem (lm_solve, lm_accept, lm_commit, lm_write) are mano_fit_common.h's; the row
// algebra, the robust terms, the limits and both closed-form starts are mano_fit_kp_common.h's, shared with
// mano_fit_seq_kp.hip.
//
// 65 unknowns: scat_mano_fit's 62, then cs, ctx, cty.  The 42 rows of the 2-D term are not stored: in the first 62 columns
// row (j, c) of the 2-D term is cs half_c times row 3 j + c of the 3-D Jacobian, and its three camera columns are
// (m_c + ct_c) half_c, and cs half_c on its own offset.  kp_gram() and kp_grad() sum over all 105 rows from the stored
// 63 x 62 Jacobian, so LDS stays at J (63 x 62) and the normal matrix (66 x 65, g as the last row).  Every sum is a
// sequential loop: rows 0..62 (3-D joints ascending), rows 63..104 (2-D joints ascending), then the priors, then the
// limits.
#include "mano_fit_kp_common.h"

namespace scat {

struct KpArgs {
    ManoArgs m;   // rots / poses / betas are set by the kernel (LDS)
    const float *targets3, *weights3, *targets2, *weights2;
    const int* joint_map;
    const float *lo, *hi;
    float* p;
    float* cost;
    int* accepted;
    int iters, init;
    float lambda0, w_pose, w_beta, w_limit, sigma3, sigma2, half[2];
    uint64_t free_mask;
    int free_cam;
};

struct KpLds {
    float J[kFRows][kFU];      // the 3-D rows, scat_mano_fit's
    float A[kKU + 1][kKU];     // lower triangle: the damped normal matrix, then its factor; row 65: g, then L^-1 g
    float col[kKU + 1];
    float delta[kKU];
    float p[kKU], pt[kKU];
    float tgt3[kFRows], tgt2[kKRows2], w3[kFJoints], w2[kFJoints];
    float lo[kFPose], hi[kFPose];
    float r[kKRows];           // residuals: 3-D rows, then 2-D rows
    float wrow[kKRows];        // the IRLS weight of a row: w rho'(e) of its joint
    float wr[kKRows];          // wrow * r, zero for a row of weight zero
    float rho[2 * kFJoints];   // w rho(e): 3-D joints, then 2-D joints
    float dcs[kKRows2];        // d u / d cs = (m_c + ct_c) half_c
    float k2[2];               // cs half_c
    float cost, lambda;
    int acc, bad, fail, take;
};

// grid = B, block = 256
__global__ __launch_bounds__(kFThreads) void mano_fit_kp_kernel(KpArgs a) {
    __shared__ JacLds m;
    __shared__ KpLds f;
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const bool has3 = a.targets3 != nullptr, has2 = a.targets2 != nullptr;
    jac_load_model(m, a.m);
    if (tid < kFJoints) {
        const int v = a.joint_map[tid];
        m.map[tid] = v < 0 ? 0 : (v > kFJoints - 1 ? kFJoints - 1 : v);
        f.w3[tid] = has3 ? (a.weights3 ? a.weights3[b * kFJoints + tid] : 1.f) : 0.f;
        f.w2[tid] = has2 ? (a.weights2 ? a.weights2[b * kFJoints + tid] : 1.f) : 0.f;
    } else if (tid >= 64 && tid < 64 + kFRows) {
        f.tgt3[tid - 64] = has3 ? a.targets3[b * kFRows + (tid - 64)] : 0.f;
    } else if (tid >= 128 && tid < 128 + kKU) {
        const int i = tid - 128;
        f.p[i] = a.init ? (i == kKCam ? 1.f : 0.f) : a.p[b * kKU + i];
    } else if (tid >= 193 && tid < 193 + kKRows2) {
        f.tgt2[tid - 193] = has2 ? a.targets2[b * kKRows2 + (tid - 193)] : 0.f;
    }
    if (tid < kFPose) {
        f.lo[tid] = a.lo ? a.lo[tid] : -INFINITY;
        f.hi[tid] = a.hi ? a.hi[tid] : INFINITY;
    }
    __syncthreads();
    if (tid == 0) {
        int bad = 0;
        for (int i = 0; i < kFRows; ++i) bad |= !fit_finite(f.tgt3[i]);
        for (int i = 0; i < kKRows2; ++i) bad |= !fit_finite(f.tgt2[i]);
        for (int j = 0; j < kFJoints; ++j)
            bad |= !(fit_finite(f.w3[j]) && f.w3[j] >= 0.f) || !(fit_finite(f.w2[j]) && f.w2[j] >= 0.f);
        f.bad = bad;
        f.acc = 0;
        f.lambda = a.lambda0;
        f.cost = INFINITY;
    }
    __syncthreads();
    if (f.bad) {   // the same for every thread of the workgroup; acc and cost are as lm_write wants them
        lm_write<kKU>(f, a, b);
        return;
    }
    ManoArgs pc = a.m, pt = a.m;
    pc.rots = f.p, pc.poses = f.p + 3, pc.betas = f.p + 3 + kFPose;
    pt.rots = f.pt, pt.poses = f.pt + 3, pt.betas = f.pt + 3 + kFPose;
    if (a.init) {
        jac_eval(m, pc, 0, false, 1.f, nullptr, 0);   // the zero pose
        if (tid == 0) {   // kp_start's dispatch, written out: through the call hipcc schedules four places of this kernel differently
            float W3 = 0.f;
            for (int j = 0; j < kFJoints; ++j) W3 += f.w3[j];
            if (W3 > 0.f || !has2) {
                fit_procrustes(m.x, f.tgt3, f.w3, f.p);
                if (has2) kp_camera_start(m.x, f, a, f.p);
            } else {
                kp_start_2d(m.x, f, a, f.p);
            }
        }
        __syncthreads();
    }
    for (int it = 0; it < a.iters; ++it) {
        jac_eval(m, pc, 0, true, expf(f.p[kFU - 1]), &f.J[0][0], kFU);
        kp_residual(m, f, a, f.p, true);
        __syncthreads();
        if (tid == 0) {
            f.cost = kp_cost(f, a, f.p);
            f.fail = 0;
        }
        // A = J^T W J + priors + active limits (lower triangle), g = J^T W r + their gradients as row 65; a frozen unknown
        // is a unit row
        for (int w = tid; w < (kKU + 1) * kKU; w += kFThreads) {
            const int ai = w / kKU, bi = w % kKU;
            const bool fb = kp_free(a, bi);
            if (ai == kKU) {
                float g = kp_grad(f, bi, has3, has2);
                if (bi >= 3 && bi < kFModel) g += (bi < 3 + kFPose ? a.w_pose : a.w_beta) * f.p[bi];
                if (bi >= 3 && bi < 3 + kFPose) g += a.w_limit * kp_excess(f, f.p, bi - 3);
                f.A[kKU][bi] = fb ? g : 0.f;
            } else if (bi <= ai) {
                const bool fa = kp_free(a, ai);
                float s = kp_gram(f, ai, bi, has3, has2);
                if (ai == bi) {
                    if (ai >= 3 && ai < kFModel) s += ai < 3 + kFPose ? a.w_pose : a.w_beta;
                    if (ai >= 3 && ai < 3 + kFPose && kp_excess(f, f.p, ai - 3) != 0.f) s += a.w_limit;
                    s *= 1.f + f.lambda;   // Marquardt: A + lambda diag(A)
                }
                f.A[ai][bi] = (fa && fb) ? s : (ai == bi ? 1.f : 0.f);
            }
        }
        __syncthreads();
        lm_solve<kKU>(f);
        if (tid < kKU) f.pt[tid] = kp_free(a, tid) ? f.p[tid] + f.delta[tid] : f.p[tid];
        jac_eval(m, pt, 0, false, 1.f, nullptr, 0);
        kp_residual(m, f, a, f.pt, false);
        __syncthreads();
        if (tid == 0) lm_accept<kKU>(f, kp_cost(f, a, f.pt));
        lm_commit<kKU>(f);
    }
    lm_write<kKU>(f, a, b);
}

}  // namespace scat

using namespace scat;

extern "C" int scat_mano_fit_kp(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                const float* hands_mean, const float* targets3, const float* weights3, const float* targets2,
                                const float* weights2, const int* joint_map, const float* pose_lo, const float* pose_hi,
                                float* p, float* cost, int* accepted, int B, int V, uint64_t parents, int tip0, int tip1,
                                int tip2, int tip3, int tip4, int iters, int init, float lambda0, float w_pose, float w_beta,
                                float w_limit, float sigma3, float sigma2, float half_w, float half_h, uint64_t free_mask,
                                int free_cam, void* stream) {
    const char* fn = "scat_mano_fit_kp";
    const void* ptrs[] = {blend, joint_t, joint_s, weights_t, hands_mean, joint_map, p, cost, accepted};
    const int tips[kMTips] = {tip0, tip1, tip2, tip3, tip4};
    KpArgs a = {fit_model_args(blend, joint_t, joint_s, weights_t, hands_mean, V, parents, tips),
                targets3, weights3, targets2, weights2, joint_map, pose_lo, pose_hi, p, cost, accepted, iters, init, lambda0,
                w_pose, w_beta, w_limit, sigma3, sigma2, {half_w, half_h}, free_mask, free_cam};
    int rc = mano_validate(fn, ptrs, 9, B, V, parents, tips, &a.m.levels);
    if (rc != SCAT_OK) return rc;
    rc = kp_check_terms(fn, targets3, weights3, targets2, weights2, pose_lo, pose_hi);
    if (rc != SCAT_OK) return rc;
    rc = fit_check_solver(fn, "the closed-form start", iters, init, lambda0, w_pose, w_beta);
    if (rc != SCAT_OK) return rc;
    rc = kp_check_loss(fn, w_limit, sigma3, sigma2, half_w, half_h);
    if (rc != SCAT_OK) return rc;
    rc = fit_check_mask(fn, free_mask);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE(free_cam >= 0 && free_cam <= 7, SCAT_E_ARG, "%s: free_cam %d outside 0..7", fn, free_cam);
    hipLaunchKernelGGL(mano_fit_kp_kernel, dim3(B), dim3(kFThreads), 0, (hipStream_t)stream, a);
    SCAT_LAUNCH_CHECK(fn);
    set_kernel_label("mano_fit_kp_v%d_i%d", V, iters);
    return SCAT_OK;
}
