// The inverse of the MANO layer, include/scat_mano_fit.h: the 21 joints with their analytic Jacobian, and a
// Levenberg-Marquardt fit of pose, shape and a similarity to 21 target joints.  One workgroup of 256 threads per sample.
//
// jac_eval (mano_fit_common.h) is what the joints kernels share.  After mano_setup (mano_common.h) it needs no pass over
// the mesh: the blend rows and skinning weights of the five tip vertices are copied into LDS once per workgroup
// (jac_load_model), a tip is blended and skinned from there in mano_vertex's order, and the Jacobian is forward mode, one
// (joint, column) pair per work-item.  With y_i the un-rotated joints (t_i of the chain, v' of a tip), x_j = Rg (y_j - y_1):
//   rots m        dRg/dr_m (y_j - y_1)
//   pose (k, m)   RG_i = RG_parent(k) R_k (...), so d RG_i = Omega RG_i and d t_i = Omega (t_i - t_k) for i in k's subtree,
//                 Omega = RG_parent(k) dR_k/dr_m RG_k^T; a tip adds T (posedirs_k . dR_k/dr_m) through v_posed
//   beta b        d t_i = d J_0 + sum over the path of RG_parent (dJ_c - dJ_parent), a tip
//                 sum_i w_i (RG_i (shapedirs_b - dJ_i) + d t_i)
// mano_fit_kernel keeps J (63 x 62), the normal matrix with g as its 63rd row, and both parameter vectors in LDS.  The
// residuals and the cost (fit_residual, fit_cost), the factorisation, the back substitution, the accept step and the final
// write (lm_solve, lm_accept, lm_commit, lm_write) are mano_fit_common.h's, described there; the walk that assembles the
// normal equations is the kernel's.  All sums are sequential loops in a fixed order.
#include "mano_fit_common.h"

namespace scat {

// grid = B, block = 256
__global__ __launch_bounds__(kFThreads) void mano_joints_jac_kernel(ManoArgs p, float* __restrict__ joints,
                                                                    float* __restrict__ jac) {
    __shared__ JacLds m;
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    jac_load_model(m, p);
    if (tid < kFJoints) m.map[tid] = tid;
    jac_eval(m, p, b, true, 1.f, jac + b * (int64_t)(kFRows * kFModel), kFModel);
    if (tid < kFRows) joints[b * kFRows + tid] = m.x[tid];
}

struct FitArgs {
    ManoArgs m;   // rots / poses / betas are set by the kernel (LDS)
    const float* targets;
    const float* weights;
    const int* joint_map;
    float* p;
    float* cost;
    int* accepted;
    int iters, init;
    float lambda0, w_pose, w_beta;
    uint64_t free_mask;
};

struct FitLds {
    float J[kFRows][kFU];
    float A[kFU + 1][kFU];   // lower triangle: the damped normal matrix, then its factor; row 62: g, then L^-1 g
    float col[kFU + 1];
    float delta[kFU];
    float p[kFU], pt[kFU];
    float tgt[kFRows], w[kFJoints], r[kFRows];
    float cost, lambda;
    int acc, bad, fail, take;
};

// grid = B, block = 256
__global__ __launch_bounds__(kFThreads) void mano_fit_kernel(FitArgs a) {
    __shared__ JacLds m;
    __shared__ FitLds f;
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    jac_load_model(m, a.m);
    if (tid < kFJoints) {
        const int v = a.joint_map[tid];
        m.map[tid] = v < 0 ? 0 : (v > kFJoints - 1 ? kFJoints - 1 : v);
        f.w[tid] = a.weights ? a.weights[b * kFJoints + tid] : 1.f;
    } else if (tid >= 64 && tid < 64 + kFRows) {
        f.tgt[tid - 64] = a.targets[b * kFRows + (tid - 64)];
    } else if (tid >= 128 && tid < 128 + kFU) {
        f.p[tid - 128] = a.init ? 0.f : a.p[b * kFU + (tid - 128)];
    }
    __syncthreads();
    if (tid == 0) {
        int bad = 0;
        for (int i = 0; i < kFRows; ++i) bad |= !fit_finite(f.tgt[i]);
        for (int j = 0; j < kFJoints; ++j) bad |= !(fit_finite(f.w[j]) && f.w[j] >= 0.f);
        f.bad = bad;
        f.acc = 0;
        f.lambda = a.lambda0;
        f.cost = INFINITY;
    }
    __syncthreads();
    if (f.bad) {   // the same for every thread of the workgroup; acc and cost are as lm_write wants them
        lm_write<kFU>(f, a, b);
        return;
    }
    ManoArgs pc = a.m, pt = a.m;
    pc.rots = f.p, pc.poses = f.p + 3, pc.betas = f.p + 3 + kFPose;
    pt.rots = f.pt, pt.poses = f.pt + 3, pt.betas = f.pt + 3 + kFPose;
    if (a.init) {
        jac_eval(m, pc, 0, false, 1.f, nullptr, 0);   // the zero pose
        if (tid == 0) fit_procrustes(m.x, f.tgt, f.w, f.p);
        __syncthreads();
    }
    const uint64_t fm = a.free_mask;
    for (int it = 0; it < a.iters; ++it) {
        jac_eval(m, pc, 0, true, expf(f.p[kFU - 1]), &f.J[0][0], kFU);
        fit_residual(m, f, f.p, true);
        __syncthreads();
        if (tid == 0) {
            f.cost = fit_cost(f, f.p, a.w_pose, a.w_beta);
            f.fail = 0;
        }
        // A = J^T W J + priors (lower triangle), g = J^T W r + the priors' gradient as row 62; a frozen unknown is a unit row
        for (int w = tid; w < (kFU + 1) * kFU; w += kFThreads) {
            const int ai = w / kFU, bi = w % kFU;
            const bool fb = (fm >> bi) & 1u;
            if (ai == kFU) {
                float g = 0.f;
                for (int row = 0; row < kFRows; ++row) g += f.w[row / 3] * f.J[row][bi] * f.r[row];
                if (bi >= 3 && bi < kFModel) g += (bi < 3 + kFPose ? a.w_pose : a.w_beta) * f.p[bi];
                f.A[kFU][bi] = fb ? g : 0.f;
            } else if (bi <= ai) {
                const bool fa = (fm >> ai) & 1u;
                float s = 0.f;
                for (int row = 0; row < kFRows; ++row) s += f.w[row / 3] * f.J[row][ai] * f.J[row][bi];
                if (ai == bi) {
                    if (ai >= 3 && ai < kFModel) s += ai < 3 + kFPose ? a.w_pose : a.w_beta;
                    s *= 1.f + f.lambda;   // Marquardt: A + lambda diag(A)
                }
                f.A[ai][bi] = (fa && fb) ? s : (ai == bi ? 1.f : 0.f);
            }
        }
        __syncthreads();
        lm_solve<kFU>(f);
        if (tid < kFU) f.pt[tid] = ((fm >> tid) & 1u) ? f.p[tid] + f.delta[tid] : f.p[tid];
        jac_eval(m, pt, 0, false, 1.f, nullptr, 0);
        fit_residual(m, f, f.pt, false);
        __syncthreads();
        if (tid == 0) lm_accept<kFU>(f, fit_cost(f, f.pt, a.w_pose, a.w_beta));
        lm_commit<kFU>(f);
    }
    lm_write<kFU>(f, a, b);
}

}  // namespace scat

using namespace scat;

extern "C" int scat_mano_joints_jac(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                                    const float* hands_mean, const float* rots, const float* poses, const float* betas,
                                    float* joints, float* jac, int B, int V, uint64_t parents, int tip0, int tip1, int tip2,
                                    int tip3, int tip4, void* stream) {
    const void* ptrs[] = {blend, joint_t, joint_s, weights_t, hands_mean, rots, poses, betas, joints, jac};
    const int tips[kMTips] = {tip0, tip1, tip2, tip3, tip4};
    ManoArgs p = {blend, joint_t, joint_s, weights_t, hands_mean, rots, poses, betas, V, 0, parents, {{tip0, tip1, tip2, tip3, tip4}}};
    const int rc = mano_validate("scat_mano_joints_jac", ptrs, 10, B, V, parents, tips, &p.levels);
    if (rc != SCAT_OK) return rc;
    hipLaunchKernelGGL(mano_joints_jac_kernel, dim3(B), dim3(kFThreads), 0, (hipStream_t)stream, p, joints, jac);
    SCAT_LAUNCH_CHECK("scat_mano_joints_jac");
    set_kernel_label("mano_joints_jac_v%d", V);
    return SCAT_OK;
}

extern "C" int scat_mano_fit(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                             const float* hands_mean, const float* targets, const float* weights, const int* joint_map,
                             float* p, float* cost, int* accepted, int B, int V, uint64_t parents, int tip0, int tip1, int tip2,
                             int tip3, int tip4, int iters, int init, float lambda0, float w_pose, float w_beta,
                             uint64_t free_mask, void* stream) {
    const char* fn = "scat_mano_fit";
    const void* ptrs[] = {blend, joint_t, joint_s, weights_t, hands_mean, targets, joint_map, p, cost, accepted};
    const int tips[kMTips] = {tip0, tip1, tip2, tip3, tip4};
    FitArgs a = {fit_model_args(blend, joint_t, joint_s, weights_t, hands_mean, V, parents, tips),
                 targets, weights, joint_map, p, cost, accepted, iters, init, lambda0, w_pose, w_beta, free_mask};
    int rc = mano_validate(fn, ptrs, 10, B, V, parents, tips, &a.m.levels);
    if (rc != SCAT_OK) return rc;
    rc = fit_check_args(fn, "Procrustes", weights, iters, init, lambda0, w_pose, w_beta, free_mask);
    if (rc != SCAT_OK) return rc;
    hipLaunchKernelGGL(mano_fit_kernel, dim3(B), dim3(kFThreads), 0, (hipStream_t)stream, a);
    SCAT_LAUNCH_CHECK(fn);
    set_kernel_label("mano_fit_v%d_i%d", V, iters);
    return SCAT_OK;
}
