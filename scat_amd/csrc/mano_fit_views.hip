// The MANO fit to keypoints seen by C calibrated pinhole cameras, include_ext/scat_mano_fit_views.h: mano_fit_kernel's
// Levenberg-Marquardt on scat_mano_fit's 62 unknowns with a perspective reprojection term per view, Geman-McClure
// weights (IRLS) and joint limits, and the triangulation that makes its start.  One workgroup of 256 threads per hand,
// all iterations in one launch, everything in LDS; jac_eval, the Procrustes start and the solver's steps (lm_solve,
// lm_accept, lm_commit, lm_write) are mano_fit_common.h's, kp_robust and kp_excess mano_fit_kp_common.h's.
//
// The 42 C rows are not stored.  A view-joint's two rows are P G_j with P = D R_c (2 x 3) and G_j rows 3 j .. 3 j + 2 of
// the stored 63 x 62 Jacobian, so one thread per joint sums its views into M_j = sum_c wi P^T P and h_j = sum_c wi P^T r
// (views_residual), all threads form the plane MG = blockdiag(M_j) J once, and the walk over the normal equations is
// mano_fit_kernel's with MG in the place of W J: A = J^T MG, g = J^T h.  Neither the walk nor LDS grow with C.  Every sum
// is a sequential loop: views ascending inside a joint, joints ascending, then the priors, then the limits.
#include "mano_fit_kp_common.h"

#include "../../include_ext/scat_mano_fit_views.h"

namespace scat {

constexpr int kVMaxC = SCAT_FIT_VIEWS_MAX_C;
constexpr int kVCam = SCAT_FIT_VIEWS_CAM;

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
    float M[kFJoints][6];      // M_j: xx, xy, xz, yy, yz, zz
    float h[kFRows];           // h_j; before the iterations the triangulated joints
    float rho[kFJoints];       // sum_c w rho(e) of a joint; before the iterations 1 for a triangulated joint, else 0
    int behind[kFJoints];      // a view of positive weight has the joint at q.z <= z_near
    float cost, lambda;
    int acc, bad, fail, take;
};

// One joint from its views, in fp64: cams[C][16], tgt the joint's first view (the next is tstride floats on), w likewise
// (null: all ones) -> X and true, or false when the joint is not triangulated (the header has the three conditions)
__device__ bool views_triangulate(const float* cams, const float* tgt, int tstride, const float* w, int wstride, int C,
                                  float z_near, double X[3]) {
    double S[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};   // xx, xy, xz, yy, yz, zz
    int n = 0;
    for (int v = 0; v < C; ++v) {
        const double wv = w ? (double)w[v * wstride] : 1.0;
        if (!(wv > 0.0)) continue;
        ++n;
        const float* c = cams + v * kVCam;
        const double dc[3] = {((double)tgt[v * tstride] - c[14]) / c[12], ((double)tgt[v * tstride + 1] - c[15]) / c[13], 1.0};
        double d[3], o[3];
        for (int k = 0; k < 3; ++k) {   // R^T
            d[k] = c[k] * dc[0] + c[3 + k] * dc[1] + c[6 + k] * dc[2];
            o[k] = -((double)c[k] * c[9] + (double)c[3 + k] * c[10] + (double)c[6 + k] * c[11]);
        }
        const double nd = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        for (int k = 0; k < 3; ++k) d[k] /= nd;
        const double od = o[0] * d[0] + o[1] * d[1] + o[2] * d[2];
        S[0] += wv * (1.0 - d[0] * d[0]), S[1] -= wv * d[0] * d[1], S[2] -= wv * d[0] * d[2];
        S[3] += wv * (1.0 - d[1] * d[1]), S[4] -= wv * d[1] * d[2], S[5] += wv * (1.0 - d[2] * d[2]);
        for (int k = 0; k < 3; ++k) b[k] += wv * (o[k] - od * d[k]);
    }
    if (n < 2) return false;
    const double floor = 1e-6 * (S[0] + S[3] + S[5]);
    if (!(S[0] > floor)) return false;
    const double l00 = sqrt(S[0]), l10 = S[1] / l00, l20 = S[2] / l00, p1 = S[3] - l10 * l10;
    if (!(p1 > floor)) return false;
    const double l11 = sqrt(p1), l21 = (S[4] - l20 * l10) / l11, p2 = S[5] - l20 * l20 - l21 * l21;
    if (!(p2 > floor)) return false;
    const double l22 = sqrt(p2);
    const double y0 = b[0] / l00, y1 = (b[1] - l10 * y0) / l11, y2 = (b[2] - l20 * y0 - l21 * y1) / l22;
    X[2] = y2 / l22;
    X[1] = (y1 - l21 * X[2]) / l11;
    X[0] = (y0 - l10 * X[1] - l20 * X[2]) / l00;
    for (int v = 0; v < C; ++v) {
        if (w && !(w[v * wstride] > 0.f)) continue;
        const float* c = cams + v * kVCam;
        const double z = (c[6] * X[0] + c[7] * X[1] + c[8] * X[2]) + c[11];
        if (!(z > (double)z_near)) return false;
    }
    return true;
}

// This thread's share of the usable-inputs scan of one sample: C cameras, their 21 C keypoints and weights (may be null)
__device__ __forceinline__ int views_unusable(const float* cams, const float* tgt, const float* w, int C, int nthreads) {
    const int tid = threadIdx.x;
    int bad = 0;
    for (int i = tid; i < C * kVCam; i += nthreads) bad |= !fit_finite(cams[i]);
    for (int i = tid; i < C * kKRows2; i += nthreads) bad |= !fit_finite(tgt[i]);
    if (w) {
        for (int i = tid; i < C * kFJoints; i += nthreads) bad |= !(fit_finite(w[i]) && w[i] >= 0.f);
    }
    return bad;
}

// One thread per joint: the four similarity columns of J, and the model joints m.x under the similarity of pp through the
// views of positive weight in ascending order: the joint's robust term, M_j, h_j, and whether a view has it behind z_near.
// Not inlined, and the same work at p and at a trial (whose columns, M and h the next iteration overwrites): the cost of a
// trial that equals p, as with every unknown frozen, must have the bits of the cost at p, and two inlined copies, one of
// them without the columns, do not contract their products alike
__device__ __noinline__ void views_residual(const JacLds& m, ViewsLds& f, const ViewsArgs& a, const float* pp) {
    const int j = threadIdx.x;
    if (j >= kFJoints) return;
    const float s = expf(pp[kFU - 1]);
    float mj[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float sx = s * m.x[3 * j + c];
        mj[c] = sx + pp[kFModel + c];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) f.J[3 * j + c][kFModel + cc] = cc == c ? 1.f : 0.f;
        f.J[3 * j + c][kFU - 1] = sx;
    }
    float M[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, h[3] = {0.f, 0.f, 0.f}, rho = 0.f;
    int behind = 0;
    for (int v = 0; v < a.C; ++v) {
        const float w = f.w[v][j];
        if (!(w > 0.f)) continue;
        const float* c = f.cam[v];
        float q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = ((c[3 * k] * mj[0] + c[3 * k + 1] * mj[1]) + c[3 * k + 2] * mj[2]) + c[9 + k];
        if (!(q[2] > a.z_near)) {   // also a q that is not a number
            behind = 1;
            continue;
        }
        const float iz = 1.f / q[2], ax = c[12] * iz, ay = c[13] * iz, px = ax * q[0], py = ay * q[1], bx = -px * iz, by = -py * iz;
        const float r0 = (px + c[14]) - f.tgt[v][2 * j], r1 = (py + c[15]) - f.tgt[v][2 * j + 1];
        float wi, rh, P0[3], P1[3];   // D R_c
        kp_robust(r0 * r0 + r1 * r1, w, a.sigma2, &wi, &rh);
        rho += rh;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            P0[k] = ax * c[k] + bx * c[6 + k];
            P1[k] = ay * c[3 + k] + by * c[6 + k];
        }
        M[0] += wi * (P0[0] * P0[0] + P1[0] * P1[0]), M[1] += wi * (P0[0] * P0[1] + P1[0] * P1[1]);
        M[2] += wi * (P0[0] * P0[2] + P1[0] * P1[2]), M[3] += wi * (P0[1] * P0[1] + P1[1] * P1[1]);
        M[4] += wi * (P0[1] * P0[2] + P1[1] * P1[2]), M[5] += wi * (P0[2] * P0[2] + P1[2] * P1[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) h[k] += wi * (P0[k] * r0 + P1[k] * r1);
    }
    f.rho[j] = rho;
    f.behind[j] = behind;
#pragma unroll
    for (int e = 0; e < 6; ++e) f.M[j][e] = M[e];
#pragma unroll
    for (int k = 0; k < 3; ++k) f.h[3 * j + k] = h[k];
}

// one thread, after views_residual
__device__ __forceinline__ int views_behind(const ViewsLds& f) {
    int b = 0;
    for (int j = 0; j < kFJoints; ++j) b |= f.behind[j];
    return b;
}

// one thread, ascending: the joints, the priors, the limits; one copy, for the same reason
__device__ __noinline__ float views_cost(const ViewsLds& f, const ViewsArgs& a, const float* pp) {
    float c2 = 0.f, sp = 0.f, sb = 0.f, sl = 0.f;
    for (int j = 0; j < kFJoints; ++j) c2 += f.rho[j];
    for (int i = 3; i < 3 + kFPose; ++i) sp += pp[i] * pp[i];
    for (int i = 3 + kFPose; i < kFModel; ++i) sb += pp[i] * pp[i];
    for (int i = 0; i < kFPose; ++i) {
        const float d = kp_excess(f, pp, i);
        sl += d * d;
    }
    return (c2 + (a.w_pose * sp + a.w_beta * sb)) + a.w_limit * sl;
}

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
        if (tid < kFJoints) {
            double X[3];
            const bool ok = views_triangulate(&f.cam[0][0], &f.tgt[0][2 * tid], kKRows2, &f.w[0][tid], kFJoints, C, a.z_near, X);
#pragma unroll
            for (int c = 0; c < 3; ++c) f.h[3 * tid + c] = ok ? (float)X[c] : 0.f;
            f.rho[tid] = ok ? 1.f : 0.f;
        }
        __syncthreads();
        if (tid == 0) {
            int n = 0;
            for (int j = 0; j < kFJoints; ++j) n += f.rho[j] > 0.f;
            f.bad = n < 3;
            if (n >= 3) fit_procrustes(m.x, f.h, f.rho, f.p);
        }
        __syncthreads();
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
        for (int w = tid; w < kFRows * kFU; w += kFThreads) {
            const int row = w / kFU, q = w % kFU, j = row / 3, c = row % 3;
            const float m0 = f.M[j][c == 0 ? 0 : (c == 1 ? 1 : 2)], m1 = f.M[j][c == 0 ? 1 : (c == 1 ? 3 : 4)];
            const float m2 = f.M[j][c == 0 ? 2 : (c == 1 ? 4 : 5)];
            f.MG[row][q] = (m0 * f.J[3 * j][q] + m1 * f.J[3 * j + 1][q]) + m2 * f.J[3 * j + 2][q];
        }
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

// the checks of the cameras and the keypoints that both entry points make, each text in one place
static int views_check(const char* fn, const float* weights2, int cam_batch, int B, int C, float z_near) {
    SCAT_REQUIRE(((uintptr_t)weights2 & 3) == 0, SCAT_E_ARG, "%s: fp32 operands must be 4-byte aligned", fn);
    SCAT_REQUIRE(C >= 1 && C <= SCAT_FIT_VIEWS_MAX_C, SCAT_E_SHAPE, "%s: %d views outside 1..%d", fn, C, SCAT_FIT_VIEWS_MAX_C);
    SCAT_REQUIRE(cam_batch == 1 || cam_batch == B, SCAT_E_SHAPE, "%s: cam_batch %d must be 1 (one rig for the batch) or the batch %d",
                 fn, cam_batch, B);
    SCAT_REQUIRE(z_near > 0.f && z_near < INFINITY, SCAT_E_ARG, "%s: z_near %g must be positive and finite", fn, (double)z_near);
    return SCAT_OK;
}

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
