// What the two multi-view kernels share (mano_fit_views.hip: one hand per workgroup; mano_fit_seq_views.hip: a track of
// frames per workgroup): the triangulation of a joint from its views, the usable-inputs scan of one frame, the per-joint
// metric M_j and h_j with the robust terms (views_residual), the behind-the-camera flag, the frame's cost and the plane
// MG = blockdiag(M_j) J.  Each works on a kernel's LDS state f and its arguments a, which are template parameters, as in
// mano_fit_kp_common.h.  f has J[63][62], MG[63][62], cam[8][16], tgt[8][42], w[8][21], lo, hi, Mj[21][6], h[63], rho[21],
// behind[21]; a has C, sigma2, z_near, w_pose, w_beta, w_limit.  The walk that assembles the normal equations stays in
// each kernel.  Every sum is a sequential loop: views ascending inside a joint, joints ascending, then the priors, then
// the limits.
#pragma once
#include "mano_fit_kp_common.h"

#include "../../include_ext/scat_mano_fit_views.h"

namespace scat {

constexpr int kVMaxC = SCAT_FIT_VIEWS_MAX_C;
constexpr int kVCam = SCAT_FIT_VIEWS_CAM;

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
template <class F, class A>
__device__ __noinline__ void views_residual(const JacLds& m, F& f, const A& a, const float* pp) {
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
    for (int e = 0; e < 6; ++e) f.Mj[j][e] = M[e];
#pragma unroll
    for (int k = 0; k < 3; ++k) f.h[3 * j + k] = h[k];
}

// one thread, after views_residual
template <class F>
__device__ __forceinline__ int views_behind(const F& f) {
    int b = 0;
    for (int j = 0; j < kFJoints; ++j) b |= f.behind[j];
    return b;
}

// one thread, ascending: the joints, the priors, the limits; one copy, for the same reason
template <class F, class A>
__device__ __noinline__ float views_cost(const F& f, const A& a, const float* pp) {
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

// all threads, after views_residual and a barrier: MG row 3 j + c is row c of M_j times G_j
template <class F>
__device__ __forceinline__ void views_form_mg(F& f) {
    for (int w = threadIdx.x; w < kFRows * kFU; w += kFThreads) {
        const int row = w / kFU, q = w % kFU, j = row / 3, c = row % 3;
        const float m0 = f.Mj[j][c == 0 ? 0 : (c == 1 ? 1 : 2)], m1 = f.Mj[j][c == 0 ? 1 : (c == 1 ? 3 : 4)];
        const float m2 = f.Mj[j][c == 0 ? 2 : (c == 1 ? 4 : 5)];
        f.MG[row][q] = (m0 * f.J[3 * j][q] + m1 * f.J[3 * j + 1][q]) + m2 * f.J[3 * j + 2][q];
    }
}

// init = 1, all threads, after jac_eval of the zero pose: the frame's joints triangulated from the staged cameras, targets
// and weights into f.h with f.rho 1 for a triangulated joint and 0 for the others, then by one thread the Procrustes of the
// zero-pose joints onto them into p[62] when at least three are; returns that count to thread 0 only.  Ends with a barrier.
template <class F>
__device__ __forceinline__ void views_start(const JacLds& m, F& f, int C, float z_near, float* p, int* few) {
    const int tid = threadIdx.x;
    if (tid < kFJoints) {
        double X[3];
        const bool ok = views_triangulate(&f.cam[0][0], &f.tgt[0][2 * tid], kKRows2, &f.w[0][tid], kFJoints, C, z_near, X);
#pragma unroll
        for (int c = 0; c < 3; ++c) f.h[3 * tid + c] = ok ? (float)X[c] : 0.f;
        f.rho[tid] = ok ? 1.f : 0.f;
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int j = 0; j < kFJoints; ++j) n += f.rho[j] > 0.f;
        *few = n < 3;
        if (n >= 3) fit_procrustes(m.x, f.h, f.rho, p);
    }
    __syncthreads();
}

}  // namespace scat

// the checks of the cameras and the keypoints that the multi-view entry points make, each text in one place
static int views_check(const char* fn, const float* weights2, int cam_batch, int B, int C, float z_near) {
    SCAT_REQUIRE(((uintptr_t)weights2 & 3) == 0, SCAT_E_ARG, "%s: fp32 operands must be 4-byte aligned", fn);
    SCAT_REQUIRE(C >= 1 && C <= SCAT_FIT_VIEWS_MAX_C, SCAT_E_SHAPE, "%s: %d views outside 1..%d", fn, C, SCAT_FIT_VIEWS_MAX_C);
    SCAT_REQUIRE(cam_batch == 1 || cam_batch == B, SCAT_E_SHAPE, "%s: cam_batch %d must be 1 (one rig for the batch) or the batch %d",
                 fn, cam_batch, B);
    SCAT_REQUIRE(z_near > 0.f && z_near < INFINITY, SCAT_E_ARG, "%s: z_near %g must be positive and finite", fn, (double)z_near);
    return SCAT_OK;
}
