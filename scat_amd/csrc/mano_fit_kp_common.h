// What the two keypoint kernels share (mano_fit_kp.hip: one frame per workgroup; mano_fit_seq_kp.hip: a track of frames
// per workgroup): the 65 unknowns, the row algebra of the 105 x 65 Jacobian whose 42 2-D rows are not stored (kp_row2_*,
// kp_gram, kp_grad), the robust terms (kp_robust, kp_residual), the limits (kp_excess), a frame's cost (kp_cost) and both
// closed-form starts (kp_camera_start, kp_start_2d).  Each works on a kernel's LDS state f and its arguments a, which
// are template parameters.  f has J[63][62], p-sized vectors, tgt3, tgt2, w3, w2, lo, hi, r, wrow, wr, rho, dcs, k2; a has
// sigma3, sigma2, half[2], w_pose, w_beta, w_limit, free_mask, free_cam.  The walk that assembles the normal equations
// stays in each kernel (mano_fit_common.h has why).  Every sum is a sequential loop: rows 0..62 (3-D joints ascending),
// rows 63..104 (2-D joints ascending), then the priors, then the limits.
#pragma once
#include "mano_fit_common.h"

#include "../../include/scat_mano_fit_kp.h"

namespace scat {

constexpr int kKU = SCAT_FIT_KP_UNKNOWNS;     // 65
constexpr int kKCam = kFU;                    // 62: cs, then ctx, cty
constexpr int kKRows2 = 2 * kFJoints;         // 42
constexpr int kKRows = kFRows + kKRows2;      // 105

template <class A>
__device__ __forceinline__ bool kp_free(const A& a, int i) {
    return i < kFU ? ((a.free_mask >> i) & 1u) : (((unsigned)a.free_cam >> (i - kFU)) & 1u);
}

// A 2-D row q = 2 j + c of the 105 x 65 Jacobian: a model column (col < 62) is cs half_c times the 3-D row 3 j + c ...
template <class F>
__device__ __forceinline__ float kp_row2_model(const F& f, int q, int col) {
    return f.k2[q & 1] * f.J[3 * (q >> 1) + (q & 1)][col];
}

// ... and a camera column is (m_c + ct_c) half_c for cs, cs half_c for its own offset, zero for the other
template <class F>
__device__ __forceinline__ float kp_row2_cam(const F& f, int q, int col) {
    return col == kKCam ? f.dcs[q] : (col - (kKCam + 1) == (q & 1) ? f.k2[q & 1] : 0.f);
}

// sum over the rows of wrow J[row][ai] J[row][bi], bi <= ai: rows 0..62, then 63..104.  The 3-D rows are zero in the
// camera columns; the loops have constant trip counts and no branch inside, so that their LDS reads overlap.
template <class F>
__device__ __forceinline__ float kp_gram(const F& f, int ai, int bi, bool has3, bool has2) {
    float s = 0.f;
    if (has3 && ai < kFU) {
        for (int row = 0; row < kFRows; ++row) s += f.wrow[row] * f.J[row][ai] * f.J[row][bi];
    }
    if (has2) {
        if (ai < kFU) {
            for (int q = 0; q < kKRows2; ++q) s += f.wrow[kFRows + q] * kp_row2_model(f, q, ai) * kp_row2_model(f, q, bi);
        } else if (bi < kFU) {
            for (int q = 0; q < kKRows2; ++q) s += f.wrow[kFRows + q] * kp_row2_cam(f, q, ai) * kp_row2_model(f, q, bi);
        } else {
            for (int q = 0; q < kKRows2; ++q) s += f.wrow[kFRows + q] * kp_row2_cam(f, q, ai) * kp_row2_cam(f, q, bi);
        }
    }
    return s;
}

// sum over the rows of J[row][bi] (wrow r)[row], the same order
template <class F>
__device__ __forceinline__ float kp_grad(const F& f, int bi, bool has3, bool has2) {
    float g = 0.f;
    if (has3 && bi < kFU) {
        for (int row = 0; row < kFRows; ++row) g += f.J[row][bi] * f.wr[row];
    }
    if (has2) {
        if (bi < kFU) {
            for (int q = 0; q < kKRows2; ++q) g += kp_row2_model(f, q, bi) * f.wr[kFRows + q];
        } else {
            for (int q = 0; q < kKRows2; ++q) g += kp_row2_cam(f, q, bi) * f.wr[kFRows + q];
        }
    }
    return g;
}

// one joint's robust terms: e its squared distance, w its weight -> the rows' weight w rho'(e) and w rho(e)
__device__ __forceinline__ void kp_robust(float e, float w, float sigma, float* wi, float* rho) {
    if (!(w > 0.f)) {
        *wi = 0.f, *rho = 0.f;
    } else if (sigma > 0.f) {
        const float s2 = sigma * sigma, q = s2 / (s2 + e);
        *wi = w * (q * q);
        *rho = w * (q * e);
    } else {
        *wi = w, *rho = w * e;
    }
}

// residuals, row weights and robust terms of the model joints m.x under the similarity and camera of pp; with_cols: the
// four similarity columns of J and the camera's derivatives as well.  One thread per joint.
template <class F, class A>
__device__ __forceinline__ void kp_residual(const JacLds& m, F& f, const A& a, const float* pp, bool with_cols) {
    const int j = threadIdx.x;
    if (j >= kFJoints) return;
    const float s = expf(pp[kFU - 1]), cs = pp[kKCam];
    float mj[3], r3[3], wi, rho;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float sx = s * m.x[3 * j + c];
        mj[c] = sx + pp[kFModel + c];
        r3[c] = mj[c] - f.tgt3[3 * j + c];
        if (with_cols) {
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) f.J[3 * j + c][kFModel + cc] = cc == c ? 1.f : 0.f;
            f.J[3 * j + c][kFU - 1] = sx;
        }
    }
    kp_robust((r3[0] * r3[0] + r3[1] * r3[1]) + r3[2] * r3[2], f.w3[j], a.sigma3, &wi, &rho);
    f.rho[j] = rho;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f.r[3 * j + c] = r3[c];
        f.wrow[3 * j + c] = wi;
        f.wr[3 * j + c] = wi > 0.f ? wi * r3[c] : 0.f;
    }
    float r2[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float d = mj[c] + pp[kKCam + 1 + c];
        r2[c] = ((cs * d) * a.half[c] + a.half[c]) - f.tgt2[2 * j + c];
        if (with_cols) {
            f.dcs[2 * j + c] = d * a.half[c];
            if (j == 0) f.k2[c] = cs * a.half[c];
        }
    }
    kp_robust(r2[0] * r2[0] + r2[1] * r2[1], f.w2[j], a.sigma2, &wi, &rho);
    f.rho[kFJoints + j] = rho;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        f.r[kFRows + 2 * j + c] = r2[c];
        f.wrow[kFRows + 2 * j + c] = wi;
        f.wr[kFRows + 2 * j + c] = wi > 0.f ? wi * r2[c] : 0.f;
    }
}

// how far pose i is outside its limits, signed: > 0 above hi, < 0 below lo; an entry that is not finite is no limit
template <class F>
__device__ __forceinline__ float kp_excess(const F& f, const float* pp, int i) {
    const float v = pp[3 + i];
    if (fit_finite(f.hi[i]) && v > f.hi[i]) return v - f.hi[i];
    if (fit_finite(f.lo[i]) && v < f.lo[i]) return -(f.lo[i] - v);
    return 0.f;
}

// one thread, ascending: the 3-D joints, the 2-D joints, the priors, the limits
template <class F, class A>
__device__ __forceinline__ float kp_cost(const F& f, const A& a, const float* pp) {
    float c3 = 0.f, c2 = 0.f, sp = 0.f, sb = 0.f, sl = 0.f;
    for (int j = 0; j < kFJoints; ++j) c3 += f.rho[j];
    for (int j = 0; j < kFJoints; ++j) c2 += f.rho[kFJoints + j];
    for (int i = 3; i < 3 + kFPose; ++i) sp += pp[i] * pp[i];
    for (int i = 3 + kFPose; i < kFModel; ++i) sb += pp[i] * pp[i];
    for (int i = 0; i < kFPose; ++i) {
        const float d = kp_excess(f, pp, i);
        sl += d * d;
    }
    return ((c3 + c2) + (a.w_pose * sp + a.w_beta * sb)) + a.w_limit * sl;
}

__device__ inline void kp_rodrigues(const double r[3], double R[9]) {
    const double x = r[0], y = r[1], z = r[2], t = x * x + y * y + z * z, th = sqrt(t);
    const double ca = t < 1e-16 ? 1.0 : sin(th) / th, cb = t < 1e-16 ? 0.5 : (1.0 - cos(th)) / t;
    R[0] = 1.0 + cb * (x * x - t), R[1] = cb * x * y - ca * z, R[2] = cb * x * z + ca * y;
    R[3] = cb * x * y + ca * z, R[4] = 1.0 + cb * (y * y - t), R[5] = cb * y * z - ca * x;
    R[6] = cb * x * z - ca * y, R[7] = cb * y * z + ca * x, R[8] = 1.0 + cb * (z * z - t);
}

// init = 1 with a 3-D term, one thread, after fit_procrustes: the camera that takes m.xy at the start p onto the
// normalised 2-D targets, one isotropic scale
template <class F, class A>
__device__ void kp_camera_start(const float* x, const F& f, const A& a, float* p) {
    double R[9], W = 0.0, ab[2] = {0, 0}, yb[2] = {0, 0}, av[kFJoints][2], yv[kFJoints][2];
    const double r[3] = {p[0], p[1], p[2]}, s = exp((double)p[kFU - 1]);
    kp_rodrigues(r, R);
    for (int j = 0; j < kFJoints; ++j) {
        const double w = f.w2[j];
        W += w;
        for (int c = 0; c < 2; ++c) {
            av[j][c] = s * (R[3 * c] * x[3 * j] + R[3 * c + 1] * x[3 * j + 1] + R[3 * c + 2] * x[3 * j + 2]) + p[kFModel + c];
            yv[j][c] = ((double)f.tgt2[2 * j + c] - a.half[c]) / a.half[c];
            ab[c] += w * av[j][c];
            yb[c] += w * yv[j][c];
        }
    }
    for (int c = 0; c < 2; ++c) {
        ab[c] /= W;
        yb[c] /= W;
    }
    double num = 0.0, den = 0.0;
    for (int j = 0; j < kFJoints; ++j)
        for (int c = 0; c < 2; ++c) {
            const double da = av[j][c] - ab[c];
            num += f.w2[j] * da * (yv[j][c] - yb[c]);
            den += f.w2[j] * da * da;
        }
    const double cs = num / den;
    if (cs > 1e-30 && cs < 1e30) {
        p[kKCam] = (float)cs;
        p[kKCam + 1] = (float)(yb[0] / cs - ab[0]);
        p[kKCam + 2] = (float)(yb[1] / cs - ab[1]);
    }
}

// init = 1 with 2-D targets only, one thread: x the zero-pose joints.  Rz(phi) and Rz(phi) Ry(pi) by the weighted complex
// least squares y ~ z a + t, a = (C x).xy; the smaller residual wins, a tie goes to the first
template <class F, class A>
__device__ void kp_start_2d(const float* x, const F& f, const A& a, float* p) {
    double best_res = 0.0, bz[2] = {0, 0}, bt[2] = {0, 0};
    int best = 0;
    for (int k = 0; k < 2; ++k) {
        const double sx = k ? -1.0 : 1.0;   // Ry(pi) (x, y, z) = (-x, y, -z)
        double W = 0.0, ab[2] = {0, 0}, yb[2] = {0, 0}, yv[kFJoints][2];
        for (int j = 0; j < kFJoints; ++j) {
            const double w = f.w2[j];
            W += w;
            ab[0] += w * sx * x[3 * j], ab[1] += w * x[3 * j + 1];
            for (int c = 0; c < 2; ++c) {
                yv[j][c] = ((double)f.tgt2[2 * j + c] - a.half[c]) / a.half[c];
                yb[c] += w * yv[j][c];
            }
        }
        for (int c = 0; c < 2; ++c) {
            ab[c] /= W;
            yb[c] /= W;
        }
        double nr = 0.0, ni = 0.0, den = 0.0;
        for (int j = 0; j < kFJoints; ++j) {
            const double w = f.w2[j], ax = sx * x[3 * j] - ab[0], ay = x[3 * j + 1] - ab[1];
            const double yx = yv[j][0] - yb[0], yy = yv[j][1] - yb[1];
            nr += w * (ax * yx + ay * yy);   // conj(a) y
            ni += w * (ax * yy - ay * yx);
            den += w * (ax * ax + ay * ay);
        }
        const double zr = nr / den, zi = ni / den;
        double res = 0.0;
        for (int j = 0; j < kFJoints; ++j) {
            const double ax = sx * x[3 * j] - ab[0], ay = x[3 * j + 1] - ab[1];
            const double ex = (yv[j][0] - yb[0]) - (zr * ax - zi * ay), ey = (yv[j][1] - yb[1]) - (zr * ay + zi * ax);
            res += f.w2[j] * (ex * ex + ey * ey);
        }
        if (k == 0 || res < best_res) {
            best = k, best_res = res;
            bz[0] = zr, bz[1] = zi;
            bt[0] = yb[0] - (zr * ab[0] - zi * ab[1]);
            bt[1] = yb[1] - (zr * ab[1] + zi * ab[0]);
        }
    }
    const double cs = sqrt(bz[0] * bz[0] + bz[1] * bz[1]);
    if (!(cs > 1e-30 && cs < 1e30)) return;   // a degenerate point set: p stays the identity
    const double phi = atan2(bz[1], bz[0]), c = cos(phi), s = sin(phi);
    const double R0[9] = {c, -s, 0, s, c, 0, 0, 0, 1}, R1[9] = {-c, -s, 0, -s, c, 0, 0, 0, -1};
    fit_axis_angle(best ? R1 : R0, p);
    p[kKCam] = (float)cs;
    p[kKCam + 1] = (float)(bt[0] / cs);
    p[kKCam + 2] = (float)(bt[1] / cs);
}

// init = 1 of one frame, one thread: p (zeros and the camera (1, 0, 0) on entry) from the zero-pose joints x and the
// frame's targets and weights in f; has3 / has2: the term is present
template <class F, class A>
__device__ __forceinline__ void kp_start(const float* x, const F& f, const A& a, float* p, bool has3, bool has2) {
    float W3 = 0.f;
    for (int j = 0; j < kFJoints; ++j) W3 += f.w3[j];
    if (W3 > 0.f || !has2) {
        fit_procrustes(x, f.tgt3, f.w3, p);
        if (has2) kp_camera_start(x, f, a, p);
    } else {
        kp_start_2d(x, f, a, p);
    }
}

}  // namespace scat

static bool kp_weight_ok(float v) { return v >= 0.f && v < INFINITY; }

// The checks of the camera, the robust loss and the limits that both keypoint entry points make, each text in one place
static int kp_check_terms(const char* fn, const float* targets3, const float* weights3, const float* targets2,
                          const float* weights2, const float* pose_lo, const float* pose_hi) {
    const uintptr_t opt = (uintptr_t)targets3 | (uintptr_t)weights3 | (uintptr_t)targets2 | (uintptr_t)weights2 |
                          (uintptr_t)pose_lo | (uintptr_t)pose_hi;
    SCAT_REQUIRE((opt & 3) == 0, SCAT_E_ARG, "%s: fp32 operands must be 4-byte aligned", fn);
    SCAT_REQUIRE(targets3 || targets2, SCAT_E_ARG, "%s: no targets: targets3 and targets2 are both null", fn);
    SCAT_REQUIRE(targets3 || !weights3, SCAT_E_ARG, "%s: weights3 given without targets3", fn);
    SCAT_REQUIRE(targets2 || !weights2, SCAT_E_ARG, "%s: weights2 given without targets2", fn);
    SCAT_REQUIRE(!pose_lo == !pose_hi, SCAT_E_ARG, "%s: pose_lo and pose_hi must both be given or both be null", fn);
    return SCAT_OK;
}

static int kp_check_loss(const char* fn, float w_limit, float sigma3, float sigma2, float half_w, float half_h) {
    SCAT_REQUIRE(kp_weight_ok(w_limit), SCAT_E_ARG, "%s: w_limit %g must be finite and not negative", fn, (double)w_limit);
    SCAT_REQUIRE(kp_weight_ok(sigma3), SCAT_E_ARG, "%s: sigma3 %g must be finite and not negative", fn, (double)sigma3);
    SCAT_REQUIRE(kp_weight_ok(sigma2), SCAT_E_ARG, "%s: sigma2 %g must be finite and not negative", fn, (double)sigma2);
    SCAT_REQUIRE(half_w > 0.f && half_w < INFINITY, SCAT_E_ARG, "%s: half_w %g must be positive and finite", fn, (double)half_w);
    SCAT_REQUIRE(half_h > 0.f && half_h < INFINITY, SCAT_E_ARG, "%s: half_h %g must be positive and finite", fn, (double)half_h);
    return SCAT_OK;
}
