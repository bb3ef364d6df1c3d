// The MANO fit to keypoints, include/scat_mano_fit_kp.h: mano_fit_kernel's Levenberg-Marquardt with a 2-D reprojection
// term through a weak-perspective camera, Geman-McClure weights (IRLS) and joint limits.  One workgroup of 256 threads per
// sample, all iterations in one launch, everything in LDS; jac_eval, the Procrustes start, the constants and the solver's
// steps that do not depend on the problem (lm_solve, lm_accept, lm_commit, lm_write) are mano_fit_common.h's.
//
// 65 unknowns: scat_mano_fit's 62, then cs, ctx, cty.  The 42 rows of the 2-D term are not stored: in the first 62 columns
// row (j, c) of the 2-D term is cs half_c times row 3 j + c of the 3-D Jacobian, and its three camera columns are
// (m_c + ct_c) half_c, and cs half_c on its own offset.  kp_gram() and kp_grad() sum over all 105 rows from the stored
// 63 x 62 Jacobian, so LDS stays at J (63 x 62) and the normal matrix (66 x 65, g as the last row).  Every sum is a
// sequential loop: rows 0..62 (3-D joints ascending), rows 63..104 (2-D joints ascending), then the priors, then the
// limits.
#include "mano_fit_common.h"

#include "../../include/scat_mano_fit_kp.h"

namespace scat {

constexpr int kKU = SCAT_FIT_KP_UNKNOWNS;     // 65
constexpr int kKCam = kFU;                    // 62: cs, then ctx, cty
constexpr int kKRows2 = 2 * kFJoints;         // 42
constexpr int kKRows = kFRows + kKRows2;      // 105

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

__device__ __forceinline__ bool kp_free(const KpArgs& a, int i) {
    return i < kFU ? ((a.free_mask >> i) & 1u) : (((unsigned)a.free_cam >> (i - kFU)) & 1u);
}

// A 2-D row q = 2 j + c of the 105 x 65 Jacobian: a model column (col < 62) is cs half_c times the 3-D row 3 j + c ...
__device__ __forceinline__ float kp_row2_model(const KpLds& f, int q, int col) {
    return f.k2[q & 1] * f.J[3 * (q >> 1) + (q & 1)][col];
}

// ... and a camera column is (m_c + ct_c) half_c for cs, cs half_c for its own offset, zero for the other
__device__ __forceinline__ float kp_row2_cam(const KpLds& f, int q, int col) {
    return col == kKCam ? f.dcs[q] : (col - (kKCam + 1) == (q & 1) ? f.k2[q & 1] : 0.f);
}

// sum over the rows of wrow J[row][ai] J[row][bi], bi <= ai: rows 0..62, then 63..104.  The 3-D rows are zero in the
// camera columns; the loops have constant trip counts and no branch inside, so that their LDS reads overlap.
__device__ __forceinline__ float kp_gram(const KpLds& f, int ai, int bi, bool has3, bool has2) {
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
__device__ __forceinline__ float kp_grad(const KpLds& f, int bi, bool has3, bool has2) {
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
__device__ __forceinline__ void kp_residual(const JacLds& m, KpLds& f, const KpArgs& a, const float* pp, bool with_cols) {
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
__device__ __forceinline__ float kp_excess(const KpLds& f, const float* pp, int i) {
    const float v = pp[3 + i];
    if (fit_finite(f.hi[i]) && v > f.hi[i]) return v - f.hi[i];
    if (fit_finite(f.lo[i]) && v < f.lo[i]) return -(f.lo[i] - v);
    return 0.f;
}

// one thread, ascending: the 3-D joints, the 2-D joints, the priors, the limits
__device__ __forceinline__ float kp_cost(const KpLds& f, const KpArgs& a, const float* pp) {
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

__device__ void kp_rodrigues(const double r[3], double R[9]) {
    const double x = r[0], y = r[1], z = r[2], t = x * x + y * y + z * z, th = sqrt(t);
    const double ca = t < 1e-16 ? 1.0 : sin(th) / th, cb = t < 1e-16 ? 0.5 : (1.0 - cos(th)) / t;
    R[0] = 1.0 + cb * (x * x - t), R[1] = cb * x * y - ca * z, R[2] = cb * x * z + ca * y;
    R[3] = cb * x * y + ca * z, R[4] = 1.0 + cb * (y * y - t), R[5] = cb * y * z - ca * x;
    R[6] = cb * x * z - ca * y, R[7] = cb * y * z + ca * x, R[8] = 1.0 + cb * (z * z - t);
}

// init = 1 with a 3-D term, one thread, after fit_procrustes: the camera that takes m.xy at the start p onto the
// normalised 2-D targets, one isotropic scale
__device__ void kp_camera_start(const float* x, const KpLds& f, const KpArgs& a, float* p) {
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
__device__ void kp_start_2d(const float* x, const KpLds& f, const KpArgs& a, float* p) {
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
        if (tid == 0) {
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

static bool kp_weight_ok(float v) { return v >= 0.f && v < INFINITY; }

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
    const uintptr_t opt = (uintptr_t)targets3 | (uintptr_t)weights3 | (uintptr_t)targets2 | (uintptr_t)weights2 |
                          (uintptr_t)pose_lo | (uintptr_t)pose_hi;
    SCAT_REQUIRE((opt & 3) == 0, SCAT_E_ARG, "%s: fp32 operands must be 4-byte aligned", fn);
    SCAT_REQUIRE(targets3 || targets2, SCAT_E_ARG, "%s: no targets: targets3 and targets2 are both null", fn);
    SCAT_REQUIRE(targets3 || !weights3, SCAT_E_ARG, "%s: weights3 given without targets3", fn);
    SCAT_REQUIRE(targets2 || !weights2, SCAT_E_ARG, "%s: weights2 given without targets2", fn);
    SCAT_REQUIRE(!pose_lo == !pose_hi, SCAT_E_ARG, "%s: pose_lo and pose_hi must both be given or both be null", fn);
    rc = fit_check_solver(fn, "the closed-form start", iters, init, lambda0, w_pose, w_beta);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE(kp_weight_ok(w_limit), SCAT_E_ARG, "%s: w_limit %g must be finite and not negative", fn, (double)w_limit);
    SCAT_REQUIRE(kp_weight_ok(sigma3), SCAT_E_ARG, "%s: sigma3 %g must be finite and not negative", fn, (double)sigma3);
    SCAT_REQUIRE(kp_weight_ok(sigma2), SCAT_E_ARG, "%s: sigma2 %g must be finite and not negative", fn, (double)sigma2);
    SCAT_REQUIRE(half_w > 0.f && half_w < INFINITY, SCAT_E_ARG, "%s: half_w %g must be positive and finite", fn, (double)half_w);
    SCAT_REQUIRE(half_h > 0.f && half_h < INFINITY, SCAT_E_ARG, "%s: half_h %g must be positive and finite", fn, (double)half_h);
    rc = fit_check_mask(fn, free_mask);
    if (rc != SCAT_OK) return rc;
    SCAT_REQUIRE(free_cam >= 0 && free_cam <= 7, SCAT_E_ARG, "%s: free_cam %d outside 0..7", fn, free_cam);
    hipLaunchKernelGGL(mano_fit_kp_kernel, dim3(B), dim3(kFThreads), 0, (hipStream_t)stream, a);
    SCAT_LAUNCH_CHECK(fn);
    set_kernel_label("mano_fit_kp_v%d_i%d", V, iters);
    return SCAT_OK;
}
