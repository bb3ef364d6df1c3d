// What the MANO kernels share (mano.hip: the layer; mano_fit.hip: the joints' Jacobian and the fit): the pose state a
// workgroup keeps in LDS, Rodrigues in t = theta^2, the 3 x 3 helpers, mano_setup, mano_vertex and the host-side checks of
// the by-value tree and tips.  include/scat_mano.h has the semantics.
#pragma once
#include "common.h"

#include "../../include/scat_mano.h"

namespace scat {

constexpr int kMJ = SCAT_MANO_JOINTS;      // 16
constexpr int kMTips = SCAT_MANO_TIPS;     // 5
constexpr int kMBeta = 10;
constexpr int kMPw = 9 * (kMJ - 1);        // 135
constexpr int kMCoef = kMBeta + kMPw;      // 145
constexpr int kMThreads = 1024;
constexpr int kMWaves = kMThreads / 64;
constexpr int kMMaxV = SCAT_MANO_MAX_V;
constexpr int kMBlendGroup = 5;            // partial sums of the forward blend, and coefficients per phase-2 unit: 145 = 29 x 5
constexpr int kMUnits = kMJ + kMCoef / kMBlendGroup;
static_assert(kMCoef % kMBlendGroup == 0, "blend units must tile the coefficients");
constexpr float kMSeries = 0.25f;          // theta^2 below which a, b and their derivatives come from the series

struct ManoTips { int v[kMTips]; };

struct ManoArgs {
    const float* blend;       // [146][3][V]
    const float* joint_t;     // [16][3]
    const float* joint_s;     // [16][3][10]
    const float* weights_t;   // [16][V]
    const float* hands_mean;  // [45]
    const float* rots;        // [B,3]
    const float* poses;       // [B,45]
    const float* betas;       // [B,10]
    int V;
    int levels;               // depth of the deepest joint
    uint64_t parents;
    ManoTips tips;
};

struct ManoPose {
    float coef[kMCoef];    // beta[10], then R_k - I for k = 1..15, row-major
    float r[kMJ][3];       // the chain's axis-angles (r[0] = 0)
    float R[kMJ][9];
    float J[kMJ][3];
    float RG[kMJ][9];      // rotation of G_i
    float t[kMJ][3];       // translation of G_i: the posed joint
    float a[kMJ][3];       // t_i - RG_i J_i
    float rg[3];           // rots
    float Rg[9];
};

__device__ __forceinline__ int mano_parent(uint64_t parents, int i) { return (int)((parents >> (4 * i)) & 15u); }

__device__ __forceinline__ int mano_depth(uint64_t parents, int i) {
    int d = 0;
    while (i > 0) {   // parent[i] < i: ends at the root in at most 15 steps
        i = mano_parent(parents, i);
        ++d;
    }
    return d;
}

// a = sin(theta)/theta, b = (1 - cos(theta))/theta^2 and their derivatives by t = theta^2
struct RodCoef { float a, b, da, db; };

__device__ __forceinline__ RodCoef rod_coef(float t) {
    RodCoef c;
    if (t < kMSeries) {
        c.a = 1.f + t * (-1.f / 6.f + t * (1.f / 120.f + t * (-1.f / 5040.f + t * (1.f / 362880.f))));
        c.b = 0.5f + t * (-1.f / 24.f + t * (1.f / 720.f + t * (-1.f / 40320.f + t * (1.f / 3628800.f))));
        c.da = -1.f / 6.f + t * (1.f / 60.f + t * (-1.f / 1680.f + t * (1.f / 90720.f)));
        c.db = -1.f / 24.f + t * (1.f / 360.f + t * (-1.f / 13440.f + t * (1.f / 907200.f)));
    } else {
        const float th = sqrtf(t);
        float s, co;
        sincosf(th, &s, &co);
        const float sh = sinf(0.5f * th);
        c.a = s / th;
        c.b = 2.f * sh * sh / t;
        c.da = (co - c.a) / (2.f * t);
        c.db = (c.a - 2.f * c.b) / (2.f * t);
    }
    return c;
}

// M = R - I = a S(r) + b (r r^T - t I), row-major
__device__ __forceinline__ void rod_minus_identity(const float r[3], float M[9]) {
    const float x = r[0], y = r[1], z = r[2];
    const float t = x * x + y * y + z * z;
    const RodCoef c = rod_coef(t);
    M[0] = c.b * (x * x - t);
    M[1] = c.b * x * y - c.a * z;
    M[2] = c.b * x * z + c.a * y;
    M[3] = c.b * x * y + c.a * z;
    M[4] = c.b * (y * y - t);
    M[5] = c.b * y * z - c.a * x;
    M[6] = c.b * x * z - c.a * y;
    M[7] = c.b * y * z + c.a * x;
    M[8] = c.b * (z * z - t);
}

// dr = (dR/dr)^T dR for R = I + a(t) S(r) + b(t) (r r^T - t I)
__device__ __forceinline__ void rod_bwd(const float r[3], const float dR[9], float dr[3]) {
    const float t = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    const RodCoef c = rod_coef(t);
    const float w[3] = {dR[7] - dR[5], dR[2] - dR[6], dR[3] - dR[1]};     // <dR, S(e_m)>
    const float tr = dR[0] + dR[4] + dR[8];
    float Mr[3], rMr = 0.f;                                               // (dR + dR^T) r and r^T dR r
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int n = 0; n < 3; ++n) {
            s += (dR[3 * m + n] + dR[3 * n + m]) * r[n];
            q += dR[3 * m + n] * r[n];
        }
        Mr[m] = s;
        rMr += r[m] * q;
    }
    const float qa = r[0] * w[0] + r[1] * w[1] + r[2] * w[2];             // <dR, S(r)>
    const float qb = rMr - t * tr;                                        // <dR, r r^T - t I>
    const float dt = qa * c.da + qb * c.db;
#pragma unroll
    for (int m = 0; m < 3; ++m) dr[m] = c.a * w[m] + c.b * (Mr[m] - 2.f * r[m] * tr) + 2.f * r[m] * dt;
}

__device__ __forceinline__ float mano_wave_sum(float v) {
    // xor butterfly: a + b and b + a are the same bits, so every lane ends with the same value
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// C = A B, C = A^T B, C = A B^T (3x3 row-major); y = A x, y = A^T x
__device__ __forceinline__ void mm(const float* A, const float* B, float* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
__device__ __forceinline__ void mtm(const float* A, const float* B, float* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
__device__ __forceinline__ void mmt(const float* A, const float* B, float* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            C[3 * i + j] = A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1] + A[3 * i + 2] * B[3 * j + 2];
}
__device__ __forceinline__ void mv(const float* A, const float* x, float* y) {
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2];
}
__device__ __forceinline__ void mtv(const float* A, const float* x, float* y) {
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = A[i] * x[0] + A[3 + i] * x[1] + A[6 + i] * x[2];
}

// Everything a vertex needs, into LDS.  Called by all threads of the workgroup (it holds barriers); b is the sample.
static __device__ void mano_setup(ManoPose& s, const ManoArgs& p, int64_t b) {
    const int tid = threadIdx.x;
    if (tid < kMJ) {   // wavefront 0: the chain's rotations
        float r[3] = {0.f, 0.f, 0.f}, M[9];
        if (tid > 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) r[c] = p.hands_mean[3 * (tid - 1) + c] + p.poses[b * 45 + 3 * (tid - 1) + c];
        }
        rod_minus_identity(r, M);
#pragma unroll
        for (int c = 0; c < 3; ++c) s.r[tid][c] = r[c];
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            s.R[tid][e] = M[e] + ((e & 3) == 0 ? 1.f : 0.f);
            if (tid > 0) s.coef[kMBeta + 9 * (tid - 1) + e] = M[e];
        }
    } else if (tid == 64) {   // wavefront 1: the global rotation
        float r[3], M[9];
#pragma unroll
        for (int c = 0; c < 3; ++c) s.rg[c] = r[c] = p.rots[b * 3 + c];
        rod_minus_identity(r, M);
#pragma unroll
        for (int e = 0; e < 9; ++e) s.Rg[e] = M[e] + ((e & 3) == 0 ? 1.f : 0.f);
    } else if (tid >= 128 && tid < 128 + 3 * kMJ) {   // wavefront 2: the folded joints
        const int q = tid - 128;
        float j = 0.f;   // the shape terms among themselves first, then onto the template
#pragma unroll
        for (int k = 0; k < kMBeta; ++k) j += p.joint_s[q * kMBeta + k] * p.betas[b * kMBeta + k];
        s.J[q / 3][q % 3] = p.joint_t[q] + j;
    } else if (tid >= 192 && tid < 192 + kMBeta) {
        s.coef[tid - 192] = p.betas[b * kMBeta + (tid - 192)];
    }
    const int depth = tid < kMJ ? mano_depth(p.parents, tid) : -1;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) s.RG[0][e] = s.R[0][e];
#pragma unroll
        for (int c = 0; c < 3; ++c) s.t[0][c] = s.J[0][c];
    }
    for (int l = 1; l <= p.levels; ++l) {
        __syncthreads();
        if (depth == l) {
            const int pa = mano_parent(p.parents, tid);
            float RGp[9], Ri[9], RGi[9], d[3], t[3];
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                RGp[e] = s.RG[pa][e];
                Ri[e] = s.R[tid][e];
            }
            mm(RGp, Ri, RGi);
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = s.J[tid][c] - s.J[pa][c];
            mv(RGp, d, t);
#pragma unroll
            for (int e = 0; e < 9; ++e) s.RG[tid][e] = RGi[e];
#pragma unroll
            for (int c = 0; c < 3; ++c) s.t[tid][c] = t[c] + s.t[pa][c];
        }
    }
    __syncthreads();
    if (tid < kMJ) {
        float RGi[9], J[3], y[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) RGi[e] = s.RG[tid][e];
#pragma unroll
        for (int c = 0; c < 3; ++c) J[c] = s.J[tid][c];
        mv(RGi, J, y);
#pragma unroll
        for (int c = 0; c < 3; ++c) s.a[tid][c] = s.t[tid][c] - y[c];
    }
    __syncthreads();
}

// v_posed of vertex v, its blended transform T (rotation, 9) and the skinned point relative to the root, d = v' - t_1
__device__ __forceinline__ void mano_vertex(const ManoPose& s, const ManoArgs& p, int v, float vp[3], float T[9], float d[3]) {
    const int V = p.V;
    const float* bl = p.blend + v;
    // five partial sums of 29 terms each, the template added last: the terms are a tenth of the template or less, and
    // added to it one by one each would round at the template's magnitude
    float acc[kMBlendGroup][3];
#pragma unroll
    for (int q = 0; q < kMBlendGroup; ++q)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[q][c] = 0.f;
    for (int k0 = 0; k0 < kMCoef; k0 += kMBlendGroup) {
#pragma unroll
        for (int q = 0; q < kMBlendGroup; ++q) {
            const float ck = s.coef[k0 + q];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[q][c] += ck * bl[((1 + k0 + q) * 3 + c) * V];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) vp[c] = bl[c * V] + (((acc[0][c] + acc[1][c]) + (acc[2][c] + acc[3][c])) + acc[4][c]);
    float Ta[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 9; ++e) T[e] = 0.f;
#pragma unroll 4
    for (int i = 0; i < kMJ; ++i) {
        const float w = p.weights_t[i * V + v];
#pragma unroll
        for (int e = 0; e < 9; ++e) T[e] += w * s.RG[i][e];
#pragma unroll
        for (int c = 0; c < 3; ++c) Ta[c] += w * s.a[i][c];
    }
    float x[3];
    mv(T, vp, x);
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = (x[c] + Ta[c]) - s.t[1][c];
}

// host: the by-value tree and tips; returns the depth of the deepest joint through *levels
static int mano_validate(const char* fn, const void* const* ptrs, int nptr, int B, int V, uint64_t parents, const int tips[5],
                         int* levels) {
    uintptr_t all = 0;
    for (int i = 0; i < nptr; ++i) {
        SCAT_REQUIRE(ptrs[i], SCAT_E_ARG, "%s: null pointer", fn);
        all |= (uintptr_t)ptrs[i];
    }
    SCAT_REQUIRE((all & 3) == 0, SCAT_E_ARG, "%s: fp32 operands must be 4-byte aligned", fn);
    SCAT_REQUIRE(B > 0, SCAT_E_SHAPE, "%s: batch %d must be positive", fn, B);
    SCAT_REQUIRE(V >= 1 && V <= kMMaxV, SCAT_E_SHAPE, "%s: %d vertices outside 1..%d", fn, V, kMMaxV);
    SCAT_REQUIRE((parents & 15u) == 0, SCAT_E_ARG, "%s: parent[0] = %d, the root must be joint 0 with parent 0", fn,
                 (int)(parents & 15u));
    int depth[kMJ] = {0}, deepest = 0;
    for (int i = 1; i < kMJ; ++i) {
        const int pa = (int)((parents >> (4 * i)) & 15u);
        SCAT_REQUIRE(pa < i, SCAT_E_ARG, "%s: parent[%d] = %d must be less than %d", fn, i, pa, i);
        depth[i] = depth[pa] + 1;
        if (depth[i] > deepest) deepest = depth[i];
    }
    for (int j = 0; j < kMTips; ++j)
        SCAT_REQUIRE(tips[j] >= 0 && tips[j] < V, SCAT_E_SHAPE, "%s: tip %d = %d outside 0..%d", fn, j, tips[j], V - 1);
    *levels = deepest;
    return SCAT_OK;
}

}  // namespace scat
