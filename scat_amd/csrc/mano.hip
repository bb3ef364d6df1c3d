// On-device MANO layer (models/mano.py:280-391): joints and mesh from rots / poses / betas, forward and backward,
// include/scat_mano.h.  One workgroup of 1024 threads per sample in both directions; threads loop over vertices.
//
// Both kernels start with mano_setup, which leaves in LDS what every vertex needs:
//   Rodrigues of the 16 chain rotations and of rots (one lane each), the 145 blend coefficients (beta, then R_k - I),
//   the folded joint positions J = joint_t + joint_s . beta, the chain G_i = G_parent(i) . [R_i | J_i - J_parent(i)] level
//   by level (lane i waits for its depth: 4 levels for MANO's tree), and a_i = t_i - R^G_i J_i.
// mano_fwd_kernel: per vertex the 145-term blend (lanes read consecutive v of blend[k][c][:]: coalesced dwords; the
//   coefficient and the A_i are LDS broadcasts, one address per wave-instruction, so no bank conflict), the skinning, the
//   global rotation and the root subtraction; the root t_1 is known after the chain, so there is no second pass.
// mano_bwd_kernel: phase 1 repeats the forward per vertex and leaves g = Rg^T dy, v_posed and d v_posed in LDS
//   (vertex-minor: lane l reads bank l); phase 2 gives each wavefront whole sums — joint i's 12 or five blend
//   coefficients — over all vertices (lane l takes v = l, l + 64, ...; then an xor butterfly, which gives every lane
//   the same bits); phase 3 walks the chain in reverse level by level (a child lane computes what it hands its parent,
//   the parent lane adds its children in ascending order) and ends in the Rodrigues derivative.
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
__device__ void mano_setup(ManoPose& s, const ManoArgs& p, int64_t b) {
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

// grid = B, block = 1024
__global__ __launch_bounds__(kMThreads) void mano_fwd_kernel(ManoArgs p, float* __restrict__ out) {
    __shared__ ManoPose s;
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, V = p.V;
    mano_setup(s, p, b);
    float* o = out + b * (int64_t)(21 + V) * 3;
    float Rg[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) Rg[e] = s.Rg[e];
    if (tid < kMJ) {
        float d[3], y[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = s.t[tid][c] - s.t[1][c];
        mv(Rg, d, y);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[3 * tid + c] = y[c];
    }
    for (int v = tid; v < V; v += kMThreads) {
        float vp[3], T[9], d[3], y[3];
        mano_vertex(s, p, v, vp, T, d);
        mv(Rg, d, y);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[3 * (21 + v) + c] = y[c];
#pragma unroll
        for (int j = 0; j < kMTips; ++j)
            if (p.tips.v[j] == v) {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[3 * (kMJ + j) + c] = y[c];
            }
    }
}

struct ManoBwdLds {
    float g[3][kMMaxV];        // Rg^T dy per vertex (tips carry their joint's dy too)
    float vp[3][kMMaxV];       // v_posed
    float dvp[3][kMMaxV];      // T_R^T g
    float part[kMWaves][12];   // per-wavefront partials: d Rg (9), sum of g (3)
    float jc[kMJ][12];         // the 16 chain joints' share of the same 12
    float tot[12];
    float dA[kMJ][12];         // d RG_i from the skinning (9), d a_i (3)
    float dcoef[kMCoef];
    float dRG[kMJ][9];
    float dt[kMJ][3];
    float dJ[kMJ][3];
    float dR[kMJ][9];
    float cRG[kMJ][9];         // what child i hands its parent's d RG
    float cu[kMJ][3];          // RG_parent^T dt_i
};

// grid = B, block = 1024
__global__ __launch_bounds__(kMThreads) void mano_bwd_kernel(ManoArgs p, const float* __restrict__ dout,
                                                             float* __restrict__ drots, float* __restrict__ dposes,
                                                             float* __restrict__ dbetas) {
    __shared__ ManoPose s;
    __shared__ ManoBwdLds m;
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, V = p.V, wave = tid >> 6, lane = tid & 63;
    mano_setup(s, p, b);
    const float* dy = dout + b * (int64_t)(21 + V) * 3;
    float Rg[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) Rg[e] = s.Rg[e];

    // ---- phase 1: per vertex
    float acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.f;
    for (int v = tid; v < V; v += kMThreads) {
        float vp[3], T[9], d[3], dyt[3], g[3], dvp[3];
        mano_vertex(s, p, v, vp, T, d);
#pragma unroll
        for (int c = 0; c < 3; ++c) dyt[c] = dy[3 * (21 + v) + c];
#pragma unroll
        for (int j = 0; j < kMTips; ++j)
            if (p.tips.v[j] == v) {
#pragma unroll
                for (int c = 0; c < 3; ++c) dyt[c] += dy[3 * (kMJ + j) + c];
            }
        mtv(Rg, dyt, g);
        mtv(T, g, dvp);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[3 * r + c] += dyt[r] * d[c];
            acc[9 + r] += g[r];
            m.g[r][v] = g[r];
            m.vp[r][v] = vp[r];
            m.dvp[r][v] = dvp[r];
        }
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        const float t = mano_wave_sum(acc[q]);
        if (lane == 0) m.part[wave][q] = t;
    }
    // the 16 chain joints: y_i = Rg (t_i - t_1)
    if (tid < kMJ) {
        float d[3], dyj[3], g[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            d[c] = s.t[tid][c] - s.t[1][c];
            dyj[c] = dy[3 * tid + c];
        }
        mtv(Rg, dyj, g);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) m.jc[tid][3 * r + c] = dyj[r] * d[c];
            m.jc[tid][9 + r] = g[r];
        }
    }
    __syncthreads();

    // ---- phase 2: whole sums per wavefront
    for (int u = wave; u < kMUnits; u += kMWaves) {
        if (u < kMJ) {   // joint u: d RG_u[r][c] = sum_v w g_r vp_c, d a_u[r] = sum_v w g_r
            float a12[12];
#pragma unroll
            for (int q = 0; q < 12; ++q) a12[q] = 0.f;
            for (int v = lane; v < V; v += 64) {
                const float w = p.weights_t[u * V + v];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float wg = w * m.g[r][v];
#pragma unroll
                    for (int c = 0; c < 3; ++c) a12[3 * r + c] += wg * m.vp[c][v];
                    a12[9 + r] += wg;
                }
            }
#pragma unroll
            for (int q = 0; q < 12; ++q) {
                const float t = mano_wave_sum(a12[q]);
                if (lane == 0) m.dA[u][q] = t;
            }
        } else {         // five blend coefficients: d coef[k] = sum_v sum_c blend[1 + k][c][v] dvp[c][v]
            const int k0 = (u - kMJ) * kMBlendGroup;
            float a5[kMBlendGroup];
#pragma unroll
            for (int q = 0; q < kMBlendGroup; ++q) a5[q] = 0.f;
            for (int v = lane; v < V; v += 64) {
                const float d0 = m.dvp[0][v], d1 = m.dvp[1][v], d2 = m.dvp[2][v];
                const float* bl = p.blend + v;
#pragma unroll
                for (int q = 0; q < kMBlendGroup; ++q) {
                    const int row = (1 + k0 + q) * 3;
                    a5[q] += bl[row * V] * d0 + bl[(row + 1) * V] * d1 + bl[(row + 2) * V] * d2;
                }
            }
#pragma unroll
            for (int q = 0; q < kMBlendGroup; ++q) {
                const float t = mano_wave_sum(a5[q]);
                if (lane == 0) m.dcoef[k0 + q] = t;
            }
        }
    }
    if (tid < 12) {   // part and jc were complete at the barrier above
        float t = 0.f;
        for (int w = 0; w < kMWaves; ++w) t += m.part[w][tid];
        for (int i = 0; i < kMJ; ++i) t += m.jc[i][tid];
        m.tot[tid] = t;
    }
    __syncthreads();

    // ---- phase 3: the chain in reverse
    const int depth = tid < kMJ ? mano_depth(p.parents, tid) : -1;
    if (tid < kMJ) {
        // a_i = t_i - RG_i J_i;  joint i's own output;  the root t_1 is subtracted from every output
        float RGi[9], da[3], u[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) RGi[e] = s.RG[tid][e];
#pragma unroll
        for (int c = 0; c < 3; ++c) da[c] = m.dA[tid][9 + c];
        mtv(RGi, da, u);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) m.dRG[tid][3 * r + c] = m.dA[tid][3 * r + c] - da[r] * s.J[tid][c];
            m.dJ[tid][r] = -u[r];
            m.dt[tid][r] = da[r] + m.jc[tid][9 + r] - (tid == 1 ? m.tot[9 + r] : 0.f);
        }
    }
    for (int l = p.levels; l >= 1; --l) {
        __syncthreads();
        if (depth == l) {   // a child: d RG_i and dt_i are final
            const int pa = mano_parent(p.parents, tid);
            float RGp[9], Ri[9], dRGi[9], dRi[9], cR[9], dti[3], u[3], dj[3];
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                RGp[e] = s.RG[pa][e];
                Ri[e] = s.R[tid][e];
                dRGi[e] = m.dRG[tid][e];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                dti[c] = m.dt[tid][c];
                dj[c] = s.J[tid][c] - s.J[pa][c];
            }
            mtm(RGp, dRGi, dRi);     // RG_i = RG_p R_i
            mmt(dRGi, Ri, cR);
            mtv(RGp, dti, u);        // t_i = RG_p (J_i - J_p) + t_p
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    m.dR[tid][3 * r + c] = dRi[3 * r + c];
                    m.cRG[tid][3 * r + c] = cR[3 * r + c] + dti[r] * dj[c];
                }
                m.cu[tid][r] = u[r];
                m.dJ[tid][r] += u[r];
            }
        }
        __syncthreads();
        if (depth == l - 1) {   // a parent: its children in ascending order
            for (int c = tid + 1; c < kMJ; ++c) {
                if (mano_parent(p.parents, c) != tid) continue;
#pragma unroll
                for (int e = 0; e < 9; ++e) m.dRG[tid][e] += m.cRG[c][e];
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    m.dt[tid][e] += m.dt[c][e];
                    m.dJ[tid][e] -= m.cu[c][e];
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {   // t_0 = J_0; R_0 is the identity, a constant
#pragma unroll
        for (int c = 0; c < 3; ++c) m.dJ[0][c] += m.dt[0][c];
    }
    __syncthreads();

    if (tid >= 1 && tid < kMJ) {   // pose k: through the chain and through pw = R_k - I
        float r[3], dR[9], dr[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = s.r[tid][c];
#pragma unroll
        for (int e = 0; e < 9; ++e) dR[e] = m.dR[tid][e] + m.dcoef[kMBeta + 9 * (tid - 1) + e];
        rod_bwd(r, dR, dr);
#pragma unroll
        for (int c = 0; c < 3; ++c) dposes[b * 45 + 3 * (tid - 1) + c] = dr[c];
    } else if (tid == 64) {
        float r[3], dR[9], dr[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = s.rg[c];
#pragma unroll
        for (int e = 0; e < 9; ++e) dR[e] = m.tot[e];
        rod_bwd(r, dR, dr);
#pragma unroll
        for (int c = 0; c < 3; ++c) drots[b * 3 + c] = dr[c];
    } else if (tid >= 128 && tid < 128 + kMBeta) {   // beta k: through v_shaped and through the joints
        const int k = tid - 128;
        float t = m.dcoef[k];
        for (int q = 0; q < 3 * kMJ; ++q) t += p.joint_s[q * kMBeta + k] * m.dJ[q / 3][q % 3];
        dbetas[b * kMBeta + k] = t;
    }
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

using namespace scat;

extern "C" int scat_mano_fwd(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                             const float* hands_mean, const float* rots, const float* poses, const float* betas, float* out,
                             int B, int V, uint64_t parents, int tip0, int tip1, int tip2, int tip3, int tip4, void* stream) {
    const void* ptrs[] = {blend, joint_t, joint_s, weights_t, hands_mean, rots, poses, betas, out};
    const int tips[kMTips] = {tip0, tip1, tip2, tip3, tip4};
    ManoArgs p = {blend, joint_t, joint_s, weights_t, hands_mean, rots, poses, betas, V, 0, parents, {{tip0, tip1, tip2, tip3, tip4}}};
    const int rc = mano_validate("scat_mano_fwd", ptrs, 9, B, V, parents, tips, &p.levels);
    if (rc != SCAT_OK) return rc;
    hipLaunchKernelGGL(mano_fwd_kernel, dim3(B), dim3(kMThreads), 0, (hipStream_t)stream, p, out);
    SCAT_LAUNCH_CHECK("scat_mano_fwd");
    set_kernel_label("mano_fwd_v%d", V);
    return SCAT_OK;
}

extern "C" int scat_mano_bwd(const float* blend, const float* joint_t, const float* joint_s, const float* weights_t,
                             const float* hands_mean, const float* rots, const float* poses, const float* betas,
                             const float* dout, float* drots, float* dposes, float* dbetas, int B, int V, uint64_t parents,
                             int tip0, int tip1, int tip2, int tip3, int tip4, void* stream) {
    const void* ptrs[] = {blend, joint_t, joint_s, weights_t, hands_mean, rots, poses, betas, dout, drots, dposes, dbetas};
    const int tips[kMTips] = {tip0, tip1, tip2, tip3, tip4};
    ManoArgs p = {blend, joint_t, joint_s, weights_t, hands_mean, rots, poses, betas, V, 0, parents, {{tip0, tip1, tip2, tip3, tip4}}};
    const int rc = mano_validate("scat_mano_bwd", ptrs, 12, B, V, parents, tips, &p.levels);
    if (rc != SCAT_OK) return rc;
    hipLaunchKernelGGL(mano_bwd_kernel, dim3(B), dim3(kMThreads), 0, (hipStream_t)stream, p, (const float*)dout, drots, dposes,
                       dbetas);
    SCAT_LAUNCH_CHECK("scat_mano_bwd");
    set_kernel_label("mano_bwd_v%d", V);
    return SCAT_OK;
}
