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
#include "mano_common.h"

namespace scat {

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
