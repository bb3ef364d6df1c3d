// On-device mesh scoring, include/scat_mesh_eval.h: per-vertex error raw and after the similarity alignment of eval.hip,
// vertex PCK counts, and F-scores from exact brute-force nearest-neighbour distances in both directions.
//
// scat_mesh_eval_accumulate, two launches:
//   mesh_sample_kernel   one workgroup of 256 threads (four wavefronts) per sample.  pred and gt are staged once into LDS
//                        as separate x / y / z arrays, the aligned points join them there as doubles.  A thread keeps up to
//                        four query vertices (tid, tid + 256, ...) in registers and walks all V candidates once for all of
//                        them: every lane of a wavefront reads the same candidate address, an LDS broadcast.  Four such
//                        passes: pred -> gt, gt -> pred, aligned -> gt, gt -> aligned.  The minimum is taken over squared
//                        distances (exact, order-independent), one sqrt after it.
//   mesh_fold_kernel     one workgroup folds the per_sample rows into the record: integer counts, and the sums serially in
//                        ascending sample order, as eval_fold_kernel does.
//   The kernel boundary is the hand-off between the two, and per_sample (a required output) carries it: no workspace.
// Every floating-point reduction over vertices is a per-thread sum over v = tid, tid + 256, ... ascending, an xor shuffle
// tree inside the wavefront, and the four wave partials added in ascending order through LDS: fixed by V alone.  Counts are
// integers: a ballot and a population count per wavefront, the four wave partials added the same way.
#include "common.h"

#include "../../include/scat_mesh_eval.h"
#include "eval_solve.h"

namespace scat {

constexpr int kMaxV = SCAT_MESH_EVAL_MAX_V;
constexpr int kMaxT = SCAT_MESH_EVAL_MAX_T;
constexpr int kMaxF = SCAT_MESH_EVAL_MAX_F;
constexpr int kThreads = 256;
constexpr int kMWaves = kThreads / 64;
constexpr int kQ = kMaxV / kThreads;                  // query vertices a thread may hold
constexpr int kMaxCnt = 2 * kMaxT + 4 * kMaxF;       // count slots of a sample: 2T PCK, then n_pred / n_gt raw and aligned
constexpr int kRedMax = 10;                          // widest batch of sums reduced at once (var1 and the 9 entries of K)
constexpr int kMeshRecHead = 8;
constexpr int kMeshRowHead = 4;

static_assert(kQ == 4 && kMaxV % kThreads == 0, "a thread holds V / 256 queries");

__device__ __forceinline__ bool mesh_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

__device__ __forceinline__ double mesh_wave_sum(double v) {
    // xor butterfly: a + b and b + a are the same bits, so every lane ends with the same value
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// N sums at once: wave partials to LDS, then every thread adds the four in ascending wave order (the same bits on every
// thread, so what follows stays workgroup-uniform).  Two barriers; red is free again after the second.
template <int N>
__device__ __forceinline__ void block_sums(double (&v)[N], double (*red)[kMWaves]) {
    static_assert(N <= kRedMax, "red holds kRedMax rows");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double s = mesh_wave_sum(v[i]);
        if (lane == 0) red[i][wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = ((red[i][0] + red[i][1]) + red[i][2]) + red[i][3];
    __syncthreads();
}

// squared distance from each of NQ queries to its nearest of V candidates; the candidate address is wave-uniform
template <int NQ, typename CT>
__device__ __forceinline__ void nn_walk(const double (&qx)[kQ], const double (&qy)[kQ], const double (&qz)[kQ],
                                        const CT* __restrict__ cx, const CT* __restrict__ cy, const CT* __restrict__ cz,
                                        int V, double (&best)[kQ]) {
#pragma unroll 4
    for (int j = 0; j < V; ++j) {
        const double x = (double)cx[j], y = (double)cy[j], z = (double)cz[j];
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            const double dx = qx[k] - x, dy = qy[k] - y, dz = qz[k] - z;
            best[k] = fmin(best[k], dx * dx + dy * dy + dz * dz);
        }
    }
}

// nq: how many of this wavefront's query slots hold a vertex (wave-uniform; no barrier inside)
template <typename CT>
__device__ __forceinline__ void nn_pass(int nq, const double (&qx)[kQ], const double (&qy)[kQ], const double (&qz)[kQ],
                                        const CT* cx, const CT* cy, const CT* cz, int V, double (&best)[kQ]) {
#pragma unroll
    for (int k = 0; k < kQ; ++k) best[k] = __builtin_huge_val();
    switch (nq) {
        case 1: nn_walk<1>(qx, qy, qz, cx, cy, cz, V, best); break;
        case 2: nn_walk<2>(qx, qy, qz, cx, cy, cz, V, best); break;
        case 3: nn_walk<3>(qx, qy, qz, cx, cy, cz, V, best); break;
        case 4: nn_walk<4>(qx, qy, qz, cx, cy, cz, V, best); break;
        default: break;
    }
}

// how many of the wavefront's valid values d (mm) pass threshold t: <= for PCK, < for the F-score
template <bool kStrict>
__device__ __forceinline__ int wave_count(const double (&d)[kQ], const bool (&valid)[kQ], double t) {
    int n = 0;
#pragma unroll
    for (int k = 0; k < kQ; ++k) n += __popcll(__ballot(valid[k] && (kStrict ? d[k] < t : d[k] <= t)));
    return n;
}

// a sample that is not scored: flag and zeros in its row, zeros in its aligned vertices
__device__ __forceinline__ void mesh_empty_row(double* __restrict__ row, int W, float* __restrict__ al, int V, int flag) {
    for (int i = threadIdx.x; i < W; i += kThreads) row[i] = i == 0 ? (double)flag : 0.0;
    if (al)
        for (int i = threadIdx.x; i < 3 * V; i += kThreads) al[i] = 0.f;
}

// grid = B, block = 256.  Static LDS: 12 KiB + 12 KiB of fp32, 24 KiB of fp64, 4.8 KiB of partials.
__global__ __launch_bounds__(kThreads) void mesh_sample_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                int V, const uint8_t* __restrict__ keep,
                                                                const float* __restrict__ th, int T,
                                                                const float* __restrict__ fth, int F,
                                                                double* __restrict__ per_sample,
                                                                float* __restrict__ aligned) {
    __shared__ float sp[3][kMaxV], sg[3][kMaxV];
    __shared__ double sa[3][kMaxV];
    __shared__ double red[kRedMax][kMWaves];
    __shared__ int scnt[kMWaves][kMaxCnt];

    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int W = kMeshRowHead + 2 * T + 6 * F;
    double* row = per_sample + (int64_t)b * W;
    float* al = aligned ? aligned + (int64_t)b * 3 * V : nullptr;

    // blockIdx-uniform: the whole workgroup leaves before its first barrier, and nothing of the sample is read
    if (keep && keep[b] == 0) {
        mesh_empty_row(row, W, al, V, 1);
        return;
    }

    // stage: coalesced over the 3V floats of the sample, de-interleaved into x / y / z
    const float* p = pred + (int64_t)b * 3 * V;
    const float* g = gt + (int64_t)b * 3 * V;
    bool fin = true;
    for (int i = tid; i < 3 * V; i += kThreads) {
        const int v = i / 3, c = i - 3 * v;
        const float a = p[i], e = g[i];
        sp[c][v] = a;
        sg[c][v] = e;
        fin = fin && mesh_finite((double)a) && mesh_finite((double)e);
    }
    if (__syncthreads_or(!fin)) {   // (also the barrier that publishes sp / sg)
        mesh_empty_row(row, W, al, V, 2);
        return;
    }

    // this thread's vertices, both as the terms of the sums and as the queries of the search
    bool valid[kQ];
    double px[kQ], py[kQ], pz[kQ], gx[kQ], gy[kQ], gz[kQ], d_raw[kQ], d_pa[kQ];
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        const int v = tid + k * kThreads;
        valid[k] = v < V;
        const int u = valid[k] ? v : 0;
        px[k] = sp[0][u], py[k] = sp[1][u], pz[k] = sp[2][u];
        gx[k] = sg[0][u], gy[k] = sg[1][u], gz[k] = sg[2][u];
    }
    const int nq = V > wave * 64 ? min(kQ, (V - wave * 64 + kThreads - 1) / kThreads) : 0;
    const double nv = (double)V;   // sums are divided, not scaled: V equal values then average to themselves

    // the 6 means and the raw distance sum
    double s7[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        const double dx = px[k] - gx[k], dy = py[k] - gy[k], dz = pz[k] - gz[k];
        d_raw[k] = 1000.0 * sqrt(dx * dx + dy * dy + dz * dz);
        if (valid[k]) {
            s7[0] += px[k], s7[1] += py[k], s7[2] += pz[k];
            s7[3] += gx[k], s7[4] += gy[k], s7[5] += gz[k];
            s7[6] += d_raw[k];
        }
    }
    block_sums(s7, red);
    const double m1x = s7[0] / nv, m1y = s7[1] / nv, m1z = s7[2] / nv;
    const double m2x = s7[3] / nv, m2y = s7[4] / nv, m2z = s7[5] / nv;
    const double mpvpe = s7[6] / nv;

    // var1 and K = X1 X2^T
    double s10[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        if (valid[k]) {
            const double x1 = px[k] - m1x, y1 = py[k] - m1y, z1 = pz[k] - m1z;
            const double x2 = gx[k] - m2x, y2 = gy[k] - m2y, z2 = gz[k] - m2z;
            s10[0] += x1 * x2, s10[1] += x1 * y2, s10[2] += x1 * z2;
            s10[3] += y1 * x2, s10[4] += y1 * y2, s10[5] += y1 * z2;
            s10[6] += z1 * x2, s10[7] += z1 * y2, s10[8] += z1 * z2;
            s10[9] += x1 * x1 + y1 * y1 + z1 * z1;
        }
    }
    block_sums(s10, red);
    const double var1 = s10[9];
    if (var1 == 0.0) {   // the same bits on every thread: workgroup-uniform
        mesh_empty_row(row, W, al, V, 2);
        return;
    }
    double R[9];
    horn_rotation(s10, R);
    const double tr = R[0] * s10[0] + R[1] * s10[3] + R[2] * s10[6] + R[3] * s10[1] + R[4] * s10[4] + R[5] * s10[7] +
                      R[6] * s10[2] + R[7] * s10[5] + R[8] * s10[8];
    const double sc = tr / var1;
    const double tx = m2x - sc * (R[0] * m1x + R[1] * m1y + R[2] * m1z);
    const double ty = m2y - sc * (R[3] * m1x + R[4] * m1y + R[5] * m1z);
    const double tz = m2z - sc * (R[6] * m1x + R[7] * m1y + R[8] * m1z);

    // the aligned points: kept in registers as queries, published in LDS as candidates
    double ax[kQ], ay[kQ], az[kQ];
    double s1[1] = {0};
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        ax[k] = sc * (R[0] * px[k] + R[1] * py[k] + R[2] * pz[k]) + tx;
        ay[k] = sc * (R[3] * px[k] + R[4] * py[k] + R[5] * pz[k]) + ty;
        az[k] = sc * (R[6] * px[k] + R[7] * py[k] + R[8] * pz[k]) + tz;
        const double ex = ax[k] - gx[k], ey = ay[k] - gy[k], ez = az[k] - gz[k];
        d_pa[k] = 1000.0 * sqrt(ex * ex + ey * ey + ez * ez);
        if (valid[k]) {
            const int v = tid + k * kThreads;
            sa[0][v] = ax[k], sa[1][v] = ay[k], sa[2][v] = az[k];
            s1[0] += d_pa[k];
        }
    }
    block_sums(s1, red);   // (its barriers also publish sa)
    const double pa = s1[0] / nv;
    if (!(mesh_finite(mpvpe) && mesh_finite(pa))) {   // not reached by finite fp32 inputs
        mesh_empty_row(row, W, al, V, 2);
        return;
    }

    // vertex PCK counts
    int* mine = scnt[wave];
    for (int t = 0; t < T; ++t) {
        const double lim = (double)th[t];
        const int n0 = wave_count<false>(d_raw, valid, lim), n1 = wave_count<false>(d_pa, valid, lim);
        if (lane == 0) mine[t] = n0, mine[T + t] = n1;
    }

    // the four searches; each leaves the nearest distance in mm of this thread's queries
    double best[kQ];
    const auto count_f = [&](int slot) {
#pragma unroll
        for (int k = 0; k < kQ; ++k) best[k] = 1000.0 * sqrt(best[k]);
        for (int f = 0; f < F; ++f) {
            const int n = wave_count<true>(best, valid, (double)fth[f]);
            if (lane == 0) mine[2 * T + slot * F + f] = n;
        }
    };
    nn_pass(nq, px, py, pz, sg[0], sg[1], sg[2], V, best);   // pred -> gt: n_pred, raw
    count_f(0);
    nn_pass(nq, gx, gy, gz, sp[0], sp[1], sp[2], V, best);   // gt -> pred: n_gt, raw
    count_f(1);
    nn_pass(nq, ax, ay, az, sg[0], sg[1], sg[2], V, best);   // aligned -> gt: n_pred, aligned
    count_f(2);
    nn_pass(nq, gx, gy, gz, sa[0], sa[1], sa[2], V, best);   // gt -> aligned: n_gt, aligned
    count_f(3);
    __syncthreads();

    // the row
    const auto total = [&](int slot) { return ((scnt[0][slot] + scnt[1][slot]) + scnt[2][slot]) + scnt[3][slot]; };
    if (tid == 0) {
        row[0] = 0.0;
        row[1] = mpvpe;
        row[2] = pa;
        row[3] = 0.0;
    }
    for (int t = tid; t < 2 * T; t += kThreads) row[kMeshRowHead + t] = (double)total(t);
    if (tid < 2 * F) {
        const int side = tid / F, f = tid - side * F;   // side 0 raw, 1 aligned
        const double np = (double)total(2 * T + (2 * side) * F + f), ng = (double)total(2 * T + (2 * side + 1) * F + f);
        double* o = row + kMeshRowHead + 2 * T + side * 3 * F + 3 * f;
        o[0] = np;
        o[1] = ng;
        o[2] = np + ng > 0.0 ? (2.0 * np * ng) / (nv * (np + ng)) : 0.0;
    }
    if (al)
        for (int i = tid; i < 3 * V; i += kThreads) {
            const int v = i / 3, c = i - 3 * v;
            al[i] = (float)sa[c][v];
        }
}

// grid = 1, block = 320: threads 0..2T-1 a count column each, 256..257+2F one sum each, 319 the frame counts
constexpr int kFoldThreads = 320;
static_assert(2 * kMaxT <= 256 && 256 + 2 + 2 * kMaxF < kFoldThreads - 1, "the fold's thread roles do not overlap");

__global__ __launch_bounds__(kFoldThreads) void mesh_fold_kernel(const double* __restrict__ rows,
                                                                 double* __restrict__ record, int B, int V, int T, int F) {
    const int t = threadIdx.x;
    const int W = kMeshRowHead + 2 * T + 6 * F;
    if (t < 2 * T) {
        int64_t n = 0;   // rows that are not kept hold zero counts
#pragma unroll 8
        for (int b = 0; b < B; ++b) n += (int64_t)rows[(int64_t)b * W + kMeshRowHead + t];
        record[kMeshRecHead + t] = (double)n;
    } else if (t >= 256 && t < 256 + 2 + 2 * F) {
        const int c = t - 256;   // mpvpe, pa_mpvpe, F raw [F], F aligned [F]
        int col, dst;
        if (c < 2) {
            col = 1 + c, dst = 4 + c;
        } else {
            const int side = (c - 2) / F, f = (c - 2) - side * F;
            col = kMeshRowHead + 2 * T + side * 3 * F + 3 * f + 2;
            dst = kMeshRecHead + 2 * T + side * F + f;
        }
        double s = 0.0;   // ascending sample order, kept samples only
#pragma unroll 8
        for (int b = 0; b < B; ++b) {
            const double flag = rows[(int64_t)b * W], v = rows[(int64_t)b * W + col];
            if (flag == 0.0) s += v;
        }
        record[dst] = s;
    } else if (t == kFoldThreads - 1) {
        int64_t n[3] = {0, 0, 0};
        for (int b = 0; b < B; ++b) {
            const int f = (int)rows[(int64_t)b * W];
            n[0] += f == 0;
            n[1] += f == 1;
            n[2] += f == 2;
        }
        record[0] = (double)B;
        record[1] = (double)n[0];
        record[2] = (double)n[1];
        record[3] = (double)n[2];
        record[6] = (double)V;
        record[7] = 0.0;
    }
}

}  // namespace scat

using namespace scat;

extern "C" int scat_mesh_eval_accumulate(const float* pred, const float* gt, int V, const uint8_t* keep,
                                         const float* thresholds_mm, int T, const float* f_thresholds_mm, int F,
                                         double* record, double* per_sample, float* aligned, int B, void* stream) {
    SCAT_REQUIRE(pred && gt && thresholds_mm && f_thresholds_mm && record && per_sample, SCAT_E_ARG,
                 "scat_mesh_eval_accumulate: null pointer");
    SCAT_REQUIRE(B > 0, SCAT_E_SHAPE, "scat_mesh_eval_accumulate: batch %d must be positive", B);
    SCAT_REQUIRE(V >= 1 && V <= kMaxV, SCAT_E_SHAPE, "scat_mesh_eval_accumulate: %d vertices outside 1..%d", V, kMaxV);
    SCAT_REQUIRE(T >= 1 && T <= kMaxT, SCAT_E_SHAPE, "scat_mesh_eval_accumulate: %d thresholds outside 1..%d", T, kMaxT);
    SCAT_REQUIRE(F >= 1 && F <= kMaxF, SCAT_E_SHAPE, "scat_mesh_eval_accumulate: %d F-score thresholds outside 1..%d", F,
                 kMaxF);
    SCAT_REQUIRE(((uintptr_t)record & 7) == 0 && ((uintptr_t)per_sample & 7) == 0, SCAT_E_ARG,
                 "scat_mesh_eval_accumulate: record and per_sample must be 8-byte aligned");
    SCAT_REQUIRE((((uintptr_t)pred | (uintptr_t)gt | (uintptr_t)thresholds_mm | (uintptr_t)f_thresholds_mm |
                   (uintptr_t)aligned) & 3) == 0,
                 SCAT_E_ARG, "scat_mesh_eval_accumulate: fp32 operands must be 4-byte aligned");
    hipLaunchKernelGGL(mesh_sample_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, pred, gt, V, keep, thresholds_mm,
                       T, f_thresholds_mm, F, per_sample, aligned);
    SCAT_LAUNCH_CHECK("scat_mesh_eval_accumulate");
    hipLaunchKernelGGL(mesh_fold_kernel, dim3(1), dim3(kFoldThreads), 0, (hipStream_t)stream, (const double*)per_sample,
                       record, B, V, T, F);
    SCAT_LAUNCH_CHECK("scat_mesh_eval_accumulate");
    set_kernel_label("mesh_eval_v%d_t%d_f%d", V, T, F);
    return SCAT_OK;
}
