// On-device evaluation (eval.py:788-1053): the blank-frame rule and the per-batch scores, include/scat_eval.h.
//
// scat_eval_frame_mask, two launches:
//   frame_sum_kernel     one HBM pass over x[B,n]: a workgroup sums one 8192-float chunk of one row in fp64;
//   frame_keep_kernel    a thread per row adds its chunk sums in ascending order and applies eval.py:818.
//   Sample 0 is always kept: the reference's idx_lst filter (eval.py:819-821) compares idxs[i] * i with i, and a dropped
//   sample's product 0 equals the index of sample 0 — the quirk is kept on purpose.
// scat_eval_accumulate, two launches:
//   eval_sample_kernel   one wavefront per sample, lanes 0..20 hold a joint: distances, the similarity alignment (Horn's
//                        quaternion, eval_solve.h, replicated on every lane), the 2-D error, the PCK counts on lanes 0..T-1;
//   eval_fold_kernel     one workgroup folds the per-sample rows into the record: integer counts, and the three sums
//                        serially in ascending sample order, which makes the row independent of the grid and of timing.
//   The kernel boundary is the hand-off between the two: no counter, no fence, nothing to go stale between XCDs.
#include "common.h"

#include "../../include/scat_eval.h"
#include "eval_solve.h"

namespace scat {

// ---------------------------------------------------------------- frame mask

constexpr int kSumThreads = 256;
constexpr int kSumVecs = 8;                                   // float4 loads in flight per thread
constexpr int64_t kChunkVecs = (int64_t)kSumThreads * kSumVecs;   // 2048 float4 = 8192 floats = 32 KB per workgroup

typedef float ev4f_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double wave_sum(double v) {
    // xor butterfly: a + b and b + a are the same bits, so every lane ends with the same value
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// chunks of a row of n floats at address p: the scalar head up to the first 16-byte boundary, the float4 body, the tail
__host__ __device__ __forceinline__ int64_t row_head(uintptr_t p, int64_t n) {
    const int64_t h = (int64_t)(((16 - (p & 15)) & 15) >> 2);
    return h < n ? h : n;
}

// grid = B * nchunk, block = 256
__global__ __launch_bounds__(kSumThreads) void frame_sum_kernel(const float* __restrict__ x, double* __restrict__ part,
                                                                int64_t n, int nchunk) {
    const int b = blockIdx.x / nchunk, c = blockIdx.x - b * nchunk;
    const float* row = x + (int64_t)b * n;
    const int64_t head = row_head((uintptr_t)row, n);
    const int64_t nv = (n - head) >> 2;
    const float* body = row + head;
    const int64_t v0 = (int64_t)c * kChunkVecs;
    const int64_t v1 = v0 + kChunkVecs < nv ? v0 + kChunkVecs : nv;

    // streamed once and not read again before the caches turn over: non-temporal, as the BatchNorm passes read x
    ev4f_t v[kSumVecs];
#pragma unroll
    for (int k = 0; k < kSumVecs; ++k) {
        const int64_t i = v0 + (int64_t)k * kSumThreads + threadIdx.x;
        v[k] = i < v1 ? __builtin_nontemporal_load((const ev4f_t*)(body + 4 * i)) : ev4f_t{0.f, 0.f, 0.f, 0.f};
    }
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < kSumVecs; ++k) acc += ((double)v[k][0] + (double)v[k][1]) + ((double)v[k][2] + (double)v[k][3]);
    acc = wave_sum(acc);

    __shared__ double sw[kSumThreads / 64];
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = (sw[0] + sw[1]) + (sw[2] + sw[3]);
        if (c == 0) {   // the row's unaligned ends ride with its first chunk: at most 3 + 3 floats
            for (int64_t i = 0; i < head; ++i) s += (double)row[i];
            for (int64_t i = head + 4 * nv; i < n; ++i) s += (double)row[i];
        }
        part[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void frame_keep_kernel(const double* __restrict__ part, uint8_t* __restrict__ keep, int B,
                                                         int nchunk, double blank_sum, double tol) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s += part[(int64_t)b * nchunk + c];
    keep[b] = (b == 0 || fabs(fabs(s) - blank_sum) > tol) ? 1 : 0;
}

static int frame_chunks(int64_t n) {
    // the largest body a row can have is n floats (an aligned row); one chunk at least, for the head and tail
    const int64_t c = (n / 4 + kChunkVecs - 1) / kChunkVecs;
    return (int)(c < 1 ? 1 : c);
}

// ---------------------------------------------------------------- scores

constexpr int kJoints = 21;
constexpr int kWaves = 4;   // samples per workgroup
constexpr int kRecHead = 8;

__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN

// workspace: rows[B][4] doubles (mpjpe, pa_mpjpe, err2d, flag), then cnt[B][2T] bytes (raw, aligned)
// grid = ceil(B / 4), block = 256: wavefront w of a workgroup owns sample 4 blockIdx + w
__global__ __launch_bounds__(64 * kWaves) void eval_sample_kernel(const float* __restrict__ out, const float* __restrict__ gt3d,
                                                                   const float* __restrict__ gt2d, int ld,
                                                                   const uint8_t* __restrict__ keep,
                                                                   const float* __restrict__ th, int T,
                                                                   double* __restrict__ rows, uint8_t* __restrict__ cnt,
                                                                   double* __restrict__ per_sample,
                                                                   float* __restrict__ aligned, int B) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * kWaves + wave;
    if (b >= B) return;   // wave-uniform; no workgroup barrier below
    const bool act = lane < kJoints;
    const int j = act ? lane : 0;

    int flag = (keep && keep[b] == 0) ? 1 : 0;
    double mpjpe = 0.0, pa = 0.0, e2d = 0.0, d_raw = 0.0, d_pa = 0.0;
    double ax = 0.0, ay = 0.0, az = 0.0;
    if (!flag) {
        const float* o = out + (int64_t)b * 66;
        const float* g3 = gt3d + (int64_t)b * ld;
        const float* g2 = gt2d + (int64_t)b * ld;
        const double cs = o[0], ctx = o[1], cty = o[2];
        const double px = o[3 + 3 * j], py = o[4 + 3 * j], pz = o[5 + 3 * j];
        const double gx = g3[3 * j], gy = g3[3 * j + 1], gz = g3[3 * j + 2];
        const double ux = g2[2 * j], uy = g2[2 * j + 1];
        const bool fin = finite64(cs) && finite64(ctx) && finite64(cty) && finite64(px) && finite64(py) && finite64(pz) &&
                         finite64(gx) && finite64(gy) && finite64(gz) && finite64(ux) && finite64(uy);
        if (__any(!fin)) {
            flag = 2;
        } else {
            const double m = act ? 1.0 : 0.0;
            const double nj = kJoints;     // sums are divided, not scaled: 21 equal fp32 values then average to themselves
            // raw distance, mm
            const double dx = px - gx, dy = py - gy, dz = pz - gz;
            d_raw = 1000.0 * sqrt(dx * dx + dy * dy + dz * dz);
            mpjpe = wave_sum(m * d_raw) / nj;
            // 2-D error, pixels (eval.py:467-475)
            const double qx = (cs * (px + ctx)) * 112.0 + 112.0 - ux, qy = (cs * (py + cty)) * 112.0 + 112.0 - uy;
            e2d = wave_sum(m * sqrt(qx * qx + qy * qy)) / nj;
            // similarity alignment (eval.py:110-161)
            const double m1x = wave_sum(m * px) / nj, m1y = wave_sum(m * py) / nj, m1z = wave_sum(m * pz) / nj;
            const double m2x = wave_sum(m * gx) / nj, m2y = wave_sum(m * gy) / nj, m2z = wave_sum(m * gz) / nj;
            const double x1 = m * (px - m1x), y1 = m * (py - m1y), z1 = m * (pz - m1z);
            const double x2 = gx - m2x, y2 = gy - m2y, z2 = gz - m2z;
            const double var1 = wave_sum(x1 * x1 + y1 * y1 + z1 * z1);
            double K[9], R[9];
            K[0] = wave_sum(x1 * x2);
            K[1] = wave_sum(x1 * y2);
            K[2] = wave_sum(x1 * z2);
            K[3] = wave_sum(y1 * x2);
            K[4] = wave_sum(y1 * y2);
            K[5] = wave_sum(y1 * z2);
            K[6] = wave_sum(z1 * x2);
            K[7] = wave_sum(z1 * y2);
            K[8] = wave_sum(z1 * z2);
            if (var1 == 0.0) {
                flag = 2;
            } else {
                horn_rotation(K, R);
                // tr(R K)
                const double tr = R[0] * K[0] + R[1] * K[3] + R[2] * K[6] + R[3] * K[1] + R[4] * K[4] + R[5] * K[7] +
                                  R[6] * K[2] + R[7] * K[5] + R[8] * K[8];
                const double sc = tr / var1;
                const double tx = m2x - sc * (R[0] * m1x + R[1] * m1y + R[2] * m1z);
                const double ty = m2y - sc * (R[3] * m1x + R[4] * m1y + R[5] * m1z);
                const double tz = m2z - sc * (R[6] * m1x + R[7] * m1y + R[8] * m1z);
                ax = sc * (R[0] * px + R[1] * py + R[2] * pz) + tx;
                ay = sc * (R[3] * px + R[4] * py + R[5] * pz) + ty;
                az = sc * (R[6] * px + R[7] * py + R[8] * pz) + tz;
                const double ex = ax - gx, ey = ay - gy, ez = az - gz;
                d_pa = 1000.0 * sqrt(ex * ex + ey * ey + ez * ez);
                pa = wave_sum(m * d_pa) / nj;
                if (!(finite64(mpjpe) && finite64(pa) && finite64(e2d))) flag = 2;   // not reached by finite fp32 inputs
            }
        }
    }
    if (flag) mpjpe = pa = e2d = ax = ay = az = 0.0;

    // PCK counts: lane t < T counts the 21 distances against threshold t (every lane takes part in the shuffles)
    {
        const double t = (!flag && lane < T) ? (double)th[lane] : 0.0;
        int n0 = 0, n1 = 0;
#pragma unroll
        for (int k = 0; k < kJoints; ++k) {
            n0 += __shfl(d_raw, k, 64) <= t ? 1 : 0;
            n1 += __shfl(d_pa, k, 64) <= t ? 1 : 0;
        }
        if (lane < T) {
            cnt[(int64_t)b * 2 * T + lane] = (uint8_t)(flag ? 0 : n0);
            cnt[(int64_t)b * 2 * T + T + lane] = (uint8_t)(flag ? 0 : n1);
        }
    }
    if (lane == 0) {
        double* r = rows + (int64_t)b * 4;
        r[0] = mpjpe;
        r[1] = pa;
        r[2] = e2d;
        r[3] = (double)flag;
        if (per_sample) {
            double* q = per_sample + (int64_t)b * 4;
            q[0] = mpjpe;
            q[1] = pa;
            q[2] = e2d;
            q[3] = (double)flag;
        }
    }
    if (aligned && act) {
        float* a = aligned + (int64_t)b * 63 + 3 * lane;
        a[0] = (float)ax;
        a[1] = (float)ay;
        a[2] = (float)az;
    }
}

// grid = 1, block = 192: threads 0..2T-1 a count column each, 128..130 one sum each, 131 the frame counts
__global__ __launch_bounds__(192) void eval_fold_kernel(const double* __restrict__ rows, const uint8_t* __restrict__ cnt,
                                                        double* __restrict__ record, int B, int T) {
    const int t = threadIdx.x;
    if (t < 2 * T) {
        int64_t n = 0;   // rows that are not kept hold zero counts
        for (int b = 0; b < B; ++b) n += cnt[(int64_t)b * 2 * T + t];
        record[kRecHead + t] = (double)n;
    } else if (t >= 128 && t < 131) {
        const int col = t - 128;
        double s = 0.0;   // ascending sample order, kept samples only
        for (int b = 0; b < B; ++b)
            if (rows[(int64_t)b * 4 + 3] == 0.0) s += rows[(int64_t)b * 4 + col];
        record[4 + col] = s;
    } else if (t == 131) {
        int64_t n[3] = {0, 0, 0};
        for (int b = 0; b < B; ++b) {
            const int f = (int)rows[(int64_t)b * 4 + 3];
            n[0] += f == 0;
            n[1] += f == 1;
            n[2] += f == 2;
        }
        record[0] = (double)B;
        record[1] = (double)n[0];
        record[2] = (double)n[1];
        record[3] = (double)n[2];
        record[7] = 0.0;
    }
}

}  // namespace scat

using namespace scat;

extern "C" int64_t scat_eval_frame_mask_ws(int B, int64_t n) {
    if (B <= 0 || n <= 0) return 0;
    return (int64_t)B * frame_chunks(n) * (int64_t)sizeof(double);
}

extern "C" int scat_eval_frame_mask(const float* x, uint8_t* keep, int B, int64_t n, float blank_sum, float tol, void* ws,
                                    int64_t ws_bytes, void* stream) {
    SCAT_REQUIRE(x && keep && ws, SCAT_E_ARG, "scat_eval_frame_mask: null pointer");
    SCAT_REQUIRE(B > 0, SCAT_E_SHAPE, "scat_eval_frame_mask: batch %d must be positive", B);
    SCAT_REQUIRE(n > 0 && n < (1ll << 40), SCAT_E_SHAPE, "scat_eval_frame_mask: row length %lld outside 1..2^40", (long long)n);
    SCAT_REQUIRE(((uintptr_t)x & 3) == 0, SCAT_E_ARG, "scat_eval_frame_mask: x must be 4-byte aligned");
    SCAT_REQUIRE(tol >= 0.f, SCAT_E_ARG, "scat_eval_frame_mask: tol must not be negative");
    const int nchunk = frame_chunks(n);
    SCAT_REQUIRE(fits_i32((int64_t)B * nchunk), SCAT_E_SHAPE, "scat_eval_frame_mask: %d rows of %d chunks exceed the grid", B,
                 nchunk);
    SCAT_REQUIRE(((uintptr_t)ws & 7) == 0, SCAT_E_ARG, "scat_eval_frame_mask: ws must be 8-byte aligned");
    SCAT_REQUIRE(ws_bytes >= scat_eval_frame_mask_ws(B, n), SCAT_E_WORKSPACE,
                 "scat_eval_frame_mask: workspace %lld < %lld bytes", (long long)ws_bytes,
                 (long long)scat_eval_frame_mask_ws(B, n));
    double* part = (double*)ws;
    hipLaunchKernelGGL(frame_sum_kernel, dim3(B * nchunk), dim3(kSumThreads), 0, (hipStream_t)stream, x, part, n, nchunk);
    SCAT_LAUNCH_CHECK("scat_eval_frame_mask");
    hipLaunchKernelGGL(frame_keep_kernel, dim3(cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, part, keep, B, nchunk,
                       (double)blank_sum, (double)tol);
    SCAT_LAUNCH_CHECK("scat_eval_frame_mask");
    set_kernel_label("eval_frame_mask_c%d", nchunk);
    return SCAT_OK;
}

extern "C" int64_t scat_eval_accumulate_ws(int B, int T) {
    if (B <= 0 || T < 1 || T > 64) return 0;
    return (int64_t)B * 4 * (int64_t)sizeof(double) + (((int64_t)B * 2 * T + 7) & ~7ll);
}

extern "C" int scat_eval_accumulate(const float* out, const float* gt3d, const float* gt2d, int ld_gt, const uint8_t* keep,
                                    const float* thresholds_mm, int T, double* record, double* per_sample, float* aligned,
                                    int B, void* ws, int64_t ws_bytes, void* stream) {
    SCAT_REQUIRE(out && gt3d && gt2d && thresholds_mm && record && ws, SCAT_E_ARG, "scat_eval_accumulate: null pointer");
    SCAT_REQUIRE(B > 0, SCAT_E_SHAPE, "scat_eval_accumulate: batch %d must be positive", B);
    SCAT_REQUIRE(T >= 1 && T <= 64, SCAT_E_SHAPE, "scat_eval_accumulate: %d thresholds outside 1..64", T);
    SCAT_REQUIRE(ld_gt >= 63, SCAT_E_SHAPE, "scat_eval_accumulate: ld_gt %d < 63", ld_gt);
    SCAT_REQUIRE(((uintptr_t)record & 7) == 0 && ((uintptr_t)per_sample & 7) == 0, SCAT_E_ARG,
                 "scat_eval_accumulate: record and per_sample must be 8-byte aligned");
    SCAT_REQUIRE((((uintptr_t)out | (uintptr_t)gt3d | (uintptr_t)gt2d | (uintptr_t)thresholds_mm | (uintptr_t)aligned) & 3) == 0,
                 SCAT_E_ARG, "scat_eval_accumulate: fp32 operands must be 4-byte aligned");
    SCAT_REQUIRE(((uintptr_t)ws & 7) == 0, SCAT_E_ARG, "scat_eval_accumulate: ws must be 8-byte aligned");
    SCAT_REQUIRE(ws_bytes >= scat_eval_accumulate_ws(B, T), SCAT_E_WORKSPACE,
                 "scat_eval_accumulate: workspace %lld < %lld bytes", (long long)ws_bytes,
                 (long long)scat_eval_accumulate_ws(B, T));
    double* rows = (double*)ws;
    uint8_t* cnt = (uint8_t*)(rows + (int64_t)B * 4);
    hipLaunchKernelGGL(eval_sample_kernel, dim3(cdiv(B, kWaves)), dim3(64 * kWaves), 0, (hipStream_t)stream, out, gt3d, gt2d,
                       ld_gt, keep, thresholds_mm, T, rows, cnt, per_sample, aligned, B);
    SCAT_LAUNCH_CHECK("scat_eval_accumulate");
    hipLaunchKernelGGL(eval_fold_kernel, dim3(1), dim3(192), 0, (hipStream_t)stream, (const double*)rows, (const uint8_t*)cnt,
                       record, B, T);
    SCAT_LAUNCH_CHECK("scat_eval_accumulate");
    set_kernel_label("eval_accumulate_t%d", T);
    return SCAT_OK;
}
