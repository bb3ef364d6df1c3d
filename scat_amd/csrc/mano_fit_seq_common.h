// What a track is, for the two kernels that walk one (mano_fit_seq.hip: 62 unknowns per frame; mano_fit_seq_kp.hip: 65):
// the workspace's layout, the cost's running sums, the staging of the unknowns, the block-tridiagonal elimination forward
// and backward, the accept step with the buffer swap, the refusal and the write-out, and the entry points' checks of T,
// the smoothness weights and the workspace.  Everything is a template on the number of unknowns U and on the kernel's LDS
// state F, as lm_factor<N, F> is: F has J and M[U][U] in a union (J is dead once A_t and g_t stand), A[U + 1][U], col,
// delta, p, pp, pn, yp, xn, dc, ds, cost, lambda, cd, cs, acc, fail, fin, cur.  What a frame is stays in each kernel.
// The damped normal matrix is block-tridiagonal, H_t (U x U) on the diagonal and -D beside it, D the smoothness weights
// of the free unknowns (f.ds); include/scat_mano_fit_seq.h has the recurrences that factor it frame by frame.
#pragma once
#include "mano_fit_common.h"

#include "../../include/scat_mano_fit_seq.h"

namespace scat {

constexpr int kSeqMaxT = SCAT_FIT_SEQ_MAX_T;
static_assert(kSeqMaxT <= kFThreads, "the start gives every frame a thread");

// The workspace of a sequence: L_t with y_t as row U for every frame, then M_t^T for every frame (t >= 1 is used), then
// the unknowns, two buffers of [T][U].  It is touched by the sequence's own workgroup only.
template <int U> constexpr int kSeqL = (U + 1) * U;
template <int U> constexpr int kSeqM = U * U;
template <int U> constexpr int kSeqFrame = kSeqL<U> + kSeqM<U> + 2 * U;   // floats per frame: 7874 at 62, 8645 at 65

template <int U>
__device__ __forceinline__ float* seq_ws_l(float* ws, int64_t s, int T) { return ws + s * ((int64_t)T * kSeqFrame<U>); }
template <int U> __device__ __forceinline__ float* seq_ws_m(float* wl, int T) { return wl + (int64_t)T * kSeqL<U>; }
template <int U> __device__ __forceinline__ float* seq_ws_p(float* wm, int T) { return wm + (int64_t)T * kSeqM<U>; }
// frame t of the first buffer of the unknowns, where a start kernel leaves the frame's start
template <int U>
__device__ __forceinline__ float* seq_ws_start(float* ws, int64_t s, int T, int t) {
    return seq_ws_p<U>(seq_ws_m<U>(seq_ws_l<U>(ws, s, T), T), T) + t * U;
}

// one thread: frame t's terms of the cost onto the running sums: its data term, which the kernel's own fit_cost / kp_cost
// gave, and its smoothness, q the frame's unknowns and qp those of the frame before
template <int U, class F>
__device__ __forceinline__ void seq_cost_add(F& f, float data, const float* q, const float* qp, int t) {
    f.cd += data;
    if (t > 0) {
        float cs = f.cs;
        for (int i = 0; i < U; ++i) {
            const float e = q[i] - qp[i];
            cs += f.dc[i] * (e * e);
        }
        f.cs = cs;
    }
}

// threads base .. base + U - 1: from the buffer P the unknowns of frames t - 1, t, t + 1 into pp, q, pn
template <int U, class F>
__device__ __forceinline__ void seq_stage_unknowns(F& f, const float* P, float* q, int t, int T, int base) {
    const int i = (int)threadIdx.x - base;
    if (i >= 0 && i < U) {
        q[i] = P[t * U + i];
        f.pp[i] = t > 0 ? P[(t - 1) * U + i] : 0.f;
        f.pn[i] = t < T - 1 ? P[(t + 1) * U + i] : 0.f;
    }
}

// All threads, with A_t and g_t (row U) in f.A: eliminate the frame before, factor, and prepare the frame after.
//   rank update   M_t^T, which the frame before left in the workspace, into the LDS that J occupied; H_t -= M_t M_t^T over
//                 the lower triangle, g_t -= M_t y_t-1
//   factor        lm_factor: g rides along as row U and ends as y_t; L_t with y_t to the workspace, y_t to yp
//   M_t+1^T       = -L_t^-1 D: one thread per column, which it alone writes and reads back, so no barrier; lower
//                 triangular as L^-1 is, which the rank update and seq_backward use; to the workspace.  Ends with a barrier
template <int U, class F>
__device__ __forceinline__ void seq_eliminate(F& f, float* wl, float* wm, int t, int T) {
    const int tid = threadIdx.x;
    if (t > 0) {
        const float* mt = wm + (int64_t)t * kSeqM<U>;
        for (int i = tid; i < kSeqM<U>; i += kFThreads) (&f.M[0][0])[i] = mt[i];
        __syncthreads();
        // M^T[k][i] = 0 for i > k
        for (int w = tid; w < (U + 1) * U; w += kFThreads) {
            const int ai = w / U, bi = w % U;
            if (ai == U) {
                float sum = 0.f;
                for (int k = bi; k < U; ++k) sum += f.M[k][bi] * f.yp[k];
                f.A[U][bi] -= sum;
            } else if (bi <= ai) {
                float sum = 0.f;
                for (int k = ai; k < U; ++k) sum += f.M[k][ai] * f.M[k][bi];
                f.A[ai][bi] -= sum;
            }
        }
        __syncthreads();
    }
    lm_factor<U>(f);
    {
        float* lt = wl + (int64_t)t * kSeqL<U>;
        for (int i = tid; i < kSeqL<U>; i += kFThreads) lt[i] = (&f.A[0][0])[i];
    }
    if (tid < U) f.yp[tid] = f.A[U][tid];
    if (t < T - 1) {
        if (tid < U) {   // column tid
            const float d = f.ds[tid];
            for (int k = 0; k < U; ++k) {
                float sum = k == tid ? -d : 0.f;
                for (int j = 0; j < k; ++j) sum -= f.A[k][j] * f.M[j][tid];
                f.M[k][tid] = sum / f.A[k][k];
            }
        }
        __syncthreads();
        float* mt = wm + (int64_t)(t + 1) * kSeqM<U>;
        for (int i = tid; i < kSeqM<U>; i += kFThreads) mt[i] = (&f.M[0][0])[i];
    }
    __syncthreads();
}

// All threads, t descending: L_t and the current unknowns of frame t back into LDS, x_t = L_t^-T (y_t - M_t+1^T x_t+1) by
// lm_backsub, x_t to xn for the frame before, and the trial unknowns of frame t to Q.  free: this thread's unknown
// (tid < U) is not frozen.  Ends with a barrier.
template <int U, class F>
__device__ __forceinline__ void seq_backward(F& f, const float* wl, const float* wm, const float* P, float* Q, int t, int T,
                                             bool free) {
    const int tid = threadIdx.x;
    const float* lt = wl + (int64_t)t * kSeqL<U>;
    for (int i = tid; i < kSeqL<U>; i += kFThreads) (&f.A[0][0])[i] = lt[i];
    if (tid < U) f.p[tid] = P[t * U + tid];
    __syncthreads();
    if (t < T - 1 && tid < U) {
        const float* mt = wm + (int64_t)(t + 1) * kSeqM<U> + tid * U;
        float sum = 0.f;
        for (int i = 0; i <= tid; ++i) sum += mt[i] * f.xn[i];
        f.A[U][tid] -= sum;
    }
    __syncthreads();
    lm_backsub<U>(f);
    if (tid < U) {
        f.xn[tid] = -f.delta[tid];
        Q[t * U + tid] = free ? f.p[tid] + f.delta[tid] : f.p[tid];
    }
    __syncthreads();
}

// One thread, after the trial's walk: the step is taken if every pivot was positive and finite, every trial unknown is
// finite and the cost drops; then the two buffers of the unknowns swap roles, where lm_commit copies pt
template <class F>
__device__ __forceinline__ void seq_decide(F& f) {
    const float c = f.cd + f.cs;
    const bool ok = !f.fail && f.fin && c < f.cost;
    lm_decide(f, ok, c);
    if (ok) f.cur ^= 1;
}

// All threads: the results of sequence s when it is not fitted.  With init = 1 its p is the refused start: zeros, and 1
// at the unknown one_at of every frame (none: -1)
template <int U, class A>
__device__ __forceinline__ void seq_refuse(const A& a, int64_t s, float* pg, int np, int one_at) {
    const int tid = threadIdx.x;
    if (a.init)
        for (int i = tid; i < np; i += kFThreads) pg[i] = i % U == one_at ? 1.f : 0.f;
    if (tid == 0) {
        a.cost[s] = INFINITY;
        a.accepted[s] = 0;
    }
}

// All threads, after a barrier: the results of sequence s, wp the two buffers of its unknowns.  A sequence without an
// accepted step keeps the caller's p
template <class F, class A>
__device__ __forceinline__ void seq_write(const F& f, const A& a, int64_t s, const float* wp, float* pg, int np) {
    const int tid = threadIdx.x;
    if (a.init || f.acc > 0) {
        const float* P = wp + f.cur * np;
        for (int i = tid; i < np; i += kFThreads) pg[i] = P[i];
    }
    if (tid == 0) {
        a.cost[s] = fit_finite(f.cost) ? f.cost : INFINITY;   // also NaN: a start that is not finite
        a.accepted[s] = f.acc;
    }
}

}  // namespace scat

// The workspace query of a track's entry point: 0 for sizes the launch refuses
template <int U>
static int64_t seq_ws_bytes(int S, int T) {
    if (S < 1 || T < 1 || T > scat::kSeqMaxT) return 0;
    return (int64_t)S * T * scat::kSeqFrame<U> * (int64_t)sizeof(float);
}

// The checks that the tracks' entry points share, each text in one place, in the style of fit_check_*
static int seq_check_frames(const char* fn, int T) {
    SCAT_REQUIRE(T >= 1 && T <= scat::kSeqMaxT, SCAT_E_SHAPE, "%s: %d frames outside 1..%d", fn, T, scat::kSeqMaxT);
    return SCAT_OK;
}

static int seq_check_smooth(const char* fn, const float* sw, const char* const* names, int n) {
    for (int i = 0; i < n; ++i)
        SCAT_REQUIRE(sw[i] >= 0.f && sw[i] < INFINITY, SCAT_E_ARG, "%s: %s %g must be finite and not negative", fn, names[i],
                     (double)sw[i]);
    return SCAT_OK;
}

static int seq_check_ws(const char* fn, const void* ws, int64_t ws_bytes, int64_t need) {
    SCAT_REQUIRE(ws && ((uintptr_t)ws & 15) == 0, SCAT_E_WORKSPACE, "%s: the workspace must be a 16-byte-aligned pointer", fn);
    SCAT_REQUIRE(ws_bytes >= need, SCAT_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn, (long long)ws_bytes,
                 (long long)need);
    return SCAT_OK;
}
