// Convolution weight-gradient: dW[Cout][Cin*KH*KW] = dY[Cout][pixels] * im2col(X)[pixels][Cin*KH*KW],
// contraction over B*OH*OW pixels, deterministic two-stage split-K (slabs + fixed-order sum).
#include "conv_common.h"

namespace scat {

// out[e] (+)= sum_z slab[z][e]: 8 independent loads in flight per thread, combined in a fixed order
__global__ void splitk_reduce_kernel(const float* __restrict__ slab, float* __restrict__ out, int64_t n, int splits,
                                     int accumulate) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        float s = accumulate ? out[e] : 0.f;
        int z = 0;
        for (; z + 8 <= splits; z += 8) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = slab[(int64_t)(z + q) * n + e];
            s += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
        }
        for (; z < splits; ++z) s += slab[(int64_t)z * n + e];
        out[e] = s;
    }
}

// The same sum for n % 4 == 0, 16 bytes per lane.  A workgroup owns 256 consecutive elements; its WAVES wavefronts
// take consecutive ranges of the slabs (a small output with hundreds of slabs — layer1's 64x64 — would otherwise be a
// few wavefronts walking the whole stack at one memory latency per 8 slabs) and their partial sums are combined
// through LDS in wavefront order: the result depends on (splits, WAVES) only, never on timing.
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void splitk_reduce4_kernel(const float4* __restrict__ slab,
                                                                    float4* __restrict__ out, int64_t n4, int splits,
                                                                    int accumulate) {
    __shared__ float4 part[WAVES > 1 ? WAVES : 1][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t e = blockIdx.x * 64ll + lane;
    const bool live = e < n4;
    const int per = (splits + WAVES - 1) / WAVES;
    const int z0 = wave * per, z1 = min(z0 + per, splits);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
        int z = z0;
        for (; z + 8 <= z1; z += 8) {
            float4 v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = slab[(int64_t)(z + q) * n4 + e];
            s.x += ((v[0].x + v[1].x) + (v[2].x + v[3].x)) + ((v[4].x + v[5].x) + (v[6].x + v[7].x));
            s.y += ((v[0].y + v[1].y) + (v[2].y + v[3].y)) + ((v[4].y + v[5].y) + (v[6].y + v[7].y));
            s.z += ((v[0].z + v[1].z) + (v[2].z + v[3].z)) + ((v[4].z + v[5].z) + (v[6].z + v[7].z));
            s.w += ((v[0].w + v[1].w) + (v[2].w + v[3].w)) + ((v[4].w + v[5].w) + (v[6].w + v[7].w));
        }
        for (; z < z1; ++z) {
            const float4 v = slab[(int64_t)z * n4 + e];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    if constexpr (WAVES > 1) {
        part[wave][lane] = s;
        __syncthreads();
        if (wave != 0) return;
        s = part[0][lane];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            const float4 v = part[w][lane];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    if (!live) return;
    if (accumulate) {
        const float4 o = out[e];
        s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
    }
    out[e] = s;
}

void launch_splitk_reduce(const float* slab, float* out, int64_t n, int splits, int accumulate, hipStream_t st) {
    static const int vec = diag_env_int("SCAT_REDUCE_VEC", 1);
    if (vec && n % 4 == 0 && (((uintptr_t)slab | (uintptr_t)out) & 15) == 0) {
        const int64_t n4 = n / 4;
        const dim3 grid((unsigned)((n4 + 63) / 64));
        const float4* s4 = (const float4*)slab;
        float4* o4 = (float4*)out;
        // enough wavefronts to cover the chip (~2048) before giving a wavefront more than 8 slabs
        const int64_t waves1 = (n4 + 63) / 64;
        if (splits >= 64 && waves1 < 512)
            hipLaunchKernelGGL(splitk_reduce4_kernel<16>, grid, dim3(1024), 0, st, s4, o4, n4, splits, accumulate);
        else if (splits >= 16 && waves1 < 2048)
            hipLaunchKernelGGL(splitk_reduce4_kernel<4>, grid, dim3(256), 0, st, s4, o4, n4, splits, accumulate);
        else
            hipLaunchKernelGGL(splitk_reduce4_kernel<1>, grid, dim3(64), 0, st, s4, o4, n4, splits, accumulate);
        return;
    }
    const int blocks = (int)((n + 63) / 64 < 4096 ? (n + 63) / 64 : 4096);
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks), dim3(64), 0, st, slab, out, n, splits, accumulate);
}

static int wgrad_splits(int M, int N, int K, int bm, int bn) {
    int tiles = cdiv(M, bm) * cdiv(N, bn);
    static const int target = diag_env_int("SCAT_WG_F32_TARGET", 1024);
    int s = cdiv(target, tiles);                     // aim for ~4 workgroups per CU
    int smax = K / 512 > 0 ? K / 512 : 1;            // keep >= 512 contraction steps per slice
    if (s > smax) s = smax;
    if (s > 256) s = 256;
    return s < 1 ? 1 : s;
}

struct WgradPlan {
    int M, N, K, bm, bn, splits;
};
static WgradPlan wgrad_plan(int B, int Cin, int Cout, int KK, int OH, int OW) {
    WgradPlan p;
    p.M = Cout;
    p.N = Cin * KK;
    p.K = B * OH * OW;
    p.bm = Cout <= 64 ? 64 : 128;
    p.bn = 64;
    p.splits = wgrad_splits(p.M, p.N, p.K, p.bm, p.bn);
    return p;
}

template <int KH, int KW, bool AV4, bool BV4, bool TF>
static void wgrad_gemm_tf(const WgradPlan& p, const GatherDesc& da, const GatherDesc& db, const OutDesc& dc,
                          hipStream_t st) {
    set_kernel_label("wgrad%dx%d_%dx64x32%s%s%s_split%d", KH, KW, p.bm, AV4 ? "_a4" : "", BV4 ? "_b4" : "",
                     TF ? "_tf" : "", p.splits);
    if (p.bm == 64)
        launch_gemm<GatherLoader<64, 32, 1, 1, false, true, AV4, false>,
                    GatherLoader<64, 32, KH, KW, false, true, BV4, TF>, 64, 64, 32, 2, 2>(da, db, dc, p.M, p.N, p.K,
                                                                                          p.splits, st);
    else
        launch_gemm<GatherLoader<128, 32, 1, 1, false, true, AV4, false>,
                    GatherLoader<64, 32, KH, KW, false, true, BV4, TF>, 128, 64, 32, 2, 2>(da, db, dc, p.M, p.N, p.K,
                                                                                           p.splits, st);
}

template <int KH, int KW, bool AV4, bool BV4>
static void wgrad_gemm(const WgradPlan& p, const GatherDesc& da, const GatherDesc& db, const OutDesc& dc,
                       hipStream_t st) {
    if constexpr (KH != 7) {
        if (db.scale) {
            wgrad_gemm_tf<KH, KW, AV4, BV4, true>(p, da, db, dc, st);
            return;
        }
    }
    wgrad_gemm_tf<KH, KW, AV4, BV4, false>(p, da, db, dc, st);
}

// measured at batch 96: the split kernel wins or ties everywhere it applies (tiny outputs with huge contractions —
// ResNet layer1's 64x64 1x1, HRNet's 32-channel 3x3 — are staging-bound on both engines; SCAT_WG_MINMN sets a floor
// on Cout*Cin*k*k below which the fp32 engine is used instead)
static bool wgrad_split_ok(int KH, int stride, int pad, int Cout, int Cin) {
    // (1x1/stride 2: the strided 8-dword gather makes the split kernel staging-bound, 315-380 us vs 240-250 us)
    static const int64_t minmn = diag_env_int("SCAT_WG_MINMN", 0ll);
    return ((KH == 1 && pad == 0 && stride == 1) || (KH == 3 && pad == 1)) && (int64_t)Cout * Cin * KH * KH > minmn;
}

// fp32 gather engine: any geometry check_geom admits, either product mode, any alignment
static void wgrad_f32_launch(const WgradPlan& p, const float* dy, const float* x, float* out, int B, int Cin, int H, int W,
                             int Cout, int KH, int stride, int pad, int OH, int OW, const float* in_scale,
                             const float* in_shift, int in_relu, hipStream_t st) {
    const int npix = B * OH * OW;
    // A: dy as [Cout][pixel]; B: x through the forward conv arithmetic as [pixel][(ci,kh,kw)]
    GatherDesc da{dy, nullptr, nullptr, 0, Cout, OH, OW, OH, OW, 1, 0, 0, 0, npix, Cout, FastDiv::make(OH * OW),
                  FastDiv::make(OW), (int64_t)B * Cout * OH * OW};
    GatherDesc db{x, in_scale, in_shift, in_relu, Cin, H, W, OH, OW, stride, 1, -pad, -pad, npix, Cin * KH * KH,
                  FastDiv::make(OH * OW), FastDiv::make(OW), (int64_t)B * Cin * H * W};
    OutDesc dc{};
    dc.p = out;
    dc.mode = 0; dc.si = p.N; dc.sj = 1; dc.sz = (int64_t)p.M * p.N; dc.I = p.M; dc.J = p.N; dc.n = (int64_t)p.M * p.N;
    const bool av4 = (OH * OW) % 4 == 0 && ((uintptr_t)dy & 15) == 0;
    const bool bv4 = KH <= 3 && stride == 1 && OH == H && OW == W && (H * W) % 4 == 0 && W >= 4 &&
                     ((uintptr_t)x & 15) == 0;
    if (KH == 1) {
        if (av4 && bv4) wgrad_gemm<1, 1, true, true>(p, da, db, dc, st);
        else if (av4) wgrad_gemm<1, 1, true, false>(p, da, db, dc, st);
        else wgrad_gemm<1, 1, false, false>(p, da, db, dc, st);
    } else if (KH == 3) {
        if (av4 && bv4) wgrad_gemm<3, 3, true, true>(p, da, db, dc, st);
        else if (av4) wgrad_gemm<3, 3, true, false>(p, da, db, dc, st);
        else wgrad_gemm<3, 3, false, false>(p, da, db, dc, st);
    } else {
        if (av4) wgrad_gemm<7, 7, true, false>(p, da, db, dc, st);
        else wgrad_gemm<7, 7, false, false>(p, da, db, dc, st);
    }
}

// ---- one plan for the workspace query and the launch
// wgrad_candidates() is the only place that names the engines of a weight gradient: it yields those the geometry
// admits, in priority order, each with its plan and the run-time conditions under which a launch may take it.  The _ws
// queries return the largest slab need over the candidates, the entry points launch the first candidate whose conditions
// hold — so a query cannot promise less than its launch writes, whatever the math mode and the pointers turn out to be.
enum WgEngine { WG_ROWS, WG_PW, WG_SPLIT, WG_F32 };

struct WgGeom {
    int B, Cin, H, W, Cout, KH, stride, pad, OH, OW;
    bool bnb;   // folded BatchNorm backward (scat_conv1x1_wgrad_bnb): 1x1 / stride 1 over H = 1, W = pixels per image
};

struct WgCand {
    WgEngine eng;
    int splits;       // slabs of Cout x Cin*KH*KH floats the engine writes ...
    bool slabs;       // ... into the workspace, reduced into dw afterwards; false: one split, straight into dw
    bool split_math;  // takes the call only in product mode 1,
    bool aligned;     // only with dy, x (and z) on 16-byte boundaries,
    bool i32;         // only while both tensors stay within 32-bit byte offsets
    WgPwPlan pw;      // the plan of eng (the rows engine plans inside its launch)
    WgSplitPlan sp;
    WgradPlan f32;
};

static int64_t wg_slab_bytes(const WgGeom& g, const WgCand& c) {
    return c.slabs ? (int64_t)c.splits * g.Cout * g.Cin * g.KH * g.KH * sizeof(float) : 0;
}

static int wgrad_candidates(const WgGeom& g, WgCand c[4]) {
    int n = 0;
    if (!g.bnb && wgrad_rows_ok(g.B, g.Cin, g.H, g.W, g.Cout, g.KH, g.stride, g.pad, nullptr, nullptr)) {
        c[n] = WgCand{WG_ROWS, wgrad_rows_splits(g.B, g.Cin, g.H, g.W, g.Cout), true, true, true, true};   // always slabs
        ++n;
    }
    if (g.KH == 1 && g.stride == 1 && g.pad == 0) {
        const WgPwPlan w = wgrad_pw_plan(g.B, g.Cin, g.Cout, g.H * g.W, g.bnb, nullptr, nullptr);
        if (w.ok) {
            c[n] = WgCand{WG_PW, w.splits, w.splits > 1, true, true, true};
            c[n++].pw = w;
        }
    }
    if (g.bnb || wgrad_split_ok(g.KH, g.stride, g.pad, g.Cout, g.Cin)) {
        const WgSplitPlan q = wgrad_split_plan(g.B, g.Cin, g.Cout, g.KH * g.KH, g.OH * g.OW);
        c[n] = WgCand{WG_SPLIT, q.splits, q.splits > 1, true, false, false};
        c[n++].sp = q;
    }
    if (!g.bnb) {       // (the folded form has split products only: its entry point insists on product mode 1)
        const WgradPlan p = wgrad_plan(g.B, g.Cin, g.Cout, g.KH * g.KH, g.OH, g.OW);
        c[n] = WgCand{WG_F32, p.splits, p.splits > 1, false, false, false};
        c[n++].f32 = p;
    }
    return n;
}

static int64_t wgrad_ws_bytes(const WgGeom& g) {
    WgCand c[4];
    const int n = wgrad_candidates(g, c);
    int64_t need = 0;
    for (int i = 0; i < n; ++i)
        if (wg_slab_bytes(g, c[i]) > need) need = wg_slab_bytes(g, c[i]);
    return need;
}

// dy2 / coef3: the folded BatchNorm backward's second tensor and coefficients (g.bnb), else null
static int wgrad_run(const char* who, const WgGeom& g, const float* dy, const float* dy2, const float* coef3,
                     const float* x, float* dw, const float* in_scale, const float* in_shift, int in_relu, void* ws,
                     int64_t ws_bytes, hipStream_t st) {
    WgCand c[4];
    const int n = wgrad_candidates(g, c);
    const bool split_math = math_mode() == 1;
    const bool aligned = (((uintptr_t)dy | (uintptr_t)dy2 | (uintptr_t)x) & 15) == 0;
    const bool i32 = fits_i32((int64_t)g.B * g.Cout * g.H * g.W * 4) && fits_i32((int64_t)g.B * g.Cin * g.H * g.W * 4);
    const WgCand* e = nullptr;
    for (int i = 0; i < n && !e; ++i)
        if ((split_math || !c[i].split_math) && (aligned || !c[i].aligned) && (i32 || !c[i].i32)) e = &c[i];
    SCAT_REQUIRE(e, SCAT_E_ARG, "%s: no engine takes this call", who);
    const int64_t need = wg_slab_bytes(g, *e);
    SCAT_REQUIRE(ws_bytes >= need && (need == 0 || ws), SCAT_E_WORKSPACE, "%s: workspace %lld < %lld bytes", who,
                 (long long)ws_bytes, (long long)need);
    SCAT_REQUIRE(need == 0 || ((uintptr_t)ws & 3) == 0, SCAT_E_WORKSPACE, "%s: workspace not 4-byte aligned", who);
    float* out = e->slabs ? (float*)ws : dw;
    if (!in_scale) in_relu = 0;
    const char* tag = "";
    switch (e->eng) {
    case WG_ROWS:
        tag = "(rows)";
        wgrad_rows_launch(dy, x, out, g.B, g.Cin, g.H, g.W, g.Cout, in_scale, in_shift, in_relu, st);
        break;
    case WG_PW:
        tag = "(pw)";
        wgrad_pw_launch(e->pw, dy, x, out, g.B, g.Cin, g.H * g.W, g.Cout, in_scale, in_shift, in_relu, st, dy2, coef3);
        break;
    case WG_SPLIT:
        wgrad_split_launch(e->sp, dy, x, out, g.B, g.Cin, g.H, g.W, g.Cout, g.KH * g.KH, g.stride, in_scale, in_shift,
                           in_relu, st, dy2, coef3);
        break;
    case WG_F32:
        wgrad_f32_launch(e->f32, dy, x, out, g.B, g.Cin, g.H, g.W, g.Cout, g.KH, g.stride, g.pad, g.OH, g.OW, in_scale,
                         in_shift, in_relu, st);
        break;
    }
    char name[64];      // (composed only when a check fails)
    SCAT_LAUNCH_CHECK((snprintf(name, sizeof name, "%s%s", who, tag), name));
    if (e->slabs) {
        launch_splitk_reduce((const float*)ws, dw, (int64_t)g.Cout * g.Cin * g.KH * g.KH, e->splits, 0, st);
        SCAT_LAUNCH_CHECK((snprintf(name, sizeof name, "%s(reduce)", who), name));
    }
    return SCAT_OK;
}

static WgGeom wg_geom_bnb(int B, int Cin, int HW, int Cout) { return WgGeom{B, Cin, 1, HW, Cout, 1, 1, 0, 1, HW, true}; }

}  // namespace scat

using namespace scat;

extern "C" int64_t scat_conv2d_wgrad_ws(int B, int Cin, int H, int W, int Cout, int KH, int KW, int stride, int pad) {
    int OH, OW;
    if (check_geom("scat_conv2d_wgrad_ws", B, Cin, H, W, Cout, KH, KW, stride, pad, &OH, &OW)) return -1;
    return wgrad_ws_bytes(WgGeom{B, Cin, H, W, Cout, KH, stride, pad, OH, OW, false});
}

extern "C" int scat_conv2d_wgrad(const float* dy, const float* x, float* dw, int B, int Cin, int H, int W, int Cout,
                                 int KH, int KW, int stride, int pad, const float* in_scale, const float* in_shift,
                                 int in_relu, void* ws, int64_t ws_bytes, void* stream) {
    int OH, OW;
    if (int e = check_geom("scat_conv2d_wgrad", B, Cin, H, W, Cout, KH, KW, stride, pad, &OH, &OW)) return e;
    SCAT_REQUIRE(dy && x && dw, SCAT_E_ARG, "scat_conv2d_wgrad: null pointer");
    SCAT_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), SCAT_E_ARG, "scat_conv2d_wgrad: scale/shift pair");
    SCAT_REQUIRE(!(in_scale && KH == 7), SCAT_E_SHAPE, "scat_conv2d_wgrad: fused input transform not built for 7x7");
    return wgrad_run("scat_conv2d_wgrad", WgGeom{B, Cin, H, W, Cout, KH, stride, pad, OH, OW, false}, dy, nullptr, nullptr,
                     x, dw, in_scale, in_shift, in_relu, ws, ws_bytes, (hipStream_t)stream);
}

// Weight gradient of a 1x1/stride-1 convolution from a BatchNorm backward that was never materialised:
// dy = ca*g + cb*z + cc per output channel (see scat_bn_bwd_pre / scat_conv1x1_s1_bnb).  Split products only.
extern "C" int64_t scat_conv1x1_wgrad_bnb_ws(int B, int Cin, int HW, int Cout) {
    return wgrad_ws_bytes(wg_geom_bnb(B, Cin, HW, Cout));
}

extern "C" int scat_conv1x1_wgrad_bnb(const float* g, const float* z, const float* coef3, const float* x, float* dw,
                                      int B, int Cin, int HW, int Cout, const float* in_scale, const float* in_shift,
                                      int in_relu, void* ws, int64_t ws_bytes, void* stream) {
    SCAT_REQUIRE(g && z && coef3 && x && dw, SCAT_E_ARG, "scat_conv1x1_wgrad_bnb: null pointer");
    SCAT_REQUIRE(math_mode() == 1, SCAT_E_ARG, "scat_conv1x1_wgrad_bnb: needs the split-operand product mode");
    SCAT_REQUIRE(B > 0 && Cin > 0 && HW > 0 && Cout > 0, SCAT_E_SHAPE, "scat_conv1x1_wgrad_bnb: non-positive dimension");
    SCAT_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), SCAT_E_ARG, "scat_conv1x1_wgrad_bnb: scale/shift pair");
    SCAT_REQUIRE(fits_i32((int64_t)B * Cout * HW * 4) && fits_i32((int64_t)B * Cin * HW * 4), SCAT_E_SHAPE,
                 "scat_conv1x1_wgrad_bnb: tensor exceeds 32-bit byte offsets");
    return wgrad_run("scat_conv1x1_wgrad_bnb", wg_geom_bnb(B, Cin, HW, Cout), g, z, coef3, x, dw, in_scale, in_shift,
                     in_relu, ws, ws_bytes, (hipStream_t)stream);
}
