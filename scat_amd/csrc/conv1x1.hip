// Pointwise (1x1, stride 1) convolution forward / data-gradient:  dst[n][m][r] = sum_c A[m][c] * f(src[n][c][r]).
//
// Same operand split as conv3x3.hip, which measured ~15 % faster than staging both operands through LDS:
//  * A (weights [M][K], K contiguous, L2-resident) goes straight from global memory to the MFMA operand
//    registers.  The contraction order inside a 16-channel sub-chunk is free, so lane (row, h) takes
//    k = 8h .. 8h+7: 32 contiguous bytes, two 16-B loads, prefetched one sub-chunk ahead.
//  * B (activations) is staged through LDS 32 channels at a time in k-pair-interleaved rows
//    [k/2][pixel][k&1]: a staging thread owns a channel PAIR x 4 pixels (two 16-B global loads -> two
//    ds_write_b128) and a lane reads its k pair with one ds_read_b64.  The fused BatchNorm+ReLU of the
//    producing layer is applied once per element on the way into LDS.
//  * one barrier per 32 channels (64 MFMAs per wave at 128x128); fragments of the second sub-chunk are
//    read while the first one computes.
//
// Replaces nn.Conv2d(k=1) and its input gradient as called at models/resnet.py:65-67,70-72,84-92 of the
// reference (conv1/conv3 of every Bottleneck) and the 1x1 reductions of models/hand_net.py, fp32.
#include "conv_common.h"
#include "split.h"

namespace scat {

struct PwDesc {
    const float* src;     // [Nimg][C][HW]
    const float* w;       // [M][C]
    const float* scale;   // optional fused input transform, per source channel
    const float* shift;
    int relu;
    int C, M, HW, npix;   // HW: source plane; npix: columns of the contraction = B * OHW
    FastDiv dHW;
    int64_t nsrc, nw;
    // split kernel only — taps: source (y, x) of column pixel (oy, ox) and tap (th, tw) is
    // (oy*a + th*tb + c0y, ox*a + tw*tb + c0x); a 1x1/stride-1 conv has ntap = 1, a = 1, OHW = HW
    int ntap, KWt, a, tb, c0y, c0x, H, W, OW, OHW;
    FastDiv dOHW, dOW;
    int variant;          // SCAT_TUNE pass-through for kernel-variant experiments
    const float* src2;    // dual-source (DS) kernels: second tensor and the [3][C] coefficient table
    const float* coef;
};

constexpr int PW_KS = 32;     // channels per LDS stage (two 16-channel sub-chunks)


template <int BM, int BN, bool V4, bool TF>
__global__ __launch_bounds__(NT, (BM * BN >= 128 * 128 ? 2 : 3)) void conv1x1_kernel(PwDesc d, OutDesc dc) {
    constexpr int MI = BM / 64, NI = BN / 64;
    constexpr int PV = V4 ? 4 : 1;                    // pixels per staging item
    constexpr int PT = BN / PV;                       // staging threads along the pixel dimension
    constexpr int NIT = 16 * PT / NT;                 // staging items (channel pair x PV pixels) per thread
    static_assert(NIT >= 1, "tile too small for 256 staging threads");
    extern __shared__ __align__(16) float lds[];      // B[2][16 k-pairs][BN][2]
    auto Bs = [&](int buf) -> float* { return lds + buf * (PW_KS * BN); };

    const int mt = (d.M + BM - 1) / BM, nt = (d.npix + BN - 1) / BN;
    const int tile = xcd_remap(blockIdx.x, mt * nt);
    const int i0 = (tile % mt) * BM, j0 = (tile / mt) * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, lh = lane >> 5;
    const int nstage = (d.C + PW_KS - 1) / PW_KS;

    // ---- activation staging: item r of this thread = channel pair p = tid/PT + r*(NT/PT), pixels (tid%PT)*PV ..
    const __amdgpu_buffer_rsrc_t rsrc_b = make_rsrc(d.src, d.nsrc);
    const __amdgpu_buffer_rsrc_t rsrc_sc = make_rsrc(TF ? d.scale : d.src, TF ? d.C : 0);
    const __amdgpu_buffer_rsrc_t rsrc_sh = make_rsrc(TF ? d.shift : d.src, TF ? d.C : 0);
    const int pcol = (tid % PT) * PV, prow = tid / PT;
    const int chw4 = d.HW * 4;
    int boff;                                          // byte offset of (n, channel 2*prow, r) or OOB
    bool bok;
    {
        const int j = j0 + pcol;
        bok = j < d.npix;
        const uint32_t jj = bok ? (uint32_t)j : 0u;
        const uint32_t n = d.dHW.div(jj);
        boff = bok ? (int)((n * (uint32_t)d.C * (uint32_t)d.HW + (jj - n * (uint32_t)d.HW)) * 4u) + 2 * prow * chw4 : OOB;
    }
    float bst[NIT][2][PV];
    f32x2 tsc[TF ? NIT : 1], tsh[TF ? NIT : 1];
    auto load_b = [&](int c0) {                        // channels >= C read 0 (also the prefetch past the end)
#pragma unroll
        for (int r = 0; r < NIT; ++r) {
            const int c = c0 + 2 * (prow + r * (NT / PT));
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int vo = c + u < d.C ? boff : OOB;
                const int so = (c0 + 2 * r * (NT / PT) + u) * chw4;
                if constexpr (V4) {
                    u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rsrc_b, vo, so, 0);
                    bst[r][u][0] = __uint_as_float(t.x); bst[r][u][1] = __uint_as_float(t.y);
                    bst[r][u][2] = __uint_as_float(t.z); bst[r][u][3] = __uint_as_float(t.w);
                } else {
                    bst[r][u][0] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc_b, vo, so, 0));
                }
            }
            if constexpr (TF) {                        // scale/shift of the pair (c even, C even: 8-B load)
                const int vo = c < d.C ? c * 4 : OOB;
                typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
                u32x2 a = __builtin_amdgcn_raw_buffer_load_b64(rsrc_sc, vo, 0, 0);
                u32x2 b = __builtin_amdgcn_raw_buffer_load_b64(rsrc_sh, vo, 0, 0);
                tsc[r] = f32x2{__uint_as_float(a.x), __uint_as_float(a.y)};
                tsh[r] = f32x2{__uint_as_float(b.x), __uint_as_float(b.y)};
            }
        }
    };
    auto store_b = [&](float* dst) {
#pragma unroll
        for (int r = 0; r < NIT; ++r) {
            float x[2][PV];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int q = 0; q < PV; ++q) {
                    float t = bst[r][u][q];
                    if constexpr (TF) {
                        t = fmaf(t, tsc[r][u], tsh[r][u]);
                        t = d.relu ? fmaxf(t, 0.f) : t;
                        t = bok ? t : 0.f;             // out-of-range pixels / channels (scale, shift read 0 there)
                    }
                    x[u][q] = t;
                }
            float* p = dst + ((prow + r * (NT / PT)) * BN + pcol) * 2;
            if constexpr (V4) {
                *(f32x4*)p = f32x4{x[0][0], x[1][0], x[0][1], x[1][1]};
                *(f32x4*)(p + 4) = f32x4{x[0][2], x[1][2], x[0][3], x[1][3]};
            } else {
                *(f32x2*)p = f32x2{x[0][0], x[1][0]};
            }
        }
    };

    // ---- weights: lane (row, h) holds k = 8h .. 8h+7 of its rows, straight from global memory
    const __amdgpu_buffer_rsrc_t rsrc_a = make_rsrc(d.w, d.nw);
    int aoff[MI];
#pragma unroll
    for (int a = 0; a < MI; ++a) {
        const int row = i0 + wm * (BM / 2) + a * 32 + l31;
        aoff[a] = row < d.M ? (row * d.C + lh * 8) * 4 : OOB;
    }
    auto load_a = [&](float (&dst)[MI][8], int c) {   // c >= C: zeros
#pragma unroll
        for (int a = 0; a < MI; ++a) {
            const int vo = c < d.C ? aoff[a] : OOB;
            u32x4 t0 = __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, vo, c * 4, 0);
            u32x4 t1 = __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, vo + 16, c * 4, 0);
            dst[a][0] = __uint_as_float(t0.x); dst[a][1] = __uint_as_float(t0.y);
            dst[a][2] = __uint_as_float(t0.z); dst[a][3] = __uint_as_float(t0.w);
            dst[a][4] = __uint_as_float(t1.x); dst[a][5] = __uint_as_float(t1.y);
            dst[a][6] = __uint_as_float(t1.z); dst[a][7] = __uint_as_float(t1.w);
        }
    };

    f32x16 acc[MI][NI];
#pragma unroll
    for (int a = 0; a < MI; ++a)
#pragma unroll
        for (int b = 0; b < NI; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    // B fragments of sub-chunk t: NI pixels x 4 k-pairs, 8 bytes each (rows t*8 + 4h + jp)
    const int b_frag = lh * 4 * BN + wn * (BN / 2) + l31;
    auto read_b = [&](f32x2 (&dst)[NI][4], const float* buf, int t) {
        const f32x2* p = (const f32x2*)buf + t * 8 * BN + b_frag;
#pragma unroll
        for (int b = 0; b < NI; ++b)
#pragma unroll
            for (int jp = 0; jp < 4; ++jp) dst[b][jp] = p[jp * BN + b * 32];
    };
    float areg[2][MI][8];
    f32x2 breg[2][NI][4];
    auto mfmas = [&](int set) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int a = 0; a < MI; ++a)
#pragma unroll
                for (int b = 0; b < NI; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[set][a][j], breg[set][b][j >> 1][j & 1],
                                                                     acc[a][b], 0, 0, 0);
    };

    load_b(0);
    load_a(areg[0], 0);
    store_b(Bs(0));
    __syncthreads();
    read_b(breg[0], Bs(0), 0);

    for (int s = 0; s < nstage; ++s) {
        const int c0 = s * PW_KS;
        const float* bcur = Bs(s & 1);
        float* bnext = Bs((s + 1) & 1);
        // sub-chunk 0: start the next stage's activations and this stage's second half
        load_b(c0 + PW_KS);
        load_a(areg[1], c0 + 16);
        read_b(breg[1], bcur, 1);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(0);
        __builtin_amdgcn_sched_barrier(0);
        // sub-chunk 1
        load_a(areg[0], c0 + PW_KS);
        __builtin_amdgcn_sched_barrier(0);
        mfmas(1);
        __builtin_amdgcn_sched_barrier(0);
        store_b(bnext);
        __syncthreads();
        read_b(breg[0], bnext, 0);
    }
    store_tile<MI, NI, BM, BN, 2, 2>(acc, dc, d.M, d.npix, i0, j0, 0);
}

// ---------------------------------------------------------------- split-operand variant (see conv3x3.hip)
//
// fp32 products as six bf16 MFMA terms of three-way split operands, fp32 accumulation.  The activations are split
// once per element on the way into LDS ([plane][k-octet][pixel][8 bf16], one ds_read_b128 per plane and
// fragment); the weights are loaded as fp32 straight into registers (lane (row, h): k = 8h..8h+7, 32 bytes) and
// split there, in the shadow of the previous chunk's MFMAs.
// DS ("dual source"): the operand is a BatchNorm-backward output that was never materialised:
//   value = ca[c]*src + cb[c]*src2 + cc[c]   (src = masked incoming gradient g, src2 = the layer's raw conv output,
//   coef = [ca | cb | cc] from scat_bn_bwd_pre).  One register set, activations one stage ahead.
// STEM: the 7x7 / stride-2 / pad-3 convolution of a 3-channel image (models/resnet.py:105, the first layer) on the same
// loop.  The contraction index is (kh, c, kw) with kw padded 7 -> 8: k-octet o = 3 kh + c holds the 8 CONSECUTIVE input
// pixels (2 oy + kh - 3, 2 ox - 3 .. 2 ox + 4) of channel c, the weight of the eighth is zero; 21 octets padded to 24
// (d.C = 192): 168 / 147 = 1.14 x the MFMA work of the exact contraction instead of 16 / 3 = 5.3 x for a channel-padded
// taps layout.  Only the staging addresses differ from the pointwise case.
// PL ("plain": one tap, C % 32 == 0 — every pointwise layer of the networks): no per-load channel bound, and a pixel
// column past the end of the tensor is left to hold whatever the transform makes of a zero (columns are independent and
// the epilogue never stores it), so the staging VALU carries no masks at all.  Beside a busy matrix pipe a SIMD issues
// about one vector instruction per MFMA (tools/mfma_probe.hip, PROBE_PC=1): every instruction taken out of the staging
// is time given back to the MFMAs.
//
// pw_split_tile: one output tile, its nstage = ntap * ceil(C / 32) contraction stages and the epilogue (store_tile).
template <int WM, int BN, bool TF, bool DS, bool STEM, bool PL, bool BNB = false>
__device__ __forceinline__ void pw_split_tile(const PwDesc& d, const OutDesc& dc, const int tile, const int nstage) {
    static_assert(!(TF && DS), "one input transform at a time");
    static_assert(!(PL && STEM), "the stem has its own staging");
    static_assert(!STEM || (!TF && !DS), "the stem reads the raw image");
    constexpr int BM = 32 * WM, WN = 4 / WM, NI = BN / (32 * WN);
    constexpr int NIT = 4 * BN / NT;                  // k-octets staged per thread per 32-channel stage
    static_assert(NIT >= 1, "tile too small");
    extern __shared__ __align__(16) float lds[];      // B[2][3 planes][4 k-octets][BN] x 16 bytes
    auto Bs = [&](int buf) -> u32x4* { return (u32x4*)lds + buf * (12 * BN); };

    const int mt = (d.M + BM - 1) / BM;
    const int i0 = (tile % mt) * BM, j0 = (tile / mt) * BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, lh = lane >> 5;
    const int nsc = (d.C + PW_KS - 1) / PW_KS;       // 32-channel stages per tap; contraction order: (tap, channel)

    // ---- activation staging: this thread's pixel, k-octets g0 + r*(NT/BN)
    const __amdgpu_buffer_rsrc_t rsrc_b = make_rsrc(d.src, d.nsrc);
    const int pcol = tid % BN, g0 = tid / BN;
    const int chw4 = d.HW * 4;
    int boff;                                          // byte offset of (n, channel 8*g0, tap (0,0)); only used under pmask
    uint32_t pmask = 0;                                // taps that fall inside the source plane for this pixel
    bool bok;
    {
        const int j = j0 + pcol;
        bok = j < d.npix;
        const uint32_t jj = bok ? (uint32_t)j : 0u;
        const uint32_t n = d.dOHW.div(jj);
        const uint32_t r = jj - n * (uint32_t)d.OHW;
        const int oy = (int)d.dOW.div(r), ox = (int)r - oy * d.OW;
        const int sy0 = oy * d.a + d.c0y, sx0 = ox * d.a + d.c0x;
        boff = ((int)n * d.C * d.HW + sy0 * d.W + sx0) * 4 + 8 * g0 * chw4;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int th = t / d.KWt, tw = t - th * d.KWt;
            const bool ok = bok && t < d.ntap && (unsigned)(sy0 + th * d.tb) < (unsigned)d.H &&
                            (unsigned)(sx0 + tw * d.tb) < (unsigned)d.W;
            pmask |= (ok ? 1u : 0u) << t;
        }
    }
    // two register sets: the activations of stage s+2 are requested at the top of stage s and written to LDS at the
    // end of stage s+1 (one stage of cover is not enough for an HBM miss at 2 waves per SIMD)
    float bst[DS ? 1 : 2][NIT][8];
    float bst2[DS ? NIT : 1][8];
    const __amdgpu_buffer_rsrc_t rsrc_b2 = make_rsrc(DS ? d.src2 : d.src, DS ? d.nsrc : 0);
    // STEM: (image, oy, ox) of this thread's pixel
    int st_n = 0, st_oy = 0, st_ox = 0;
    if constexpr (STEM) {
        const uint32_t jj = bok ? (uint32_t)(j0 + pcol) : 0u;
        const uint32_t n = d.dOHW.div(jj);
        const uint32_t r = jj - n * (uint32_t)d.OHW;
        st_n = (int)n; st_oy = (int)d.dOW.div(r); st_ox = (int)r - st_oy * d.OW;
    }
    auto load_b = [&](int st, auto set_tag) {         // st >= nstage: every lane reads 0
        constexpr int Q = decltype(set_tag)::value;
        if constexpr (STEM) {
#pragma unroll
            for (int r = 0; r < NIT; ++r) {
                const int o = 4 * st + g0 + r * (NT / BN);          // k-octet = (kh, c)
                const int kh = o / 3, c = o - 3 * kh;
                const int iy = 2 * st_oy + kh - 3, ix0 = 2 * st_ox - 3;
                const bool rowok = bok && o < 21 && st < nstage && (unsigned)iy < (unsigned)d.H;
                const int base = (((st_n * 3 + c) * d.H + iy) * d.W + ix0) * 4;
#pragma unroll
                for (int m = 0; m < 8; ++m)
                    bst[Q][r][m] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                        rsrc_b, rowok && (unsigned)(ix0 + m) < (unsigned)d.W ? base + 4 * m : OOB, 0, 0));
            }
            return;
        }
        const int tap = st / nsc, c0 = (st - tap * nsc) * PW_KS;
        const int th = tap / d.KWt, tw = tap - th * d.KWt;
        const int vbase = ((pmask >> (tap < 9 ? tap : 9)) & 1u) && st < nstage ? boff + (th * d.W + tw) * d.tb * 4 : OOB;
#pragma unroll
        for (int r = 0; r < NIT; ++r) {
            const int c = c0 + 8 * (g0 + r * (NT / BN));
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                bst[Q][r][m] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                    rsrc_b, PL || c + m < d.C ? vbase : OOB, (c0 + 8 * r * (NT / BN) + m) * chw4, 0));
                if constexpr (DS)
                    bst2[r][m] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                        rsrc_b2, PL || c + m < d.C ? vbase : OOB, (c0 + 8 * r * (NT / BN) + m) * chw4, 0));
            }
        }
    };
    // a staging thread's k-octet is the same for its whole wavefront (BN >= 64): the fused transform's constants are
    // scalar loads
    const int g0u = __builtin_amdgcn_readfirstlane(g0);
    const float relu_lo = d.relu ? 0.f : -__builtin_inff();     // ReLU as a lower bound: one v_max, no select
    auto store_b = [&](int st, u32x4* dst, auto set_tag) {
        constexpr int Q = decltype(set_tag)::value;
        const int tap = st / nsc, c0 = (st - tap * nsc) * PW_KS;
        const bool live = (pmask >> (tap < 9 ? tap : 9)) & 1u;   // padding must stay zero AFTER the transform
#pragma unroll
        for (int r = 0; r < NIT; ++r) {
            u32x4 hi, mid, lo;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float x[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int m = 2 * q + u;
                    float t = bst[Q][r][m];
                    if constexpr (TF) {
                        const int c = c0 + 8 * (g0u + r * (NT / BN)) + m;
                        const int cc = PL || c < d.C ? c : 0;
                        t = fmaxf(fmaf(t, d.scale[cc], d.shift[cc]), relu_lo);
                        if constexpr (!PL) t = live ? t : 0.f;
                    }
                    if constexpr (DS) {
                        const int c = c0 + 8 * (g0u + r * (NT / BN)) + m;
                        const int cc = PL || c < d.C ? c : 0;
                        t = fmaf(d.coef[cc], t, fmaf(d.coef[d.C + cc], bst2[r][m], d.coef[2 * d.C + cc]));
                        if constexpr (!PL) t = (live && c < d.C) ? t : 0.f;
                    }
                    x[u] = t;
                }
                uint32_t h, mm, l;
                split3(x[0], x[1], h, mm, l);
                hi[q] = h; mid[q] = mm; lo[q] = l;
            }
            const int g = g0 + r * (NT / BN);
            dst[(0 * 4 + g) * BN + pcol] = hi;
            dst[(1 * 4 + g) * BN + pcol] = mid;
            dst[(2 * 4 + g) * BN + pcol] = lo;
        }
    };

    // the same work in 2*NI slices, one per MFMA group of a stage: slice i splits PP element pairs and writes an
    // octet's three fragments once its fourth pair is done (fragments live in shi/smid/slo across slices)
    constexpr int PP = NIT * 4 / (2 * NI) > 0 ? NIT * 4 / (2 * NI) : 1;
    uint32_t shi[2], smid[2], slo[2];                  // one half octet: written as 8 bytes per plane
    auto store_slice = [&](int st, u32x4* dst, auto set_tag, auto idx_tag) {
        constexpr int Q = decltype(set_tag)::value, IDX = decltype(idx_tag)::value;
        const int tap = st / nsc, c0 = (st - tap * nsc) * PW_KS;
        const bool live = (pmask >> (tap < 9 ? tap : 9)) & 1u;
        static_for<PP>([&](auto j_tag) {
            constexpr int pp = IDX * PP + decltype(j_tag)::value;
            if constexpr (pp < NIT * 4) {
            constexpr int r = pp >> 2, q = pp & 3;
            float x[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int m = 2 * q + u;
                float t = bst[Q][r][m];
                if constexpr (TF) {
                    const int c = c0 + 8 * (g0u + r * (NT / BN)) + m;
                    const int cc = PL || c < d.C ? c : 0;
                    t = fmaxf(fmaf(t, d.scale[cc], d.shift[cc]), relu_lo);
                    if constexpr (!PL) t = live ? t : 0.f;
                }
                x[u] = t;
            }
            uint32_t h, mm, l;
            split3(x[0], x[1], h, mm, l);
            shi[q & 1] = h; smid[q & 1] = mm; slo[q & 1] = l;
            if constexpr ((q & 1) == 1) {
                typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
                const int g = g0 + r * (NT / BN);
                u32x2* p = (u32x2*)(dst + (0 * 4 + g) * BN + pcol) + (q >> 1);
                p[0] = u32x2{shi[0], shi[1]};
                p[(size_t)4 * BN * 2] = u32x2{smid[0], smid[1]};
                p[(size_t)8 * BN * 2] = u32x2{slo[0], slo[1]};
            }
            }
        });
    };
    // ---- weights: pre-split planes ws[chunk][plane][row][16 bf16]; lane (row, h) takes 16 bytes per plane
    const __amdgpu_buffer_rsrc_t rsrc_a = make_rsrc(d.w, d.nw);
    const int row = i0 + wm * 32 + l31;
    const int aoff = row < d.M ? row * 32 + lh * 16 : OOB;
    const int aplane = d.M * 32;                       // bytes per (chunk, plane) slab
    const int nchunk = (d.C + 15) / 16;
    // sub-chunk q = 2*stage + t of the (tap, channel) order -> slab (tap*nchunk + chunk); a stage's second sub-chunk
    // may lie past the channels (C % 32 == 16), the sub-chunk after the last stage always does: zeros
    auto load_a = [&](u32x4 (&dst)[3], int q) {
        const int st = q >> 1, tap = st / nsc, ch = (st - tap * nsc) * 2 + (q & 1);
        const int vo = (ch < nchunk && st < nstage) ? aoff : OOB;
#pragma unroll
        for (int p = 0; p < 3; ++p)
            dst[p] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, vo, ((tap * nchunk + ch) * 3 + p) * aplane, 0);
    };

    f32x16 acc[1][NI];
#pragma unroll
    for (int b = 0; b < NI; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][b][r] = 0.f;

    const int b_frag = lh * BN + wn * (BN / WN) + l31;          // u32x4 index inside (plane 0, octet pair 0)
    auto read_b = [&](u32x4 (&dst)[3], const u32x4* buf, int t, int b) {
        const u32x4* p = buf + 2 * t * BN + b_frag + b * 32;
#pragma unroll
        for (int q = 0; q < 3; ++q) dst[q] = p[q * 4 * BN];
    };

    u32x4 areg[2][3];
    u32x4 bfr[2][3];

    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    // diag build only (SCAT_TUNE=77, tools/pw_stamp.py): thread 0 overwrites the tile's first 8 outputs with time stamps
    const bool stamp = kDiag && d.variant == 77;
    unsigned long long ts0 = 0, ts1 = 0, ts2 = 0;
    if (stamp) ts0 = __builtin_amdgcn_s_memrealtime();
    if constexpr (DS) {
        load_b(0, S0{});
        load_a(areg[0], 0);
        store_b(0, Bs(0), S0{});
        __syncthreads();
        read_b(bfr[0], Bs(0), 0, 0);
        for (int s = 0; s < nstage; ++s) {
            const u32x4* bcur = Bs(s & 1);
            u32x4* bnext = Bs((s + 1) & 1);
            load_b(s + 1, S0{});
            static_for<2 * NI>([&](auto i_tag) {
                constexpr int I = decltype(i_tag)::value, t = I / NI, b = I % NI;
                if constexpr (b == 0) load_a(areg[t ^ 1], 2 * s + t + 1);
                constexpr int fcur = I & 1, fnxt = fcur ^ 1;
                if constexpr (b + 1 < NI) read_b(bfr[fnxt], bcur, t, b + 1);
                else if constexpr (t == 0) read_b(bfr[fnxt], bcur, 1, 0);
                __builtin_amdgcn_sched_barrier(0);
                acc[0][b] = mfma_split(areg[t], bfr[fcur], acc[0][b]);
                __builtin_amdgcn_sched_barrier(0);
            });
            store_b(s + 1, bnext, S0{});
            __syncthreads();
            read_b(bfr[0], bnext, 0, 0);
        }
    } else {
        load_b(0, S0{});
        load_b(1, S1{});
        load_a(areg[0], 0);
        store_b(0, Bs(0), S0{});
        __syncthreads();
        read_b(bfr[0], Bs(0), 0, 0);
        if (stamp) ts1 = __builtin_amdgcn_s_memrealtime();

        // stage s: LDS buffer s & 1, register set s & 1 is free again (its data went to LDS one stage ago)
        auto stage = [&](int s, auto cur_tag) {
            constexpr int CUR = decltype(cur_tag)::value;
            const u32x4* bcur = Bs(CUR);
            u32x4* bnext = Bs(CUR ^ 1);
            load_b(s + 2, std::integral_constant<int, CUR>{});
                // the split of stage s+1 (its data landed a stage ago, its LDS buffer has been free since the last
                // barrier) rides in the shadow of this stage's MFMAs: one slice per MFMA group
                static_for<2 * NI>([&](auto i_tag) {
                    constexpr int I = decltype(i_tag)::value, t = I / NI, b = I % NI;
                    if constexpr (b == 0) load_a(areg[t ^ 1], 2 * s + t + 1);
                    constexpr int fcur = I & 1, fnxt = fcur ^ 1;
                    if constexpr (b + 1 < NI) read_b(bfr[fnxt], bcur, t, b + 1);
                    else if constexpr (t == 0) read_b(bfr[fnxt], bcur, 1, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    store_slice(s + 1, bnext, std::integral_constant<int, CUR ^ 1>{}, i_tag);
                    acc[0][b] = mfma_split(areg[t], bfr[fcur], acc[0][b]);
                    __builtin_amdgcn_sched_barrier(0);
                });
            __syncthreads();
            read_b(bfr[0], bnext, 0, 0);
        };
        for (int s = 0; s < nstage; s += 2) {
            stage(s, S0{});
            if (s + 1 < nstage) stage(s + 1, S1{});
        }
    }
    if (stamp) ts2 = __builtin_amdgcn_s_memrealtime();
    store_tile<1, NI, BM, BN, WM, WN, BNB>(acc, dc, d.M, d.npix, i0, j0, 0);
    if (stamp) {
        __syncthreads();
        if (tid == 0 && dc.mode == 1) {
            __builtin_amdgcn_s_waitcnt(0);
            const uint32_t n = dc.dHW.div((uint32_t)j0);
            const int hw = j0 - (int)n * dc.HW;
            if (hw + 8 <= dc.HW && ((hw & 1) == 0)) {
                unsigned long long* o = (unsigned long long*)(dc.p + ((int64_t)n * dc.C + i0) * dc.HW + hw);
                o[0] = ts0; o[1] = ts1; o[2] = ts2; o[3] = __builtin_amdgcn_s_memrealtime();
            }
        }
    }
}

// one tile per workgroup, XCD-aware tile order
template <int WM, int BN, bool TF, bool DS = false, bool STEM = false, bool PL = false, bool BNB = false>
__global__ __launch_bounds__(NT, 3) void conv1x1_split_kernel(PwDesc d, OutDesc dc) {
    constexpr int BM = 32 * WM;
    const int mt = (d.M + BM - 1) / BM, nt = (d.npix + BN - 1) / BN;
    const int tile = xcd_remap(blockIdx.x, mt * nt);
    const int nstage = d.ntap * ((d.C + PW_KS - 1) / PW_KS);
    if constexpr (kDiag) {
        // tools build, SCAT_TUNE = 300 + t: the workgroups of the second / third residency slot of a CU (block index / 256)
        // start t / 2t microseconds late, so that the co-resident tiles' prologues and epilogues stop coinciding
        if (d.variant >= 300 && d.variant < 400) {
            const int slot = (blockIdx.x >> 8) % 3;
            const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();     // 100 MHz
            const unsigned long long wait = (unsigned long long)slot * (d.variant - 300) * 100ull;
            while (__builtin_amdgcn_s_memrealtime() - t0 < wait) __builtin_amdgcn_s_sleep(32);
        }
    }
    pw_split_tile<WM, BN, TF, DS, STEM, PL, BNB>(d, dc, tile, nstage);
}

// ---------------------------------------------------------------- producer / consumer wave specialisation
//
// The split kernel above makes every wavefront do everything: request activations, apply the fused transform, split
// them into bf16 terms, write LDS, read fragments, issue MFMAs.  Its instruction stream per 32-channel stage is
// ~230 VALU + ~250 SALU + 24 LDS reads + 22 loads around 48 MFMAs, and a wavefront issues in order: the matrix pipe
// idles while its owner splits (PMC: 0.34 busy at 2.3 wavefronts per SIMD, half of every wavefront's life spent
// waiting to issue).  Here a 768-thread workgroup has two kinds of wavefront:
//   * wavefronts 8-11, producers: global loads (three stages ahead) -> fused BatchNorm+ReLU -> three-way split ->
//     LDS (two stages ahead of the readers, three buffers).  No MFMA, no LDS reads.
//   * wavefronts 0-7, consumers (32 rows each): weights straight from L2 into operand registers (pre-split planes),
//     activation fragments from LDS, 32x32x16 MFMAs.  No staging VALU; the first fragment of the next stage is read
//     before the barrier because that stage was published a barrier earlier.
// One s_barrier per stage joins the two streams.  A 256 x 128 tile is staged once for eight consumers: a SIMD holds two
// consumers and one producer of ONE workgroup per CU, its matrix pipe fed by two wavefronts whose streams are MFMA +
// LDS reads only, its VALU by one whose stream never waits for the matrix pipe.
// W4 (pointwise stride-1 layers with HW % 4 == 0): column (b, c) of the tile is pixel 4c + b instead of 32b + c.  A
// producer lane then owns FOUR CONSECUTIVE pixels of four channels — four 16-byte loads per stage instead of sixteen
// 4-byte ones, LDS writes of 8 bytes that consecutive lanes place in consecutive slots — and a consumer lane's four
// accumulator columns are four consecutive pixels of one row: the epilogue stores 16 bytes per instruction instead of
// 4.  The MFMA does not care which pixel a column is; only the two ends of the kernel know.
// (Four consumers, 64 rows per consumer, 16x16x32 consumers and a barrier-free ring were measured and lost: DESIGN 1b.)
constexpr int PC_NCW = 8;                             // consumer wavefronts; + 4 producers
template <bool TF, bool W4>
__global__ __launch_bounds__((PC_NCW + 4) * 64, 3) void conv1x1_pc_kernel(PwDesc d, OutDesc dc) {
    constexpr int NCW = PC_NCW, BN = 128, BM = 32 * NCW, NI = 4, PT = 256;
    constexpr int NIT = 4 * BN / PT;                  // k-octets per producer thread per 32-channel stage
    constexpr int BUF = 12 * BN;                      // u32x4 per buffer: [3 planes][4 k-octets][BN]
    extern __shared__ __align__(16) float lds[];
    u32x4* const B0 = (u32x4*)lds;

    const int mt = (d.M + BM - 1) / BM, nt = (d.npix + BN - 1) / BN;
    const int tile = xcd_remap(blockIdx.x, mt * nt);
    const int i0 = (tile % mt) * BM, j0 = (tile / mt) * BN;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int nsc = (d.C + PW_KS - 1) / PW_KS;
    const int nstage = d.ntap * nsc;
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;

    if constexpr (W4) {
      if (wave >= NCW) {
        // ------------------------------------------------------------ producer, wide form: wavefront = k-octet,
        // lane = (pixel quad p, channel half h)
        const __amdgpu_buffer_rsrc_t rsrc_b = make_rsrc(d.src, d.nsrc);
        const __amdgpu_buffer_rsrc_t rsrc_sc = make_rsrc(TF ? d.scale : d.src, TF ? d.C : 0);
        const __amdgpu_buffer_rsrc_t rsrc_sh = make_rsrc(TF ? d.shift : d.src, TF ? d.C : 0);
        const int g = wave - NCW, p = lane >> 1, h = lane & 1;
        const int chw4 = d.HW * 4;
        int boff;                                      // byte offset of (image, channel 8g + 4h, first pixel of the quad)
        {
            const int j = j0 + 4 * p;
            const bool bok = j < d.npix;
            const uint32_t jj = bok ? (uint32_t)j : 0u;
            const uint32_t n = d.dHW.div(jj);
            boff = bok ? (int)((n * (uint32_t)d.C * (uint32_t)d.HW + (jj - n * (uint32_t)d.HW)) * 4u) +
                             (8 * g + 4 * h) * chw4 : OOB;
        }
        u32x4 bst[2][4];                               // [register set][channel m] = 4 pixels
        f32x4 tsc[2], tsh[2];
        auto load_b = [&](int st, auto set_tag) {     // st >= nstage: zeros
            constexpr int Q = decltype(set_tag)::value;
            const int c0 = st * PW_KS;
            const int vo = (c0 + 8 * g < d.C && st < nstage) ? boff : OOB;      // C % 16 == 0: whole octets
#pragma unroll
            for (int m = 0; m < 4; ++m)
                bst[Q][m] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_b, vo, (c0 + m) * chw4, 0);
            if constexpr (TF) {
                const int co = (c0 + 8 * g + 4 * h < d.C && st < nstage) ? (c0 + 8 * g + 4 * h) * 4 : OOB;
                tsc[Q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_sc, co, 0, 0));
                tsh[Q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_sh, co, 0, 0));
            }
        };
        typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
        auto store_b = [&](int st, u32x4* dst, auto set_tag) {
            constexpr int Q = decltype(set_tag)::value;
            u32x2* base = (u32x2*)(dst + g * BN + p) + h;             // plane 0, position p (pixel 4p), half h
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float x[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    float t = __uint_as_float(bst[Q][m][k]);
                    if constexpr (TF) {
                        t = fmaf(t, tsc[Q][m], tsh[Q][m]);          // (channels >= C: scale = shift = 0 -> 0)
                        t = d.relu ? fmaxf(t, 0.f) : t;
                    }
                    x[m] = t;
                }
                uint32_t h0, m0, l0, h1, m1, l1;
                split3(x[0], x[1], h0, m0, l0);
                split3(x[2], x[3], h1, m1, l1);
                u32x2* q = base + (size_t)k * 32 * 2;                  // position k*32 + p
                q[0] = u32x2{h0, h1};
                q[(size_t)4 * BN * 2] = u32x2{m0, m1};
                q[(size_t)8 * BN * 2] = u32x2{l0, l1};
            }
        };
        load_b(0, S0{});
        load_b(1, S1{});
        store_b(0, B0, S0{});
        load_b(2, S0{});
        store_b(1, B0 + BUF, S1{});
        __syncthreads();
        int wb = 2;
        auto iter = [&](int s, auto par_tag) {
            constexpr int P = decltype(par_tag)::value;
            load_b(s + 3, std::integral_constant<int, P ^ 1>{});
            store_b(s + 2, B0 + wb * BUF, par_tag);
            wb = wb == 2 ? 0 : wb + 1;
            __syncthreads();
        };
        for (int s = 0; s < nstage; s += 2) {
            iter(s, S0{});
            if (s + 1 < nstage) iter(s + 1, S1{});
        }
        return;
      }
    } else
    if (wave >= NCW) {
        // ------------------------------------------------------------ producer
        const int ptid = threadIdx.x - 64 * NCW;
        const __amdgpu_buffer_rsrc_t rsrc_b = make_rsrc(d.src, d.nsrc);
        const int pcol = ptid % BN, g0 = ptid / BN;
        const int g0u = __builtin_amdgcn_readfirstlane(g0);
        const int chw4 = d.HW * 4;
        int boff;
        uint32_t pmask = 0;
        {
            const int j = j0 + pcol;
            const bool bok = j < d.npix;
            const uint32_t jj = bok ? (uint32_t)j : 0u;
            const uint32_t n = d.dOHW.div(jj);
            const uint32_t r = jj - n * (uint32_t)d.OHW;
            const int oy = (int)d.dOW.div(r), ox = (int)r - oy * d.OW;
            const int sy0 = oy * d.a + d.c0y, sx0 = ox * d.a + d.c0x;
            boff = ((int)n * d.C * d.HW + sy0 * d.W + sx0) * 4 + 8 * g0 * chw4;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int th = t / d.KWt, tw = t - th * d.KWt;
                const bool ok = bok && t < d.ntap && (unsigned)(sy0 + th * d.tb) < (unsigned)d.H &&
                                (unsigned)(sx0 + tw * d.tb) < (unsigned)d.W;
                pmask |= (ok ? 1u : 0u) << t;
            }
        }
        float bst[2][NIT][8];
        auto load_b = [&](int st, auto set_tag) {     // st >= nstage: every lane reads 0
            constexpr int Q = decltype(set_tag)::value;
            const int tap = st / nsc, c0 = (st - tap * nsc) * PW_KS;
            const int th = tap / d.KWt, tw = tap - th * d.KWt;
            const int vbase = ((pmask >> (tap < 9 ? tap : 9)) & 1u) && st < nstage ? boff + (th * d.W + tw) * d.tb * 4 : OOB;
#pragma unroll
            for (int r = 0; r < NIT; ++r) {
                const int cu = c0 + 8 * (g0u + r * (PT / BN));          // wave-uniform; C % 16 == 0: whole octets
                const int vo = cu < d.C ? vbase : OOB;
#pragma unroll
                for (int m = 0; m < 8; ++m)
                    bst[Q][r][m] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                        rsrc_b, vo, (c0 + 8 * r * (PT / BN) + m) * chw4, 0));
            }
        };
        auto store_b = [&](int st, u32x4* dst, auto set_tag) {
            constexpr int Q = decltype(set_tag)::value;
            const int tap = st / nsc, c0 = (st - tap * nsc) * PW_KS;
            const bool live = (pmask >> (tap < 9 ? tap : 9)) & 1u;       // padding must stay zero AFTER the transform
#pragma unroll
            for (int r = 0; r < NIT; ++r) {
                float x[8];
                const int cu = c0 + 8 * (g0u + r * (PT / BN));
                const int cc = cu < d.C ? cu : 0;
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    float t = bst[Q][r][m];
                    if constexpr (TF) {
                        t = fmaf(t, d.scale[cc + m], d.shift[cc + m]);
                        t = d.relu ? fmaxf(t, 0.f) : t;
                        t = (live && cu < d.C) ? t : 0.f;
                    }
                    x[m] = t;
                }
                u32x4 hi, mid, lo;
                split3x8(x, hi, mid, lo);
                const int g = g0 + r * (PT / BN);
                dst[(0 * 4 + g) * BN + pcol] = hi;
                dst[(1 * 4 + g) * BN + pcol] = mid;
                dst[(2 * 4 + g) * BN + pcol] = lo;
            }
        };
        load_b(0, S0{});
        load_b(1, S1{});
        store_b(0, B0, S0{});
        load_b(2, S0{});
        store_b(1, B0 + BUF, S1{});
        __syncthreads();
        int wb = 2;                                    // buffer of stage s + 2
        auto iter = [&](int s, auto par_tag) {
            constexpr int P = decltype(par_tag)::value;
            load_b(s + 3, std::integral_constant<int, P ^ 1>{});
            store_b(s + 2, B0 + wb * BUF, par_tag);
            wb = wb == 2 ? 0 : wb + 1;
            __syncthreads();
        };
        for (int s = 0; s < nstage; s += 2) {
            iter(s, S0{});
            if (s + 1 < nstage) iter(s + 1, S1{});
        }
        return;
    }

    // ---------------------------------------------------------------- consumer: rows i0 + wave*32 ..
    const int l31 = lane & 31, lh = lane >> 5;
    const __amdgpu_buffer_rsrc_t rsrc_a = make_rsrc(d.w, d.nw);
    // (a one-trip loop, left from the form with several row blocks per consumer: without it hipcc orders the address
    // arithmetic of the wide form differently, and the kernel keeps the instruction stream it was measured with)
    int aoff = OOB;
#pragma unroll
    for (int a = 0; a < 1; ++a) {
        const int row = i0 + (wave + a) * 32 + l31;
        aoff = row < d.M ? row * 32 + lh * 16 : OOB;
    }
    const int aplane = d.M * 32;
    const int nchunk = (d.C + 15) / 16;
    auto load_a = [&](u32x4 (&dst)[3], int q) {
        const int st = q >> 1, tap = st / nsc, ch = (st - tap * nsc) * 2 + (q & 1);
        const bool ok = ch < nchunk && st < nstage;
#pragma unroll
        for (int p = 0; p < 3; ++p)
            dst[p] = __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, ok ? aoff : OOB, ((tap * nchunk + ch) * 3 + p) * aplane, 0);
    };
    f32x16 acc[1][NI];
#pragma unroll
    for (int b = 0; b < NI; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][b][r] = 0.f;
    const int b_frag = lh * BN + l31;
    auto read_b = [&](u32x4 (&dst)[3], const u32x4* buf, int t, int b) {
        const u32x4* p = buf + 2 * t * BN + b_frag + b * 32;
#pragma unroll
        for (int q = 0; q < 3; ++q) dst[q] = p[q * 4 * BN];
    };
    u32x4 areg[2][3];
    u32x4 bfr[2][3];
    load_a(areg[0], 0);
    __syncthreads();
    read_b(bfr[0], B0, 0, 0);
    int rb = 0;
    for (int s = 0; s < nstage; ++s) {
        const u32x4* bcur = B0 + rb * BUF;
        if (++rb == 3) rb = 0;
        static_for<2 * NI>([&](auto i_tag) {
            constexpr int I = decltype(i_tag)::value, t = I / NI, b = I % NI;
            if constexpr (b == 0) load_a(areg[t ^ 1], 2 * s + t + 1);
            constexpr int fcur = I & 1, fnxt = fcur ^ 1;
            if constexpr (b + 1 < NI) read_b(bfr[fnxt], bcur, t, b + 1);
            else if constexpr (t == 0) read_b(bfr[fnxt], bcur, 1, 0);
            else read_b(bfr[fnxt], B0 + rb * BUF, 0, 0);      // the next stage: published one barrier ago
            __builtin_amdgcn_sched_barrier(0);
            acc[0][b] = mfma_split(areg[t], bfr[fcur], acc[0][b]);
            __builtin_amdgcn_sched_barrier(0);
        });
        __syncthreads();
    }
    if constexpr (W4) {
        // lane (l31, lh): rows (reg & 3) + 8 (reg >> 2) + 4 lh of its 32-row block, pixels j0 + 4 l31 .. + 3 = the four
        // accumulator tiles' column l31: one 16-byte store per row (NCHW, whole quads inside one image)
        const __amdgpu_buffer_rsrc_t rc = make_rsrc(dc.p, dc.n);
        const int j = j0 + 4 * l31;
        const bool colok = j < d.npix;
        const uint32_t jj = colok ? (uint32_t)j : 0u;
        const uint32_t n = dc.dHW.div(jj);
        const int coloff = (int)n * dc.C * dc.HW + (int)(jj - n * (uint32_t)dc.HW);
        const bool biasi = dc.bias && dc.bias_mode == 1;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const bool ok = colok && i < d.M;
            const int vo = ok ? (coloff + i * dc.HW) * 4 : OOB;
            const float bi = biasi ? dc.bias[i < d.M ? i : 0] : 0.f;
            f32x4 v = f32x4{acc[0][0][r] + bi, acc[0][1][r] + bi, acc[0][2][r] + bi, acc[0][3][r] + bi};
            if (dc.accumulate) v += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rc, vo, 0, 0));
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rc, vo, 0, 0);
        }
        return;
    }
    store_tile<1, NI, BM, BN, NCW, 1>(acc, dc, d.M, d.npix, i0, j0, 0);
}

// ws[tap][ch][plane][i][16 bf16]: the three bf16 terms of element (i, c, tap).  w is the conv weight
// [Cout][Cin][KH][KW]; forward: (i, c) = (co, ci); transposed (data gradient): (i, c) = (ci, co).  Tap t of the ntap
// listed ones is (kh0 + ts*(t / KWt), kw0 + ts*(t % KWt)).  (WPrepJob in conv_common.h.)
// One work item = one k-octet of one row: 8 source weights -> three 16-byte stores (hi | mid | lo planes), the stores of
// a wavefront contiguous (item index = (r, i, half) with half fastest).  The first version made one element per thread
// with three 2-byte stores: 207 us per step for the 106 convolutions of ResNet-50 against ~60 us of HBM time.
__device__ __forceinline__ void wprep_octet(const WPrepJob& j, int64_t e) {
    const int nchunk = (j.C + 15) / 16;
    const int half = e & 1;
    int64_t r = e >> 1;
    const int i = r % j.M;
    r /= j.M;                                            // r = tap * nchunk + ch
    const int ch = r % nchunk, t = r / nchunk;
    const int kh = j.kh0 + j.ts * (t / j.KWt), kw = j.kw0 + j.ts * (t % j.KWt);
    const int c0 = ch * 16 + half * 8;
    const int64_t tap = (int64_t)kh * j.KW + kw, kk = (int64_t)j.KH * j.KW;
    float v[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int c = c0 + m;
        const int64_t pair = j.transposed ? (int64_t)c * j.M + i : (int64_t)i * j.C + c;
        v[m] = c < j.C ? j.w[pair * kk + tap] : 0.f;
    }
    u32x4 hi, mid, lo;
    split3x8(v, hi, mid, lo);
    u32x4* dst = (u32x4*)j.dst + ((r * 3) * j.M + i) * 2 + half;      // 16-byte units
    dst[0] = hi;
    dst[(int64_t)j.M * 2] = mid;
    dst[(int64_t)j.M * 4] = lo;
}
static inline int64_t wprep_elements(const WPrepJob& j) { return (int64_t)j.ntap * ((j.C + 15) / 16) * j.M * 2; }

__global__ __launch_bounds__(256) void w_taps_split_kernel(WPrepJob j) {
    const int64_t n = (int64_t)j.ntap * ((j.C + 15) / 16) * j.M * 2;
    for (int64_t e = blockIdx.x * 256ll + threadIdx.x; e < n; e += gridDim.x * 256ll) wprep_octet(j, e);
}

// the same for a table of jobs (device memory, sorted by blk0): block b belongs to the last job with blk0 <= b
__global__ __launch_bounds__(256) void w_prep_batch_kernel(const WPrepJob* __restrict__ jobs, int njobs) {
    int lo = 0, hi = njobs - 1;
    const int b = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].blk0 <= b) lo = mid;
        else hi = mid - 1;
    }
    const WPrepJob j = jobs[lo];
    const int64_t n = (int64_t)j.ntap * ((j.C + 15) / 16) * j.M * 2;
    const int64_t e = (int64_t)(b - j.blk0) * 256 + threadIdx.x;
    if (e < n) wprep_octet(j, e);
}

WPrepJob wprep_job(const float* w, void* dst, int M, int C, int transposed, int KH, int KW, int ntap, int KWt, int kh0,
                   int kw0, int ts) {
    WPrepJob j{};
    j.w = w; j.dst = (uint16_t*)dst; j.M = M; j.C = C; j.transposed = transposed; j.KH = KH; j.KW = KW; j.ntap = ntap;
    j.KWt = KWt; j.kh0 = kh0; j.kw0 = kw0; j.ts = ts;
    j.blk0 = 0;
    j.nblk = (int)((wprep_elements(j) + 255) / 256);
    return j;
}

void wprep_batch_launch(const WPrepJob* jobs_dev, int njobs, int nblocks, hipStream_t st) {
    hipLaunchKernelGGL(w_prep_batch_kernel, dim3(nblocks), dim3(256), 0, st, jobs_dev, njobs);
}

void wprep_launch(const WPrepJob& j, hipStream_t st) {
    hipLaunchKernelGGL(w_taps_split_kernel, dim3(j.nblk < 2048 ? j.nblk : 2048), dim3(256), 0, st, j);
}

// fp32 transpose for the fp32-MFMA twin: ws[i][c] = w[c][i]
__global__ void w1x1_t_kernel(const float* __restrict__ w, float* __restrict__ ws, int M, int C) {
    const int64_t n = (int64_t)M * C;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int c = e % C, i = e / C;
        ws[e] = w[(int64_t)c * M + i];
    }
}

static int pw_plain_mode() {
    static const int m = diag_env_int("SCAT_PW_PLAIN", 1);
    return m;
}

template <int WM, int BN, bool TF, bool DS = false, bool STEM = false>
static void launch_pw_split(const PwDesc& d, const OutDesc& dc_in, hipStream_t st, ScatEpilogue* epi = nullptr) {
    constexpr int BM = 32 * WM;
    const int mt = cdiv(d.M, BM), nt = cdiv(d.npix, BN);
    constexpr size_t lds_bytes = (size_t)2 * 12 * BN * 16;
    OutDesc dc = dc_in;
    if (!dc.accumulate && !dc.bias) {                 // a forward convolution: its BatchNorm's sums ride in the epilogue
        dc.sg = nt * (4 / WM);
        if (epi_fits(epi, d.M, dc.sg)) { dc.stats = epi->part; dc.stats_shift = epi->shift; }
    }
    if (!dc.accumulate) dc.st_aux = store_policy(dc.n * 4);
    if constexpr (!STEM && !DS && !TF && WM == 4 && BN == 128) {
        // a data gradient that completes the gradient of a block output (C += ...): the BatchNorm backward's reduction
        // of the block that produced it rides in the epilogue when the caller asks for it (ScatEpilogue x / mask / mean)
        if (dc.accumulate && !dc.bias && dc.mode == 1 && d.ntap == 1 && d.C % 32 == 0 && pw_plain_mode() && epi &&
            epi->x && epi->mask && epi->mean && epi_fits(epi, d.M, nt * (4 / WM))) {
            dc.bnb_x = epi->x; dc.bnb_mask = epi->mask; dc.bnb_mean = epi->mean; dc.bnb_part = epi->part;
            dc.bnb_sg = nt * (4 / WM);
            hipLaunchKernelGGL((conv1x1_split_kernel<WM, BN, TF, DS, false, true, true>), dim3(mt * nt), dim3(NT), lds_bytes,
                               st, d, dc);
            append_kernel_label("_epibn");
            return;
        }
    }
    if constexpr (!STEM) {
        if (d.ntap == 1 && d.C % 32 == 0 && pw_plain_mode()) {
            hipLaunchKernelGGL((conv1x1_split_kernel<WM, BN, TF, DS, false, true>), dim3(mt * nt), dim3(NT), lds_bytes, st,
                               d, dc);
            return;
        }
    }
    hipLaunchKernelGGL((conv1x1_split_kernel<WM, BN, TF, DS, STEM>), dim3(mt * nt), dim3(NT), lds_bytes, st, d, dc);
}

// Tile of the split kernel by cfg: 0 = 128x128, 1 = 64x128, 2 = 64x64 (rows x pixels).  The dual-source and the stem
// kernels exist on the two 128-pixel tiles and without the fused transform only (their callers ask for nothing else).
static const char* pw_tile_name(int cfg) {
    static const char* const names[] = {"128x128", "64x128", "64x64"};
    return names[cfg];
}

template <bool DS = false, bool STEM = false>
static void launch_pw_split_cfg(int cfg, bool tf, const PwDesc& d, const OutDesc& dc, hipStream_t st,
                                ScatEpilogue* epi = nullptr) {
    if constexpr (!DS && !STEM) {
        if (tf) {
            if (cfg == 0) launch_pw_split<4, 128, true>(d, dc, st, epi);
            else if (cfg == 1) launch_pw_split<2, 128, true>(d, dc, st, epi);
            else launch_pw_split<2, 64, true>(d, dc, st, epi);
            return;
        }
        if (cfg == 2) {
            launch_pw_split<2, 64, false>(d, dc, st, epi);
            return;
        }
    }
    if (cfg == 0) launch_pw_split<4, 128, false, DS, STEM>(d, dc, st, epi);
    else launch_pw_split<2, 128, false, DS, STEM>(d, dc, st, epi);
}

// Geometry of a pointwise problem (one tap, stride 1): B images of C channels x HW pixels, M output rows.
static PwDesc pw_desc(int B, int C, int HW, int M) {
    PwDesc d{};
    d.C = C; d.M = M; d.HW = HW; d.npix = B * HW; d.dHW = FastDiv::make(HW);
    d.ntap = 1; d.KWt = 1; d.a = 1; d.tb = 1; d.c0y = 0; d.c0x = 0; d.H = 1; d.W = HW; d.OW = HW; d.OHW = HW;
    d.dOHW = FastDiv::make(HW); d.dOW = FastDiv::make(HW);
    d.nsrc = (int64_t)B * C * HW;
    d.variant = tuning();
    return d;
}

// ws[chunk = o / 2][plane][co][16 bf16], k16 = 8 (o & 1) + kw: the three bf16 terms of w[co][c][kh][kw], o = 3 kh + c;
// kw = 7 and o >= 21 are zero
__global__ __launch_bounds__(256) void stem_wprep_kernel(const float* __restrict__ w, uint16_t* __restrict__ dst, int M) {
    const int n = 12 * M * 16;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const int k16 = e & 15, co = (e >> 4) % M, ch = (e >> 4) / M;
        const int o = 2 * ch + (k16 >> 3), kw = k16 & 7;
        const int kh = o / 3, c = o - 3 * kh;
        const float v = (o < 21 && kw < 7) ? w[((co * 3 + c) * 7 + kh) * 7 + kw] : 0.f;
        uint32_t hi, mid, lo;
        split3(v, 0.f, hi, mid, lo);
        const int base = ((ch * 3) * M + co) * 16 + k16;
        dst[base] = (uint16_t)hi;
        dst[base + M * 16] = (uint16_t)mid;
        dst[base + 2 * M * 16] = (uint16_t)lo;
    }
}

// SCAT_PC: unset = per-layer choice (see scat_conv1x1_s1), 0 = every wavefront stages and multiplies
// (conv1x1_split_kernel), 5 / 6 = eight consumer wavefronts on a 256 x 128 tile (plain / wide form where the plane
// allows it); any other value = 0
static int pc_mode() {
    static const int m = [] { const char* e = getenv("SCAT_PC"); return e ? atoi(e) : -1; }();
    return m;
}

template <bool TF, bool W4>
static void launch_pw_pc(const PwDesc& d, const OutDesc& dc, hipStream_t st) {
    constexpr int BM = 32 * PC_NCW, BN = 128;
    const int mt = cdiv(d.M, BM), nt = cdiv(d.npix, BN);
    constexpr size_t lds_bytes = (size_t)3 * 12 * BN * 16;
    auto kern = conv1x1_pc_kernel<TF, W4>;
    static bool once = (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)lds_bytes) == hipSuccess);
    (void)once;
    hipLaunchKernelGGL(kern, dim3(mt * nt), dim3((PC_NCW + 4) * 64), lds_bytes, st, d, dc);
}

template <int BM, int BN, bool V4, bool TF>
static void launch_pw(const PwDesc& d, const OutDesc& dc, hipStream_t st) {
    const int mt = cdiv(d.M, BM), nt = cdiv(d.npix, BN);
    constexpr size_t lds_bytes = sizeof(float) * 2 * PW_KS * BN;
    hipLaunchKernelGGL((conv1x1_kernel<BM, BN, V4, TF>), dim3(mt * nt), dim3(NT), lds_bytes, st, d, dc);
}

template <bool V4, bool TF>
static void launch_pw_cfg(int cfg, const PwDesc& d, const OutDesc& dc, hipStream_t st) {
    if (cfg == 0) launch_pw<128, 128, V4, TF>(d, dc, st);
    else if (cfg == 1) launch_pw<64, 128, V4, TF>(d, dc, st);
    else launch_pw<64, 64, V4, TF>(d, dc, st);
}

// General entry of the split kernel: dst (+)= sum over the listed taps and C source channels.
//   source pixel of column (oy, ox), tap (th, tw): (oy*a + th*tb + c0y, ox*a + tw*tb + c0x) of src[B][C][H][W]
//   weights: taps (kh0 + ts*th, kw0 + ts*tw) of the conv weight w[Cout][Cin][KH][KW], (row, channel) = (co, ci) or,
//   transposed, (ci, co).  ws >= taps_split_ws(M, C, KHt*KWt) bytes.
int64_t taps_split_ws(int M, int C, int ntap) { return (int64_t)ntap * M * ((C + 15) / 16 * 16) * 6; }

void taps_split_launch(const TapsGeom& g, const float* src, const float* w, const OutDesc& dc, int B, int C, int M,
                       const float* in_scale, const float* in_shift, int in_relu, void* ws, const char* label,
                       hipStream_t st, bool w_ready, ScatEpilogue* epi) {
    PwDesc d{};
    d.src = src; d.scale = in_scale; d.shift = in_shift; d.relu = in_scale ? in_relu : 0;
    d.C = C; d.M = M; d.HW = g.H * g.W; d.npix = B * g.OH * g.OW; d.dHW = FastDiv::make(d.HW);
    d.ntap = g.KHt * g.KWt; d.KWt = g.KWt; d.a = g.a; d.tb = g.tb; d.c0y = g.c0y; d.c0x = g.c0x; d.H = g.H; d.W = g.W;
    d.OW = g.OW; d.OHW = g.OH * g.OW; d.dOHW = FastDiv::make(d.OHW); d.dOW = FastDiv::make(g.OW);
    d.nsrc = (int64_t)B * C * d.HW;
    d.variant = tuning();
    const int64_t nel = (int64_t)d.ntap * M * ((C + 15) / 16 * 16);
    if (!w_ready)
        wprep_launch(wprep_job(w, ws, M, C, g.transposed, g.KH, g.KW, d.ntap, g.KWt, g.kh0, g.kw0, g.ts), st);
    d.w = (const float*)ws;
    d.nw = (nel * 6 + 3) / 4;
    int cfg = M > 64 ? 0 : 1;
    if ((int64_t)cdiv(M, 128) * cdiv(d.npix, 128) < 256 && (int64_t)cdiv(M, 64) * cdiv(d.npix, 64) >= 256) cfg = 2;
    if (tuning() >= 1 && tuning() <= 3) cfg = tuning() - 1;
    set_kernel_label("%s_split_%sx32%s", label, pw_tile_name(cfg), in_scale ? "_tf" : "");
    launch_pw_split_cfg(cfg, in_scale != nullptr, d, dc, st, epi);
}

}  // namespace scat

using namespace scat;

extern "C" int64_t scat_conv2d_fwd_split_ws(int Cout, int Cin, int KH, int KW) {
    return taps_split_ws(Cout, Cin, KH * KW);
}

// Forward convolution (1x1 or 3x3, stride 1 or 2) on the taps kernel: contraction ordered (tap, channel), one
// 32-channel activation stage of one tap per barrier.  Split-operand products only (scat_get_math_mode() == 1);
// Cin % 16 == 0.  Used for the stride-2 convolutions (3x3/s1 has the halo kernel, 1x1/s1 scat_conv1x1_s1).
extern "C" int scat_conv2d_fwd_split(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int H,
                                     int W, int Cout, int KH, int KW, int stride, int pad, const float* in_scale,
                                     const float* in_shift, int in_relu, void* ws, int64_t ws_bytes, int w_ready,
                                     ScatEpilogue* epi, void* stream) {
    if (epi) epi->groups = 0;
    int OH, OW;
    if (int e = check_geom("scat_conv2d_fwd_split", B, Cin, H, W, Cout, KH, KW, stride, pad, &OH, &OW)) return e;
    SCAT_REQUIRE(x && w && y, SCAT_E_ARG, "scat_conv2d_fwd_split: null pointer");
    SCAT_REQUIRE(math_mode() == 1, SCAT_E_ARG, "scat_conv2d_fwd_split: needs the split-operand product mode");
    SCAT_REQUIRE(KH <= 3 && Cin % 16 == 0, SCAT_E_SHAPE, "scat_conv2d_fwd_split: 1x1/3x3 and Cin % 16 == 0 only");
    SCAT_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), SCAT_E_ARG, "scat_conv2d_fwd_split: scale/shift pair");
    SCAT_REQUIRE(ws && ws_bytes >= scat_conv2d_fwd_split_ws(Cout, Cin, KH, KW) && ((uintptr_t)ws & 15) == 0,
                 SCAT_E_WORKSPACE, "scat_conv2d_fwd_split: workspace too small / unaligned");
    TapsGeom g{};
    g.H = H; g.W = W; g.OH = OH; g.OW = OW; g.a = stride; g.tb = 1; g.c0y = -pad; g.c0x = -pad;
    g.KHt = KH; g.KWt = KW; g.KH = KH; g.KW = KW; g.kh0 = 0; g.kw0 = 0; g.ts = 1; g.transposed = 0;
    OutDesc dc{};
    dc.p = y; dc.mode = 1; dc.I = Cout; dc.J = B * OH * OW; dc.C = Cout; dc.HW = OH * OW;
    dc.dHW = FastDiv::make(OH * OW); dc.bias = bias; dc.bias_mode = bias ? 1 : 0; dc.n = (int64_t)B * Cout * OH * OW;
    char label[32];
    snprintf(label, sizeof label, "conv%dx%d_s%d", KH, KW, stride);
    taps_split_launch(g, x, w, dc, B, Cin, Cout, in_scale, in_shift, in_relu, ws, label, (hipStream_t)stream,
                      w_ready != 0, epi);
    SCAT_LAUNCH_CHECK("scat_conv2d_fwd_split");
    return SCAT_OK;
}

extern "C" int64_t scat_conv7x7_s2_fwd_split_ws(int Cout) { return (int64_t)12 * 3 * Cout * 32; }

// The ResNet stem (models/resnet.py:105: Conv2d(3, 64, 7, stride 2, padding 3, bias=False)) on split-operand products:
// y[B,Cout,OH,OW] = conv(x[B,3,H,W], w[Cout,3,7,7]).  ws: scat_conv7x7_s2_fwd_split_ws(Cout) bytes.
extern "C" int scat_conv7x7_s2_fwd_split(const float* x, const float* w, float* y, int B, int H, int W, int Cout,
                                         void* ws, int64_t ws_bytes, ScatEpilogue* epi, void* stream) {
    if (epi) epi->groups = 0;
    SCAT_REQUIRE(x && w && y, SCAT_E_ARG, "scat_conv7x7_s2_fwd_split: null pointer");
    SCAT_REQUIRE(math_mode() == 1, SCAT_E_ARG, "scat_conv7x7_s2_fwd_split: needs the split-operand product mode");
    SCAT_REQUIRE(B > 0 && H > 6 && W > 6 && Cout > 0, SCAT_E_SHAPE, "scat_conv7x7_s2_fwd_split: bad dimension");
    SCAT_REQUIRE(ws && ws_bytes >= scat_conv7x7_s2_fwd_split_ws(Cout) && ((uintptr_t)ws & 15) == 0, SCAT_E_WORKSPACE,
                 "scat_conv7x7_s2_fwd_split: workspace too small / unaligned");
    const int OH = (H + 6 - 7) / 2 + 1, OW = (W + 6 - 7) / 2 + 1;
    SCAT_REQUIRE(fits_i32((int64_t)B * 3 * H * W * 4) && fits_i32((int64_t)B * Cout * OH * OW * 4), SCAT_E_SHAPE,
                 "scat_conv7x7_s2_fwd_split: tensor exceeds 32-bit byte offsets");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(stem_wprep_kernel, dim3(cdiv(12 * Cout * 16, 256)), dim3(256), 0, st, w, (uint16_t*)ws, Cout);
    PwDesc d{};
    d.src = x; d.w = (const float*)ws; d.C = 192; d.M = Cout; d.HW = H * W; d.npix = B * OH * OW;
    d.dHW = FastDiv::make(d.HW);
    d.ntap = 1; d.KWt = 1; d.a = 1; d.tb = 1; d.c0y = 0; d.c0x = 0; d.H = H; d.W = W; d.OW = OW; d.OHW = OH * OW;
    d.dOHW = FastDiv::make(d.OHW); d.dOW = FastDiv::make(OW);
    d.nsrc = (int64_t)B * 3 * H * W; d.nw = ((int64_t)12 * 3 * Cout * 32 + 3) / 4;
    d.variant = tuning();
    OutDesc dc{};
    dc.p = y; dc.mode = 1; dc.I = Cout; dc.J = d.npix; dc.C = Cout; dc.HW = OH * OW; dc.dHW = FastDiv::make(OH * OW);
    dc.n = (int64_t)B * Cout * OH * OW;
    const int cfg = Cout > 64 ? 0 : 1;
    set_kernel_label("conv7x7_s2_split_%sx32", pw_tile_name(cfg));
    launch_pw_split_cfg<false, true>(cfg, false, d, dc, st, epi);
    SCAT_LAUNCH_CHECK("scat_conv7x7_s2_fwd_split");
    return SCAT_OK;
}

// Data gradient of a 1x1/stride-1 convolution whose output gradient is a BatchNorm backward that was never
// materialised: dx[B,Cin,HW] (+)= w^T . (ca*g + cb*z + cc), g = masked incoming gradient [B,Cout,HW] (written by
// scat_bn_bwd_pre), z = the conv's raw output [B,Cout,HW], coef3 = [ca | cb | cc] per output channel.
// Split-operand products only; Cout % 16 == 0.  ws: scat_conv1x1_s1_ws(Cin, Cout) bytes.
extern "C" int scat_conv1x1_s1_bnb(const float* g, const float* z, const float* coef3, const float* w, float* dx, int B,
                                   int Cin, int HW, int Cout, int accumulate, void* ws, int64_t ws_bytes,
                                   int w_ready, void* stream) {
    SCAT_REQUIRE(g && z && coef3 && w && dx, SCAT_E_ARG, "scat_conv1x1_s1_bnb: null pointer");
    SCAT_REQUIRE(math_mode() == 1, SCAT_E_ARG, "scat_conv1x1_s1_bnb: needs the split-operand product mode");
    SCAT_REQUIRE(B > 0 && Cin > 0 && HW > 0 && Cout > 0 && Cout % 16 == 0, SCAT_E_SHAPE,
                 "scat_conv1x1_s1_bnb: bad dimension (Cout must be a multiple of 16)");
    SCAT_REQUIRE(ws && ws_bytes >= taps_split_ws(Cin, Cout, 1) && ((uintptr_t)ws & 15) == 0, SCAT_E_WORKSPACE,
                 "scat_conv1x1_s1_bnb: workspace too small / unaligned");
    SCAT_REQUIRE(fits_i32((int64_t)B * Cout * HW * 4) && fits_i32((int64_t)B * Cin * HW * 4), SCAT_E_SHAPE,
                 "scat_conv1x1_s1_bnb: tensor exceeds 32-bit byte offsets");
    hipStream_t st = (hipStream_t)stream;
    const int C = Cout, M = Cin;
    PwDesc d = pw_desc(B, C, HW, M);
    d.src = g; d.src2 = z; d.coef = coef3;
    const int64_t nel = (int64_t)M * ((C + 15) / 16 * 16);
    if (!w_ready) wprep_launch(wprep_job(w, ws, M, C, 1, 1, 1, 1, 1, 0, 0, 1), st);
    d.w = (const float*)ws;
    d.nw = (nel * 6 + 3) / 4;
    OutDesc dc{};
    dc.p = dx; dc.mode = 1; dc.I = M; dc.J = d.npix; dc.C = M; dc.HW = HW; dc.dHW = FastDiv::make(HW);
    dc.accumulate = accumulate; dc.n = (int64_t)B * M * HW;
    const int cfg = M > 64 ? 0 : 1;
    set_kernel_label("conv1x1_split_%sx32_bnb", pw_tile_name(cfg));
    launch_pw_split_cfg<true>(cfg, false, d, dc, st);
    SCAT_LAUNCH_CHECK("scat_conv1x1_s1_bnb");
    return SCAT_OK;
}

extern "C" int64_t scat_conv1x1_s1_ws(int M, int C) { return (int64_t)M * ((C + 15) / 16 * 16) * 6; }

// dst[B,M,HW] (+)= A[M,C] . f(src[B,C,HW]),  f = relu(x*scale+shift) when scale is given.
//   transposed = 0, forward:        w = [M][C]  (M = Cout, C = Cin)
//   transposed = 1, data gradient:  w = [C][M]  (the forward weight; M = Cin, C = Cout), src = dy
// ws: scat_conv1x1_s1_ws(M, C) bytes (the weights' bf16 terms, or their fp32 transpose).
// Needs C % 16 == 0 and 16-B aligned w/src; callers fall back to scat_conv2d_fwd / scat_conv2d_dgrad otherwise.
extern "C" int scat_conv1x1_s1(const float* src, const float* w, float* dst, int B, int C, int HW, int M,
                               int transposed, const float* bias, const float* in_scale, const float* in_shift,
                               int in_relu, int accumulate, void* ws, int64_t ws_bytes, int w_ready, ScatEpilogue* epi,
                               void* stream) {
    if (epi) epi->groups = 0;
    SCAT_REQUIRE(src && w && dst, SCAT_E_ARG, "scat_conv1x1_s1: null pointer");
    SCAT_REQUIRE(!w_ready || math_mode() == 1, SCAT_E_ARG, "scat_conv1x1_s1: prepared weights exist for split products only");
    SCAT_REQUIRE(ws && ws_bytes >= scat_conv1x1_s1_ws(M, C), SCAT_E_WORKSPACE, "scat_conv1x1_s1: workspace too small");
    SCAT_REQUIRE(B > 0 && C > 0 && HW > 0 && M > 0, SCAT_E_SHAPE, "scat_conv1x1_s1: non-positive dimension");
    SCAT_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), SCAT_E_ARG, "scat_conv1x1_s1: scale/shift pair");
    SCAT_REQUIRE(C % 16 == 0, SCAT_E_SHAPE, "scat_conv1x1_s1: channels must be a multiple of 16");
    SCAT_REQUIRE(((uintptr_t)w & 15) == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)ws & 15) == 0, SCAT_E_ARG,
                 "scat_conv1x1_s1: 16-B alignment");
    SCAT_REQUIRE(!in_scale || (((uintptr_t)in_scale & 15) == 0 && ((uintptr_t)in_shift & 15) == 0), SCAT_E_ARG,
                 "scat_conv1x1_s1: scale/shift must be 16-B aligned");
    SCAT_REQUIRE(fits_i32((int64_t)B * C * HW * 4) && fits_i32((int64_t)B * M * HW * 4) && fits_i32((int64_t)M * C * 4),
                 SCAT_E_SHAPE, "scat_conv1x1_s1: tensor exceeds 32-bit byte offsets");
    hipStream_t st = (hipStream_t)stream;
    PwDesc d = pw_desc(B, C, HW, M);
    d.src = src; d.w = w; d.scale = in_scale; d.shift = in_shift; d.relu = in_scale ? in_relu : 0;
    d.nw = (int64_t)M * C;
    OutDesc dc{};
    dc.p = dst; dc.mode = 1; dc.I = M; dc.J = d.npix; dc.C = M; dc.HW = HW; dc.dHW = FastDiv::make(HW);
    dc.bias = bias; dc.bias_mode = bias ? 1 : 0; dc.accumulate = accumulate; dc.n = (int64_t)B * M * HW;
    auto tiles = [&](int bm, int bn) { return (int64_t)cdiv(M, bm) * cdiv(d.npix, bn); };
    int cfg = (M > 64 && tiles(128, 128) >= 1024) ? 0 : 2;   // measured: 64x128 never wins at batch 96
    if (tuning() >= 1 && tuning() <= 3) cfg = tuning() - 1;
    const int64_t nel = (int64_t)M * ((C + 15) / 16 * 16);
    const int rblocks = (int)((nel + 255) / 256 < 2048 ? (nel + 255) / 256 : 2048);
    if (math_mode() == 1) {
        if (!w_ready) wprep_launch(wprep_job(w, ws, M, C, transposed, 1, 1, 1, 1, 0, 0, 1), st);
        d.w = (const float*)ws;
        d.nw = (nel * 6 + 3) / 4;
        if (!(tuning() >= 1 && tuning() <= 3)) {
            static const int thin = diag_env_int("SCAT_PW_THIN", 0);
            cfg = M > 64 ? 0 : 1;   // measured at batch 96: 64x64 never wins
            if (cfg == 0 && tiles(128, 128) < thin) cfg = 1;          // (SCAT_PW_THIN: 64x128 below that many tiles)
        }
        int pc = pc_mode();
        // default (SCAT_PC unset): the 8-consumer producer/consumer form for the few layers whose 128x128 tile count is
        // just over one tile per CU (294-296 tiles at batch 96: 1024->256 @14x14 forward, 256->1024 @14x14 and
        // 1024->2048 @7x7 data gradients) — there the round-1 kernel runs 38 CUs with two workgroups and 218 with one,
        // and one 256x128 workgroup per CU is 10-15 % faster (profiles/r02_conv_shapes.txt); everywhere else the
        // round-1 form wins.  The 64-wide tile counts are batch dependent, the rule is not.
        if (pc < 0) pc = (cfg == 0 && M >= 256 && tiles(128, 128) >= 257 && tiles(128, 128) < 330) ? 6 : 0;
        // wide form: pointwise, whole pixel quads inside one image, 16-byte aligned planes, NCHW output
        const bool w4ok = HW % 4 == 0 && ((uintptr_t)dst & 15) == 0 && (!bias || dc.bias_mode == 1);
        if (cfg == 0 && (pc == 5 || pc == 6) && M >= 256) {
            const bool wide = pc == 6 && w4ok;
            set_kernel_label("conv1x1_split_pc%s256x128x32%s", wide ? "4_" : "8w_", in_scale ? "_tf" : "");
            if (wide) {
                if (in_scale) launch_pw_pc<true, true>(d, dc, st); else launch_pw_pc<false, true>(d, dc, st);
            } else {
                if (in_scale) launch_pw_pc<true, false>(d, dc, st); else launch_pw_pc<false, false>(d, dc, st);
            }
            SCAT_LAUNCH_CHECK("scat_conv1x1_s1");
            return SCAT_OK;
        }
        set_kernel_label("conv1x1_split_%sx32%s", pw_tile_name(cfg), in_scale ? "_tf" : "");
        launch_pw_split_cfg(cfg, in_scale != nullptr, d, dc, st, epi);
        SCAT_LAUNCH_CHECK("scat_conv1x1_s1");
        return SCAT_OK;
    }
    if (transposed) {
        hipLaunchKernelGGL(w1x1_t_kernel, dim3(rblocks), dim3(256), 0, st, w, (float*)ws, M, C);
        d.w = (const float*)ws;
    }
    const bool v4 = HW % 4 == 0;
    set_kernel_label("conv1x1_pw_%sx32%s%s", pw_tile_name(cfg), v4 ? "_b4" : "", in_scale ? "_tf" : "");
    if (v4) {
        if (in_scale) launch_pw_cfg<true, true>(cfg, d, dc, st);
        else launch_pw_cfg<true, false>(cfg, d, dc, st);
    } else {
        if (in_scale) launch_pw_cfg<false, true>(cfg, d, dc, st);
        else launch_pw_cfg<false, false>(cfg, d, dc, st);
    }
    SCAT_LAUNCH_CHECK("scat_conv1x1_s1");
    return SCAT_OK;
}

// ---------------------------------------------------------------- dense GEMM on the pointwise split kernel
//
// C[M][N] (+)= op(A)[M][K] . B[K][N] (+ bias[N]); B and C row-major, A either [M][K] (a_transposed = 0) or stored
// [K][M] (a_transposed = 1).  This IS the pointwise convolution above with one image: A plays the weights (split once
// into MFMA operand planes by the re-layout launch: ws), B the activations [K channels][N pixels] that are split on
// their way into LDS, C the NCHW output [1][M][N].  It puts the ViT projections (vision_transformer.py:46-79:
// x.Wqkv^T, attn.Wout^T and their gradients, M = 2016 tokens at batch 96) on split-operand products:
//   forward   y  = x . W^T      A = x [M][K],             B = W^T [K][N] (scat_transpose2d of the weight)
//   dgrad     dx = dy . W       A = dy [M][N'],           B = W [N'][K'] as stored
//   wgrad     dW = dy^T . x     A = dy, a_transposed = 1, B = x [tokens][K] as stored
// K need not be a multiple of 16 (the re-layout pads A, the activation loads mask the ragged channels).
extern "C" int64_t scat_gemm_split_ws(int M, int K) { return taps_split_ws(M, K, 1); }

extern "C" int scat_gemm_split(const float* a, int a_transposed, const float* b, float* c, int M, int N, int K,
                               const float* bias_n, int accumulate, void* ws, int64_t ws_bytes, void* stream) {
    SCAT_REQUIRE(a && b && c, SCAT_E_ARG, "scat_gemm_split: null pointer");
    SCAT_REQUIRE(M > 0 && N > 0 && K > 0, SCAT_E_SHAPE, "scat_gemm_split: non-positive dimension");
    SCAT_REQUIRE(math_mode() == 1, SCAT_E_ARG, "scat_gemm_split: needs the split-operand product mode");
    SCAT_REQUIRE(ws && ws_bytes >= scat_gemm_split_ws(M, K) && ((uintptr_t)ws & 15) == 0, SCAT_E_WORKSPACE,
                 "scat_gemm_split: workspace too small / unaligned");
    SCAT_REQUIRE(fits_i32((int64_t)K * N * 4) && fits_i32((int64_t)M * N * 4) && fits_i32((int64_t)M * K * 4),
                 SCAT_E_SHAPE, "scat_gemm_split: operand exceeds 32-bit byte offsets");
    hipStream_t st = (hipStream_t)stream;
    wprep_launch(wprep_job(a, ws, M, K, a_transposed, 1, 1, 1, 1, 0, 0, 1), st);
    PwDesc d = pw_desc(1, K, N, M);
    d.src = b;
    const int64_t nel = (int64_t)M * ((K + 15) / 16 * 16);
    d.w = (const float*)ws;
    d.nw = (nel * 6 + 3) / 4;
    OutDesc dc{};
    dc.p = c; dc.mode = 1; dc.I = M; dc.J = N; dc.C = M; dc.HW = N; dc.dHW = FastDiv::make(N);
    dc.bias = bias_n; dc.bias_mode = bias_n ? 2 : 0; dc.accumulate = accumulate; dc.n = (int64_t)M * N;
    // few, small problems (2016 x 1536 x 784 is the largest): the tile is chosen for workgroup count first
    auto tiles = [&](int bm, int bn) { return (int64_t)cdiv(M, bm) * cdiv(N, bn); };
    int cfg = tiles(128, 128) >= 512 ? 0 : (tiles(64, 128) >= 512 ? 1 : 2);
    if (tuning() >= 1 && tuning() <= 3) cfg = tuning() - 1;
    set_kernel_label("gemm_split_%sx32", pw_tile_name(cfg));
    launch_pw_split_cfg(cfg, false, d, dc, st);
    SCAT_LAUNCH_CHECK("scat_gemm_split");
    return SCAT_OK;
}

// dst[C][R] = src[R][C] (row-major): the weight transpose of the forward projection above
__global__ __launch_bounds__(256) void transpose2d_kernel(const float* __restrict__ src, float* __restrict__ dst, int R,
                                                          int C) {
    __shared__ float tile[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + ty + 8 * k, cc = c0 + tx;
        tile[ty + 8 * k][tx] = (r < R && cc < C) ? src[(int64_t)r * C + cc] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int cc = c0 + ty + 8 * k, r = r0 + tx;
        if (cc < C && r < R) dst[(int64_t)cc * R + r] = tile[tx][ty + 8 * k];
    }
}

extern "C" int scat_transpose2d(const float* src, float* dst, int R, int C, void* stream) {
    SCAT_REQUIRE(src && dst && R > 0 && C > 0, SCAT_E_ARG, "scat_transpose2d: bad argument");
    hipLaunchKernelGGL(transpose2d_kernel, dim3(cdiv(C, 32), cdiv(R, 32)), dim3(256), 0, (hipStream_t)stream, src, dst,
                       R, C);
    SCAT_LAUNCH_CHECK("scat_transpose2d");
    return SCAT_OK;
}
