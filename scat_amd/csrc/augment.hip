// On-device sample augmentation (dataset/load_STB.py:252-294, dataset/rotation.py:7-55): mirror, motion blur, rotation
// onto the enlarged canvas, the crop around the hand and the resize to 224 x 224, with the matching label changes.
//
// Two launches per batch:
//   augment_plan_kernel     one wavefront per sample: the labels in fp64 (the reference computes them in numpy float64)
//                           and a plan record that describes the sample's image map;
//   augment_warp_u8_kernel  one pass over the output: every output pixel is ONE composed map into the source frame
//                           (the reference resamples three times, rounding to uint8 in between: DESIGN.md section 8).
//
// Plan record, SCAT_AUGMENT_PLAN_FLOATS (24) floats = 96 bytes per sample, 8-byte aligned:
//   floats  0..11   six fp64 values (bit patterns) A00 A01 A02 A10 A11 A12: for the output position p = ox + (sx+.5)/n,
//                   q = oy + (sy+.5)/n the source point is x = A00 p + A01 q + A02, y = A10 p + A11 q + A12, i.e.
//                   M^-1 composed with u = L + p nw/224 - .5, v = T + q nh/224 - .5
//   floats 12..15   L, T, nw, nh    the crop box PIL makes of (left, top, right, bottom): integers, stored as floats
//   float  16       n               side of the box pre-filter grid, 1..4
//   floats 17..19   flip, k, vert   mirror (0/1), blur length (0 = none, 1..10), blur direction (1 = vertical)
//   floats 20..23   zero
#include "common.h"

#include <math.h>

namespace scat {

constexpr int kPlanFloats = 24;
constexpr int kOut = 224;          // the plan's map and the 2-D labels are composed for this output size
constexpr int kMaxBlur = 10;
constexpr int kMaxGrid = 4;

__device__ __forceinline__ double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// grid = B, block = 64 (one wavefront); lanes 0..20 hold joint `lane`
__global__ __launch_bounds__(64) void augment_plan_kernel(const float* __restrict__ j2d, const float* __restrict__ j3d,
                                                          const int32_t* __restrict__ params, float* __restrict__ labels,
                                                          float* __restrict__ plan, int W, int H, int normalize_3d) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const bool act = lane < 21;
    const int j = act ? lane : 0;
    const float* p2 = j2d + (int64_t)b * 42;
    const float* p3 = j3d + (int64_t)b * 63;
    const int32_t* pr = params + (int64_t)b * 4;
    // drawn parameters, held to their ranges: a bad record must not turn into a wild loop count in the warp
    const int flip = pr[0] != 0;
    const int k = min(max(pr[1], 0), kMaxBlur);
    const int vert = pr[2] != 0;
    const int angle = min(max(pr[3], 0), 360);

    double x2 = p2[j * 2], y2 = p2[j * 2 + 1];
    double x3 = p3[j * 3], y3 = p3[j * 3 + 1], z3 = p3[j * 3 + 2];

    if (normalize_3d) {   // rescale_3d_joints_flip, load_STB.py:98-110
        double dx = (double)p3[12] - (double)p3[15], dy = (double)p3[13] - (double)p3[16], dz = (double)p3[14] - (double)p3[17];
        double sc = 0.03058954 / sqrt(dx * dx + dy * dy + dz * dz);
        double rx = -((double)p3[3] * sc), ry = (double)p3[4] * sc, rz = (double)p3[5] * sc;   // joint 1 after scale and sign
        x3 = -(x3 * sc) - rx;
        y3 = y3 * sc - ry;
        z3 = z3 * sc - rz;
    }
    if (flip) x2 = (double)W - x2;   // hand_flip, load_STB.py:69-74: W - x, not W - 1 - x

    // rotate_img, rotation.py:11-45; M maps the frame onto the enlarged canvas, (ia ib / ic id | itx ity) is its inverse
    double nW = W, nH = H;
    double ia = 1.0, ib = 0.0, itx = 0.0, ity = 0.0;
    if (angle) {
        const double rad = (double)angle * (3.14159265358979323846 / 180.0);
        const double a = cos(rad), bb = sin(rad);
        const double cx = W / 2, cy = H / 2;
        double m02 = (1.0 - a) * cx - bb * cy, m12 = bb * cx + (1.0 - a) * cy;   // cv2.getRotationMatrix2D
        nW = (double)(int)(H * fabs(bb) + W * fabs(a));
        nH = (double)(int)(H * fabs(a) + W * fabs(bb));
        m02 += nW / 2 - cx;
        m12 += nH / 2 - cy;
        const double nx = a * x2 + bb * y2 + m02, ny = -bb * x2 + a * y2 + m12;
        x2 = nx;
        y2 = ny;
        const double n3x = a * x3 + bb * y3, n3y = -bb * x3 + a * y3;   // M_3d, rotation.py:39-45; z untouched
        x3 = n3x;
        y3 = n3y;
        // inverse of [R | t] with R = [[a, b], [-b, a]]: R^T, -R^T t
        ia = a;
        ib = -bb;
        itx = -(a * m02 - bb * m12);
        ity = -(bb * m02 + a * m12);
    }

    // crop_hand, load_STB.py:76-96
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const double mnx = fmax(wave_min(act ? x2 : inf), 0.0), mny = fmax(wave_min(act ? y2 : inf), 0.0);
    const double mxx = fmin(wave_max(act ? x2 : -inf), nW), mxy = fmin(wave_max(act ? y2 : -inf), nH);
    const double cx2 = __shfl(x2, 4, 64), cy2 = __shfl(y2, 4, 64);
    double s = fmax(1.3 * fmax(mxx - cx2, cx2 - mnx), 1.3 * fmax(mxy - cy2, cy2 - mny));
    s = fmin(fmax(s, 10.0), 500.0);
    const double l = cx2 - s, t = cy2 - s, r = cx2 + s, bt = cy2 + s;
    // Image.crop rounds the box half to even
    const double L = rint(l), T = rint(t), R = rint(r), Bt = rint(bt);
    const double nw = R - L, nh = Bt - T;
    const double sc2 = (double)kOut / nw;   // the un-rounded origin and nw serve both axes, as in the reference
    x2 = (x2 - l) * sc2;
    y2 = (y2 - t) * sc2;

    if (act) {
        float* lab = labels + (int64_t)b * 105;
        lab[j * 3] = (float)x3;
        lab[j * 3 + 1] = (float)y3;
        lab[j * 3 + 2] = (float)z3;
        lab[63 + j * 2] = (float)x2;
        lab[63 + j * 2 + 1] = (float)y2;
    }
    if (lane == 0) {
        float* rec = plan + (int64_t)b * kPlanFloats;
        double* A = reinterpret_cast<double*>(rec);
        const double sx = nw / kOut, sy = nh / kOut, u0 = L - 0.5, v0 = T - 0.5;
        // M^-1 = [[ia, ib, itx], [-ib, ia, ity]]
        A[0] = ia * sx;
        A[1] = ib * sy;
        A[2] = ia * u0 + ib * v0 + itx;
        A[3] = -ib * sx;
        A[4] = ia * sy;
        A[5] = -ib * u0 + ia * v0 + ity;
        int n = (int)floor(nw / kOut + 0.5);
        n = min(max(n, 1), kMaxGrid);
        rec[12] = (float)L;
        rec[13] = (float)T;
        rec[14] = (float)nw;
        rec[15] = (float)nh;
        rec[16] = (float)n;
        rec[17] = (float)flip;
        rec[18] = (float)k;
        rec[19] = (float)vert;
        rec[20] = rec[21] = rec[22] = rec[23] = 0.f;
    }
}

// cv2's BORDER_REFLECT_101 for an offset of at most kMaxBlur / 2 beyond an axis of n >= 11 points; the last clamp cannot
// bind on such input and keeps every address inside the frame whatever the plan record holds
__device__ __forceinline__ int reflect101(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

// grid = (49 tiles, B), block = 256: a tile is 32 output columns x 32 rows, a thread four consecutive columns of one row,
// a wavefront 32 columns x 8 rows.  HWC: a source pixel's three bytes are adjacent.
template <bool HWC>
__global__ __launch_bounds__(256) void augment_warp_u8_kernel(const uint8_t* __restrict__ src, const float* __restrict__ plan,
                                                              float* __restrict__ dst, int SH, int SW) {
    const int b = blockIdx.y;
    const float* rec = plan + (int64_t)b * kPlanFloats;   // block-uniform: scalar loads
    const double* A = reinterpret_cast<const double*>(rec);
    const double a00 = A[0], a01 = A[1], a02 = A[2], a10 = A[3], a11 = A[4], a12 = A[5];
    const int n = min(max((int)rec[16], 1), kMaxGrid);
    const bool flip = rec[17] != 0.f;
    const int kr = min(max((int)rec[18], 0), kMaxBlur);
    const bool vert = rec[19] != 0.f;
    // k = 0 (no blur) and k = 1 are the same single tap
    const int k = max(kr, 1), ka = k / 2, km = (k - 1) / 2;
    const int fix = km - ka;                  // offset across the blur direction: -1 for an even k (cv2's anchor)

    const int tile = blockIdx.x, tx = tile % 7, ty = tile / 7;
    const int ox0 = tx * 32 + (threadIdx.x & 7) * 4, oy = ty * 32 + (threadIdx.x >> 3);

    const int64_t plane = (int64_t)SH * SW;
    const uint8_t* img = src + (int64_t)b * 3 * plane;
    const int cs = HWC ? 1 : (int)plane;      // channel stride, pixel stride (both fit: the host checked 3*SH*SW)
    const int ps = HWC ? 3 : 1;

    float acc[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = acc[i][2] = 0.f;

    const double inv_n = 1.0 / n;
    for (int sy = 0; sy < n; ++sy) {
        const double q = oy + (sy + 0.5) * inv_n;
        for (int sx = 0; sx < n; ++sx) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double p = (ox0 + i) + (sx + 0.5) * inv_n;
                // fp64 here: at x = 640 one fp32 ulp is 6e-5 of a pixel, which a random frame turns into output error
                double x = a00 * p + a01 * q + a02, y = a10 * p + a11 * q + a12;
                x = fmin(fmax(x, -2.0), (double)SW + 1.0);
                y = fmin(fmax(y, -2.0), (double)SH + 1.0);
                const double xf = floor(x), yf = floor(y);
                const float wx = (float)(x - xf), wy = (float)(y - yf);
                const int x0 = (int)xf, y0 = (int)yf;
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) {
                    const int px = x0 + (c4 & 1), py = y0 + (c4 >> 1);
                    const bool in = px >= 0 && px < SW && py >= 0 && py < SH;   // outside the frame: black
                    float w = ((c4 & 1) ? wx : 1.f - wx) * ((c4 >> 1) ? wy : 1.f - wy);
                    w = in ? w : 0.f;
                    const int pxc = min(max(px, 0), SW - 1), pyc = min(max(py, 0), SH - 1);
                    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
                    for (int t = 0; t < k; ++t) {
                        int xs = reflect101(pxc + (vert ? fix : t - ka), SW);
                        const int ys = reflect101(pyc + (vert ? t - ka : fix), SH);
                        xs = flip ? SW - 1 - xs : xs;
                        const uint8_t* g = img + (ys * SW + xs) * ps;
                        s0 += (float)g[0];
                        s1 += (float)g[cs];
                        s2 += (float)g[2 * cs];
                    }
                    acc[i][0] += w * s0;
                    acc[i][1] += w * s1;
                    acc[i][2] += w * s2;
                }
            }
        }
    }
    const float norm = 1.f / (127.5f * (float)(k * n * n));
    float* out = dst + (((int64_t)b * 3) * kOut + oy) * kOut + ox0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        // the four weights sum to 1 only to an fp32 rounding: hold a saturated patch to the stated range
        float4 v = make_float4(fminf(acc[0][c] * norm - 1.f, 1.f), fminf(acc[1][c] * norm - 1.f, 1.f),
                               fminf(acc[2][c] * norm - 1.f, 1.f), fminf(acc[3][c] * norm - 1.f, 1.f));
        *reinterpret_cast<float4*>(out + (int64_t)c * kOut * kOut) = v;   // default cache policy: the stem reads it next
    }
}

}  // namespace scat

using namespace scat;

extern "C" int scat_augment_plan(const float* j2d, const float* j3d, const int32_t* params, float* labels, float* plan, int B,
                                 int W, int H, int normalize_3d, void* stream) {
    SCAT_REQUIRE(j2d && j3d && params && labels && plan, SCAT_E_ARG, "scat_augment_plan: null pointer");
    SCAT_REQUIRE(B > 0, SCAT_E_SHAPE, "scat_augment_plan: batch %d must be positive", B);
    SCAT_REQUIRE(W >= 11 && H >= 11 && W <= 16384 && H <= 16384, SCAT_E_SHAPE,
                 "scat_augment_plan: frame %d x %d outside 11..16384", W, H);
    SCAT_REQUIRE(normalize_3d == 0 || normalize_3d == 1, SCAT_E_ARG, "scat_augment_plan: normalize_3d must be 0 or 1");
    SCAT_REQUIRE(((uintptr_t)plan & 7) == 0, SCAT_E_ARG, "scat_augment_plan: plan must be 8-byte aligned");
    hipLaunchKernelGGL(augment_plan_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, j2d, j3d, params, labels, plan, W, H,
                       normalize_3d);
    SCAT_LAUNCH_CHECK("scat_augment_plan");
    set_kernel_label("augment_plan");
    return SCAT_OK;
}

extern "C" int scat_augment_warp_u8(const uint8_t* src, const float* plan, float* dst, int B, int SH, int SW, int OH, int OW,
                                    int hwc, void* stream) {
    SCAT_REQUIRE(src && plan && dst, SCAT_E_ARG, "scat_augment_warp_u8: null pointer");
    SCAT_REQUIRE(B > 0 && B <= 65535, SCAT_E_SHAPE, "scat_augment_warp_u8: batch %d outside 1..65535", B);
    SCAT_REQUIRE(OH == OW && OH == kOut, SCAT_E_SHAPE,
                 "scat_augment_warp_u8: output %d x %d unsupported (the plan is composed for %d x %d)", OH, OW, kOut, kOut);
    // the blur's reflected border reaches 5 pixels beyond an edge
    SCAT_REQUIRE(SH >= 11 && SW >= 11 && SH <= 16384 && SW <= 16384, SCAT_E_SHAPE,
                 "scat_augment_warp_u8: source %d x %d outside 11..16384", SH, SW);
    SCAT_REQUIRE(hwc == 0 || hwc == 1, SCAT_E_ARG, "scat_augment_warp_u8: hwc must be 0 or 1");
    SCAT_REQUIRE(((uintptr_t)plan & 7) == 0 && ((uintptr_t)dst & 15) == 0, SCAT_E_ARG,
                 "scat_augment_warp_u8: plan must be 8-byte and dst 16-byte aligned");
    dim3 grid((kOut / 32) * (kOut / 32), B);
    if (hwc)
        hipLaunchKernelGGL(augment_warp_u8_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, src, plan, dst, SH, SW);
    else
        hipLaunchKernelGGL(augment_warp_u8_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, src, plan, dst, SH, SW);
    SCAT_LAUNCH_CHECK("scat_augment_warp_u8");
    set_kernel_label("augment_warp_u8_%s", hwc ? "hwc" : "chw");
    return SCAT_OK;
}
