// On-device mesh and skeleton renderer (include/scat_render.h): projection with vertex normals, a tiled exact-coverage
// rasteriser with Lambert shading, and a joints-and-bones overlay.  Semantics and the reference lines: the header.
#include "common.h"

#include "../../include/scat_render.h"

namespace scat {
namespace {

constexpr int kRMaxV = SCAT_RENDER_MAX_V;
constexpr int kRMaxF = SCAT_RENDER_MAX_F;
constexpr int kRMaxHW = SCAT_RENDER_MAX_HW;
constexpr int kRMaxL = SCAT_RENDER_MAX_LIGHTS;
constexpr int kRMaxJ = SCAT_RENDER_MAX_J;
constexpr int kRMaxB = SCAT_RENDER_MAX_BONES;
constexpr int kPW = SCAT_RENDER_PROJ_WORDS;
constexpr int kSnapLimit = SCAT_RENDER_SNAP_LIMIT;
constexpr int kProjThreads = 512;
constexpr int kTile = 16;
constexpr int kRasterThreads = kTile * kTile;      // one thread per pixel of the tile, one face per thread of a chunk
constexpr int kSkelThreads = 256;

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// One fp32 operation, rounded to nearest on its own: never contracted with a neighbour into a fused multiply-add, so that
// a numpy fp32 restatement gives the same bits (the exact coverage rests on it).
__device__ __forceinline__ float mul_rn(float x, float y) {
#pragma clang fp contract(off)
    return x * y;
}
__device__ __forceinline__ float add_rn(float x, float y) {
#pragma clang fp contract(off)
    return x + y;
}

// ------------------------------------------------------------------------------------------------ projection
// One workgroup per sample.  Pass 1: every vertex into LDS with its snapped coordinates and validity.  Pass 2: the
// vertex normals from LDS (a face counts only if its three vertices are valid), and the eight words of the vertex.
__global__ __launch_bounds__(kProjThreads) void render_project_kernel(const float* __restrict__ verts,
                                                                      const float* __restrict__ cam,
                                                                      const int32_t* __restrict__ faces,
                                                                      const int32_t* __restrict__ vf_off,
                                                                      const int32_t* __restrict__ vf_idx,
                                                                      int32_t* __restrict__ proj, int V, int F, float hw,
                                                                      float hh) {
    __shared__ float s_v[kRMaxV * 3];
    __shared__ int32_t s_xy[kRMaxV * 2];
    __shared__ uint8_t s_ok[kRMaxV];
    const int b = blockIdx.x;
    const float s = cam[b * 3 + 0], tx = cam[b * 3 + 1], ty = cam[b * 3 + 2];
    const float* vb = verts + (size_t)b * V * 3;
    for (int v = threadIdx.x; v < V; v += kProjThreads) {
        const float x = vb[v * 3 + 0], y = vb[v * 3 + 1], z = vb[v * 3 + 2];
        const float u = add_rn(mul_rn(mul_rn(s, add_rn(x, tx)), hw), hw);
        const float w = add_rn(mul_rn(mul_rn(s, add_rn(y, ty)), hh), hh);
        const float uf = mul_rn(u, 256.f), wf = mul_rn(w, 256.f);
        // |uf| <= 2^22 is decided in fp32 before the conversion (rint of a float of that size is exact), so that the
        // conversion never sees a value outside int32
        bool ok = finite_f(x) && finite_f(y) && finite_f(z) && finite_f(uf) && finite_f(wf);
        int X = 0, Y = 0;
        if (ok) {
            const float ru = rintf(uf), rw = rintf(wf);
            ok = fabsf(ru) <= (float)kSnapLimit && fabsf(rw) <= (float)kSnapLimit;
            if (ok) {
                X = (int)ru;
                Y = (int)rw;
            }
        }
        s_v[v * 3 + 0] = x;
        s_v[v * 3 + 1] = y;
        s_v[v * 3 + 2] = z;
        s_xy[v * 2 + 0] = X;
        s_xy[v * 2 + 1] = Y;
        s_ok[v] = ok ? 1 : 0;
    }
    __syncthreads();
    int32_t* pb = proj + (size_t)b * V * kPW;
    for (int v = threadIdx.x; v < V; v += kProjThreads) {
        const bool ok = s_ok[v] != 0;
        float nx = 0.f, ny = 0.f, nz = 0.f;
        if (ok) {
            int k0 = vf_off[v], k1 = vf_off[v + 1];
            k0 = max(k0, 0);
            k1 = min(k1, 3 * F);
            for (int k = k0; k < k1; ++k) {
                const int f = vf_idx[k];
                if (f < 0 || f >= F) continue;
                const int a = faces[f * 3 + 0], bb = faces[f * 3 + 1], c = faces[f * 3 + 2];
                if ((unsigned)a >= (unsigned)V || (unsigned)bb >= (unsigned)V || (unsigned)c >= (unsigned)V) continue;
                if (!(s_ok[a] && s_ok[bb] && s_ok[c])) continue;
                const float ax = s_v[a * 3], ay = s_v[a * 3 + 1], az = s_v[a * 3 + 2];
                const float ux = s_v[bb * 3] - ax, uy = s_v[bb * 3 + 1] - ay, uz = s_v[bb * 3 + 2] - az;
                const float wx = s_v[c * 3] - ax, wy = s_v[c * 3 + 1] - ay, wz = s_v[c * 3 + 2] - az;
                nx += uy * wz - uz * wy;
                ny += uz * wx - ux * wz;
                nz += ux * wy - uy * wx;
            }
        }
        const float len = sqrtf(nx * nx + ny * ny + nz * nz);
        if (ok && len > 0.f && finite_f(len)) {
            nx /= len;
            ny /= len;
            nz /= len;
        } else {
            nx = 0.f;
            ny = 0.f;
            nz = -1.f;
        }
        int32_t* p = pb + (size_t)v * kPW;
        p[0] = s_xy[v * 2 + 0];
        p[1] = s_xy[v * 2 + 1];
        p[2] = __float_as_int(ok ? s_v[v * 3 + 2] : 0.f);
        p[3] = __float_as_int(nx);
        p[4] = __float_as_int(ny);
        p[5] = __float_as_int(nz);
        p[6] = ok ? 1 : 0;
        p[7] = 0;
    }
}

// ------------------------------------------------------------------------------------------------ rasteriser
// A face that survived its chunk's test against the tile, oriented so that A > 0.  Edge i is the one opposite vertex i
// (0: 1->2, 1: 2->0, 2: 0->1); e[i] is its edge function at the centre of the tile's first pixel, so that at pixel
// (ii, jj) of the tile it is e[i] + 256 (dx[i] jj - dy[i] ii), a 32-bit product sum: |dx|, |dy| < 2^23, ii, jj < 16.
struct TileFace {
    int32_t dx[3], dy[3];
    int64_t e[3];
    float z[3];
    float area;
    int32_t fid;
    int32_t tie;      // bit i: a pixel centre exactly on edge i belongs to this face
};

struct FaceSetup {
    int32_t x[3], y[3];      // snapped, after the swap
    int32_t v[3];            // vertex indices, after the swap
    int64_t area;            // > 0
    bool back;
};

// the header's rules for one face; false: dropped
__device__ __forceinline__ bool face_setup(const int32_t* __restrict__ pb, const int32_t* __restrict__ faces, int f, int V,
                                           int cull, FaceSetup* s) {
    const int a = faces[f * 3 + 0], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
    if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)c >= (unsigned)V) return false;
    const int32_t *pa = pb + (size_t)a * kPW, *pbb = pb + (size_t)b * kPW, *pc = pb + (size_t)c * kPW;
    if (!(pa[6] && pbb[6] && pc[6])) return false;
    const int x0 = pa[0], y0 = pa[1], x1 = pbb[0], y1 = pbb[1], x2 = pc[0], y2 = pc[1];
    // a projected-vertex record from elsewhere could hold anything: keep the differences below 2^23 whatever it holds
    const auto wide = [](int v) { return (unsigned)v + (unsigned)kSnapLimit > 2u * (unsigned)kSnapLimit; };
    if (wide(x0) || wide(x1) || wide(x2) || wide(y0) || wide(y1) || wide(y2)) return false;
    const int64_t area = (int64_t)(x1 - x0) * (y2 - y0) - (int64_t)(y1 - y0) * (x2 - x0);
    if (area == 0) return false;
    if (area > 0 && cull) return false;
    s->x[0] = x0;
    s->y[0] = y0;
    s->v[0] = a;
    if (area < 0) {
        s->x[1] = x2, s->y[1] = y2, s->v[1] = c;
        s->x[2] = x1, s->y[2] = y1, s->v[2] = b;
        s->area = -area;
        s->back = false;
    } else {
        s->x[1] = x1, s->y[1] = y1, s->v[1] = b;
        s->x[2] = x2, s->y[2] = y2, s->v[2] = c;
        s->area = area;
        s->back = true;
    }
    return true;
}

__device__ __forceinline__ int64_t edge_at(int xa, int ya, int xb, int yb, int px, int py) {
    return (int64_t)(xb - xa) * (py - ya) - (int64_t)(yb - ya) * (px - xa);
}

__device__ __forceinline__ uint8_t to_level(float v) {
    v = fminf(fmaxf(v, 0.f), 1.f);
    return (uint8_t)(int)rintf(255.f * v);
}

struct RasterArgs {
    const int32_t* proj;
    const int32_t* faces;
    const uint8_t* img;
    int32_t* face_id;
    float* depth;
    uint8_t* rgb;
    int V, F, H, W, L, cull;
    float base[3], ambient;
};

__global__ __launch_bounds__(kRasterThreads) void render_raster_kernel(RasterArgs a, const float* __restrict__ lights) {
    __shared__ TileFace s_face[kRasterThreads];
    __shared__ int s_count[kRasterThreads / 64];
    __shared__ float s_light[kRMaxL][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z;
    const int tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
    const int ii = tid & (kTile - 1), jj = tid >> 4;
    const int px = tx0 + ii, py = ty0 + jj;
    const int32_t* pb = a.proj + (size_t)b * a.V * kPW;
    if (tid < a.L * 4) s_light[tid >> 2][tid & 3] = lights[tid];
    // pixel centres of the tile in snapped units: [cx0, cx1] x [cy0, cy1]
    const int cx0 = 256 * tx0 + 128, cy0 = 256 * ty0 + 128;
    const int cx1 = cx0 + 256 * (kTile - 1), cy1 = cy0 + 256 * (kTile - 1);

    int best = -1;
    float bz = __int_as_float(0x7f800000);
    for (int base = 0; base < a.F; base += kRasterThreads) {
        const int f = base + tid;
        FaceSetup fs;
        bool keep = f < a.F && face_setup(pb, a.faces, f, a.V, a.cull, &fs);
        if (keep) {
            const int xmin = min(min(fs.x[0], fs.x[1]), fs.x[2]), xmax = max(max(fs.x[0], fs.x[1]), fs.x[2]);
            const int ymin = min(min(fs.y[0], fs.y[1]), fs.y[2]), ymax = max(max(fs.y[0], fs.y[1]), fs.y[2]);
            keep = xmax >= cx0 && xmin <= cx1 && ymax >= cy0 && ymin <= cy1;
        }
        // compaction in face order: lanes of a wavefront by ballot, wavefronts by their counts
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_count[wave] = __popcll(m);
        __syncthreads();
        int slot = before, total = 0;
        for (int w = 0; w < kRasterThreads / 64; ++w) {
            const int c = s_count[w];
            if (w < wave) slot += c;
            total += c;
        }
        if (keep) {
            TileFace& t = s_face[slot];
            for (int i = 0; i < 3; ++i) {
                const int p = (i + 1) % 3, q = (i + 2) % 3;      // edge i runs p -> q
                const int dx = fs.x[q] - fs.x[p], dy = fs.y[q] - fs.y[p];
                t.dx[i] = dx;
                t.dy[i] = dy;
                t.e[i] = edge_at(fs.x[p], fs.y[p], fs.x[q], fs.y[q], cx0, cy0);
                t.z[i] = __int_as_float(pb[(size_t)fs.v[i] * kPW + 2]);
            }
            int tie = 0;
            for (int i = 0; i < 3; ++i)
                if (t.dy[i] > 0 || (t.dy[i] == 0 && t.dx[i] < 0)) tie |= 1 << i;
            t.tie = tie;
            t.area = (float)fs.area;
            t.fid = f;
        }
        __syncthreads();
        for (int k = 0; k < total; ++k) {
            const TileFace& t = s_face[k];      // every lane reads the same address: a broadcast
            const int64_t e0 = t.e[0] + ((int64_t)(t.dx[0] * jj - t.dy[0] * ii) << 8);
            const int64_t e1 = t.e[1] + ((int64_t)(t.dx[1] * jj - t.dy[1] * ii) << 8);
            const int64_t e2 = t.e[2] + ((int64_t)(t.dx[2] * jj - t.dy[2] * ii) << 8);
            const int tie = t.tie;
            const bool in = (e0 + (tie & 1)) > 0 && (e1 + ((tie >> 1) & 1)) > 0 && (e2 + ((tie >> 2) & 1)) > 0;
            if (in) {
                const float num = add_rn(add_rn(mul_rn((float)e0, t.z[0]), mul_rn((float)e1, t.z[1])),
                                            mul_rn((float)e2, t.z[2]));
                const float z = num / t.area;
                if (best < 0 || z < bz) {      // the list is in face order: an equal z keeps the lower index
                    best = t.fid;
                    bz = z;
                }
            }
        }
        __syncthreads();
    }
    if (px >= a.W || py >= a.H) return;
    const size_t pix = ((size_t)b * a.H + py) * a.W + px;
    a.face_id[pix] = best;
    a.depth[pix] = best < 0 ? __int_as_float(0x7f800000) : bz;
    if (!a.rgb) return;
    uint8_t* out = a.rgb + pix * 3;
    if (best < 0) {
        const uint8_t* in = a.img ? a.img + pix * 3 : nullptr;
        out[0] = in ? in[0] : 0;
        out[1] = in ? in[1] : 0;
        out[2] = in ? in[2] : 0;
        return;
    }
    FaceSetup fs;
    face_setup(pb, a.faces, best, a.V, a.cull, &fs);      // it passed once: the same answer
    const int cx = 256 * px + 128, cy = 256 * py + 128;
    const float area = (float)fs.area;
    float n[3] = {0.f, 0.f, 0.f};
    for (int i = 0; i < 3; ++i) {
        const int p = (i + 1) % 3, q = (i + 2) % 3;
        const float w = (float)edge_at(fs.x[p], fs.y[p], fs.x[q], fs.y[q], cx, cy) / area;
        const int32_t* pv = pb + (size_t)fs.v[i] * kPW;
        n[0] += w * __int_as_float(pv[3]);
        n[1] += w * __int_as_float(pv[4]);
        n[2] += w * __int_as_float(pv[5]);
    }
    const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (len > 0.f && finite_f(len)) {
        n[0] /= len, n[1] /= len, n[2] /= len;
    } else {
        n[0] = 0.f, n[1] = 0.f, n[2] = -1.f;
    }
    if (fs.back) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
    float shade = a.ambient;
    for (int l = 0; l < a.L; ++l) {
        const float d = n[0] * s_light[l][0] + n[1] * s_light[l][1] + n[2] * s_light[l][2];
        shade += s_light[l][3] * fmaxf(d, 0.f);
    }
    shade = fminf(shade, 1.f);
    out[0] = to_level(a.base[0] * shade);
    out[1] = to_level(a.base[1] * shade);
    out[2] = to_level(a.base[2] * shade);
}

// ------------------------------------------------------------------------------------------------ skeleton
__global__ __launch_bounds__(kSkelThreads) void render_skeleton_kernel(const float* __restrict__ j2d,
                                                                       const int32_t* __restrict__ bones,
                                                                       const uint8_t* __restrict__ colors,
                                                                       uint8_t* __restrict__ rgb, int J, int NB, int H, int W,
                                                                       float rb, float rj) {
    __shared__ float s_j[kRMaxJ][2];
    __shared__ int s_b[kRMaxB][2];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid < J * 2) s_j[tid >> 1][tid & 1] = j2d[(size_t)b * J * 2 + tid];
    if (tid < NB * 2) s_b[tid >> 1][tid & 1] = bones[tid];
    __syncthreads();
    const int p = blockIdx.x * kSkelThreads + tid;
    if (p >= H * W) return;
    const int j = p / W, i = p - j * W;
    const float cx = (float)i + 0.5f, cy = (float)j + 0.5f;
    int win = -1;
    for (int k = 0; k < NB; ++k) {
        const int ia = s_b[k][0], ib = s_b[k][1];
        if ((unsigned)ia >= (unsigned)J || (unsigned)ib >= (unsigned)J) continue;
        const float ax = s_j[ia][0], ay = s_j[ia][1], bx = s_j[ib][0], by = s_j[ib][1];
        if (!(finite_f(ax) && finite_f(ay) && finite_f(bx) && finite_f(by))) continue;
        const float dx = bx - ax, dy = by - ay, qx = cx - ax, qy = cy - ay;
        const float l2 = dx * dx + dy * dy;
        float t = l2 > 0.f ? (qx * dx + qy * dy) / l2 : 0.f;
        t = fminf(fmaxf(t, 0.f), 1.f);
        const float rx = qx - t * dx, ry = qy - t * dy;
        if (sqrtf(rx * rx + ry * ry) <= rb) win = k;
    }
    for (int k = 0; k < J; ++k) {
        const float ax = s_j[k][0], ay = s_j[k][1];
        if (!(finite_f(ax) && finite_f(ay))) continue;
        const float rx = cx - ax, ry = cy - ay;
        if (sqrtf(rx * rx + ry * ry) <= rj) win = NB + k;
    }
    if (win < 0) return;
    uint8_t* out = rgb + ((size_t)b * H * W + p) * 3;
    out[0] = colors[win * 3 + 0];
    out[1] = colors[win * 3 + 1];
    out[2] = colors[win * 3 + 2];
}

int check_image(const char* fn, int B, int H, int W) {
    SCAT_REQUIRE(B > 0, SCAT_E_SHAPE, "%s: batch %d must be positive", fn, B);
    SCAT_REQUIRE(H >= 1 && H <= kRMaxHW && W >= 1 && W <= kRMaxHW, SCAT_E_SHAPE, "%s: image %d x %d outside 1..%d", fn, H, W,
                 kRMaxHW);
    SCAT_REQUIRE(fits_i32((int64_t)B * H * W * 3), SCAT_E_SHAPE, "%s: %d images of %d x %d are too many", fn, B, H, W);
    return SCAT_OK;
}

int check_mesh(const char* fn, int V, int F) {
    SCAT_REQUIRE(V >= 1 && V <= kRMaxV, SCAT_E_SHAPE, "%s: %d vertices outside 1..%d", fn, V, kRMaxV);
    SCAT_REQUIRE(F >= 1 && F <= kRMaxF, SCAT_E_SHAPE, "%s: %d faces outside 1..%d", fn, F, kRMaxF);
    return SCAT_OK;
}

int check_words(const char* fn, const void* const* ptrs, int n) {
    uintptr_t all = 0;
    for (int i = 0; i < n; ++i) {
        SCAT_REQUIRE(ptrs[i], SCAT_E_ARG, "%s: null pointer", fn);
        all |= (uintptr_t)ptrs[i];
    }
    SCAT_REQUIRE((all & 3) == 0, SCAT_E_ARG, "%s: fp32 and int32 operands must be 4-byte aligned", fn);
    return SCAT_OK;
}

}  // namespace
}  // namespace scat

using namespace scat;

extern "C" int scat_render_project(const float* verts, const float* cam, const int32_t* faces, const int32_t* vf_off,
                                   const int32_t* vf_idx, int32_t* proj, int B, int V, int F, int H, int W, void* stream) {
    const char* fn = "scat_render_project";
    const void* ptrs[] = {verts, cam, faces, vf_off, vf_idx, proj};
    if (int rc = check_words(fn, ptrs, 6)) return rc;
    if (int rc = check_image(fn, B, H, W)) return rc;
    if (int rc = check_mesh(fn, V, F)) return rc;
    hipLaunchKernelGGL(render_project_kernel, dim3(B), dim3(kProjThreads), 0, (hipStream_t)stream, verts, cam, faces, vf_off,
                       vf_idx, proj, V, F, 0.5f * (float)W, 0.5f * (float)H);
    SCAT_LAUNCH_CHECK("scat_render_project");
    set_kernel_label("render_project_v%d", V);
    return SCAT_OK;
}

extern "C" int scat_render_raster(const int32_t* proj, const int32_t* faces, const uint8_t* img, const float* lights,
                                  int32_t* face_id, float* depth, uint8_t* rgb, int B, int V, int F, int H, int W, int L,
                                  float base_r, float base_g, float base_b, float ambient, int cull, void* stream) {
    const char* fn = "scat_render_raster";
    SCAT_REQUIRE(L >= 0 && L <= kRMaxL, SCAT_E_SHAPE, "%s: %d lights outside 0..%d", fn, L, kRMaxL);
    const void* ptrs[] = {proj, faces, face_id, depth, lights};
    if (int rc = check_words(fn, ptrs, L > 0 ? 5 : 4)) return rc;
    SCAT_REQUIRE(cull == 0 || cull == 1, SCAT_E_ARG, "%s: cull %d must be 0 or 1", fn, cull);
    if (int rc = check_image(fn, B, H, W)) return rc;
    if (int rc = check_mesh(fn, V, F)) return rc;
    SCAT_REQUIRE(B <= 65535, SCAT_E_SHAPE, "%s: batch %d above 65535", fn, B);
    RasterArgs a;
    a.proj = proj, a.faces = faces, a.img = img, a.face_id = face_id, a.depth = depth, a.rgb = rgb;
    a.V = V, a.F = F, a.H = H, a.W = W, a.L = L, a.cull = cull;
    a.base[0] = base_r, a.base[1] = base_g, a.base[2] = base_b, a.ambient = ambient;
    hipLaunchKernelGGL(render_raster_kernel, dim3(cdiv(W, kTile), cdiv(H, kTile), B), dim3(kRasterThreads), 0,
                       (hipStream_t)stream, a, lights);
    SCAT_LAUNCH_CHECK("scat_render_raster");
    set_kernel_label("render_raster_f%d%s", F, rgb ? "_rgb" : "");
    return SCAT_OK;
}

extern "C" int scat_render_skeleton(const float* j2d, const int32_t* bones, const uint8_t* colors, uint8_t* rgb, int B, int J,
                                    int NB, int H, int W, float radius_bone, float radius_joint, void* stream) {
    const char* fn = "scat_render_skeleton";
    SCAT_REQUIRE(J >= 1 && J <= kRMaxJ, SCAT_E_SHAPE, "%s: %d joints outside 1..%d", fn, J, kRMaxJ);
    SCAT_REQUIRE(NB >= 0 && NB <= kRMaxB, SCAT_E_SHAPE, "%s: %d bones outside 0..%d", fn, NB, kRMaxB);
    const void* ptrs[] = {j2d, bones};
    if (int rc = check_words(fn, ptrs, NB > 0 ? 2 : 1)) return rc;
    SCAT_REQUIRE(colors && rgb, SCAT_E_ARG, "%s: null pointer", fn);
    if (int rc = check_image(fn, B, H, W)) return rc;
    SCAT_REQUIRE(B <= 65535, SCAT_E_SHAPE, "%s: batch %d above 65535", fn, B);
    hipLaunchKernelGGL(render_skeleton_kernel, dim3(cdiv((int64_t)H * W, kSkelThreads), B), dim3(kSkelThreads), 0,
                       (hipStream_t)stream, j2d, bones, colors, rgb, J, NB, H, W, radius_bone, radius_joint);
    SCAT_LAUNCH_CHECK("scat_render_skeleton");
    set_kernel_label("render_skeleton_j%d_b%d", J, NB);
    return SCAT_OK;
}
