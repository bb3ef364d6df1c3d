/* libscat_hip — C ABI of the on-device mesh and skeleton renderer (fourth public header of the one library; the
 * conventions are those of scat_mano.h: device pointers owned by the caller, explicit sizes, hipStream_t as void* last,
 * stream-ordered, never synchronises, never allocates, retains no pointer, returns 0 or a negative SCAT_E_* code).  No
 * workspace is needed: the projected vertices are an output of their own, sized here.
 *
 * Stands in for the viewing half of the reference's workflow (reference checkout tomguluson92/SCAT):
 *   data_utils/render.py:10-88   the MANO mesh over the frame with pyrender (needs an OpenGL/EGL context)
 *   render.py:43-60              mesh turned 180 degrees about x, weak-perspective camera, scale [sx, sx], translation
 *                                [tx, ty]: the reference does not ship its WeakPerspectiveCamera class, so the image is
 *                                defined by the formula below, which is the projection the loss and the evaluation use
 *                                (train.py:112-120, scat_eval_accumulate), so that projected joints and the mesh line up
 *   render.py:25                 ambient light 0.3
 *   render.py:29-37              three point lights; here three directions in the camera frame
 *   render.py:39                 base colour (1.0, 1.0, 0.9)
 *   render.py:81-83              pixels the mesh does not cover show the frame
 *   train.py:211-222, eval.py:715-742   debug_pred_gt / plot_2d_hand: joints and bones over the frame (matplotlib)
 *
 * This is Lambert shading of interpolated vertex normals.  It claims NO pixel parity with pyrender's physically based
 * shading: the parity target is the fp64 oracle of tests/_render_oracle.py.
 *
 * Frame: x right, y down, the camera looks along +z, a smaller z is nearer.  A pixel (i, j) = (column, row) has its centre
 * at (i + 0.5, j + 0.5).  Images are [B,H,W,...] row-major; 1 <= H, W <= SCAT_RENDER_MAX_HW.
 *
 * ---- exact coverage ----
 * Vertices are snapped to 1/256 pixel (8 sub-pixel bits: a 224-pixel image is 57344 steps, |X| is admitted to 2^22, i.e.
 * 16384 pixels, a difference is below 2^23 and a product of two below 2^46, so every edge function is exact in int64) and
 * coverage is integer arithmetic on the snapped coordinates.  For a face (a, b, c) with snapped (x0,y0), (x1,y1), (x2,y2):
 *   A = (x1-x0)(y2-y0) - (y1-y0)(x2-x0)                       signed area, int64
 *   A == 0   the face is dropped
 *   A <  0   vertices 1 and 2 are swapped; the face is FRONT-facing (its normal (b-a)x(c-a) points toward the camera)
 *   A >  0   the face is back-facing; with cull = 1 it is dropped
 *   edge function of the directed edge (a->b) at P = (256 i + 128, 256 j + 128):  e = (xb-xa)(Py-ya) - (yb-ya)(Px-xa)
 *   the pixel is inside iff, for all three edges, e > 0, or e == 0 and (dy > 0 or (dy == 0 and dx < 0)), with
 *   (dx, dy) = (xb-xa, yb-ya): a pixel centre on an edge shared by two faces belongs to exactly one of them
 *   z = (e0 z_a + e1 z_b + e2 z_c) / A, e_i the edge function opposite vertex i (after the swap), in fp32 with every
 *   operation rounded on its own, left to right; e_i and A are converted from int64 to fp32 first
 *   the visible face has the smallest z; equal z goes to the lowest face index
 * A face with an invalid vertex, or with a vertex index outside 0..V-1, is dropped.
 */
#ifndef SCAT_RENDER_H
#define SCAT_RENDER_H
#include <stdint.h>

#include "scat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define SCAT_RENDER_MAX_V 1536 /* as SCAT_MANO_MAX_V */
#define SCAT_RENDER_MAX_F 4096
#define SCAT_RENDER_MAX_HW 1024
#define SCAT_RENDER_MAX_LIGHTS 4
#define SCAT_RENDER_MAX_J 32
#define SCAT_RENDER_MAX_BONES 32
#define SCAT_RENDER_PROJ_WORDS 8 /* 32-bit words per projected vertex */
#define SCAT_RENDER_SNAP_LIMIT 4194304 /* 2^22: a vertex with |X| or |Y| above it is invalid */

/* verts[B,V,3] fp32, cam[B,3] = (s, tx, ty) -> proj[B,V,8] 32-bit words, B * V * 32 bytes, every word written:
 *   0  X = rint(u * 256) int32, u = (s (x + tx)) (W/2) + W/2      each fp32 operation rounded on its own, no contraction;
 *   1  Y = rint(v * 256) int32, v = (s (y + ty)) (H/2) + H/2      W/2 and H/2 are exact in fp32
 *   2  z fp32, copied
 *   3..5  unit vertex normal fp32: the sum, in ascending face order, of (b-a)x(c-a) over the incident faces whose three
 *         vertices are all valid (area-weighted, metres, fp32), normalised; a zero or non-finite sum gives (0, 0, -1)
 *   6  1 if the vertex is valid, else 0: invalid if x, y, z, u * 256 or v * 256 is not finite or |X| or |Y| exceeds
 *      SCAT_RENDER_SNAP_LIMIT; an invalid vertex has X = Y = 0, z = 0 and the normal (0, 0, -1)
 *   7  0 (spare)
 * The topology is data, prepared once by the caller: faces[F,3] int32 and the vertex -> face table vf_off[V+1],
 * vf_idx[3F] int32 (vf_idx[vf_off[v] .. vf_off[v+1]) are the faces that name v, ascending).  An index outside its range
 * is skipped, never followed.  1 <= V <= SCAT_RENDER_MAX_V, 1 <= F <= SCAT_RENDER_MAX_F.  One workgroup per sample.
 * Operands at any 4-byte-aligned address. */
int scat_render_project(const float* verts, const float* cam, const int32_t* faces, const int32_t* vf_off,
                        const int32_t* vf_idx, int32_t* proj, int B, int V, int F, int H, int W, void* stream);

/* proj[B,V,8] + faces[F,3] -> face_id[B,H,W] int32 (-1 where no face covers the pixel), depth[B,H,W] fp32 (+inf there)
 * and, unless rgb is null, rgb[B,H,W,3] bytes at any address:
 *   n      = the barycentric blend (e_i / A) of the three vertex normals, normalised ((0,0,-1) if its length is zero or
 *            not finite), negated for a back-facing face
 *   shade  = min(1, ambient + sum_l I_l max(0, n . d_l)),  lights[L,4] = (unit direction toward the light, I_l),
 *            0 <= L <= SCAT_RENDER_MAX_LIGHTS (lights may be null when L = 0)
 *   pixel  = round-half-even(255 clamp(base * shade, 0, 1)) per channel, base = (base_r, base_g, base_b)
 *   a pixel no face covers copies img[B,H,W,3] (bytes, any address), or is 0 when img is null
 * cull: 0 or 1.  One workgroup per (sample, 16 x 16 tile); no atomics and no floating-point sum across threads, so the
 * same call gives the same bits. */
int scat_render_raster(const int32_t* proj, const int32_t* faces, const uint8_t* img, const float* lights,
                       int32_t* face_id, float* depth, uint8_t* rgb, int B, int V, int F, int H, int W, int L,
                       float base_r, float base_g, float base_b, float ambient, int cull, void* stream);

/* j2d[B,J,2] fp32 pixel coordinates, bones[NB,2] int32 (joint indices), colors[NB+J,3] bytes (bones first), rgb[B,H,W,3]
 * bytes in/out at any address.  A pixel centre (i + 0.5, j + 0.5) is painted by bone k if its distance to the segment is
 * <= radius_bone and by joint k if its distance to the point is <= radius_joint; bones ascending, then joints ascending,
 * the last one wins; other pixels are left as they are.  All fp32, one thread per pixel.  A bone with a non-finite end
 * (or an index outside 0..J-1) and a joint with a non-finite coordinate paint nothing.
 * 1 <= J <= SCAT_RENDER_MAX_J, 0 <= NB <= SCAT_RENDER_MAX_BONES (bones may be null when NB = 0). */
int scat_render_skeleton(const float* j2d, const int32_t* bones, const uint8_t* colors, uint8_t* rgb, int B, int J, int NB,
                         int H, int W, float radius_bone, float radius_joint, void* stream);

#ifdef __cplusplus
}
#endif
#endif
