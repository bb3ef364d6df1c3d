"""The renderer of include/scat_render.h restated in plain numpy: the fp32 projection and snap operation for operation
(so the integers are the device's, bit for bit), coverage in int64 arithmetic on the snapped coordinates, depth, normals
and shading in fp64.  Besides the images it returns an AMBIGUITY MASK, the pixels where a correct fp32 implementation may
differ from fp64: the second-nearest covering face within 1e-4 (z_max - z_min) of the nearest, a blended normal shorter
than 1e-3, and for the skeleton a distance within 1e-3 px of a radius.
Plain helper module: no fixtures, no pytest hooks."""
from __future__ import annotations

import numpy as np

SNAP_LIMIT = 1 << 22
DEPTH_BAND = 1e-4       # of the sample's z range
SHORT_NORMAL = 1e-3
SKELETON_BAND = 1e-3    # pixels

AMBIENT = 0.3
BASE_RGB = (1.0, 1.0, 0.9)
LIGHTS = np.array([d / np.linalg.norm(d) for d in np.array([[0, 1, -1], [0, -1, -1], [1, -1, -2]], dtype=np.float64)])
LIGHTS = np.concatenate([LIGHTS, np.full((3, 1), 0.4)], axis=1)      # [3,4]: unit direction toward the light, intensity

MANO_PARENTS = (0, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)
MANO_BONES = tuple((MANO_PARENTS[i], i) for i in range(1, 16)) + tuple((3 * k, 15 + k) for k in range(1, 6))


def rotation(axis, angle):
    """Rodrigues in fp64"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def project(verts, cam, H, W):
    """verts [V,3] fp32, cam (s, tx, ty) -> X, Y int64 [V], valid bool [V]; every fp32 operation rounded on its own"""
    f = np.float32
    verts, cam = np.asarray(verts, dtype=f), np.asarray(cam, dtype=f)
    s, tx, ty = cam[0], cam[1], cam[2]
    hw, hh = f(0.5) * f(W), f(0.5) * f(H)
    with np.errstate(all="ignore"):
        u = (s * (verts[:, 0] + tx)) * hw + hw
        v = (s * (verts[:, 1] + ty)) * hh + hh
        uf, vf = u * f(256.0), v * f(256.0)
        assert uf.dtype == f and vf.dtype == f
        ok = np.isfinite(verts).all(axis=1) & np.isfinite(uf) & np.isfinite(vf)
        ru, rv = np.rint(np.where(ok, uf, 0)), np.rint(np.where(ok, vf, 0))
    ok &= (np.abs(ru) <= SNAP_LIMIT) & (np.abs(rv) <= SNAP_LIMIT)
    X, Y = np.where(ok, ru, 0).astype(np.int64), np.where(ok, rv, 0).astype(np.int64)
    return X, Y, ok


def vertex_normals(verts, faces, valid):
    """fp64: area-weighted sum of (b-a)x(c-a) over the incident faces whose three vertices are valid, normalised; a zero
    sum, or an invalid vertex, gives (0, 0, -1)"""
    v = np.where(valid[:, None], np.asarray(verts, dtype=np.float64), 0.0)
    fa = faces[valid[faces].all(axis=1)]
    cr = np.cross(v[fa[:, 1]] - v[fa[:, 0]], v[fa[:, 2]] - v[fa[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, fa[:, k], cr)
    ln = np.linalg.norm(n, axis=1)
    good = valid & (ln > 0)
    out = np.tile(np.array([0.0, 0.0, -1.0]), (len(v), 1))
    out[good] = n[good] / ln[good, None]
    return out


def orient(X, Y, face):
    """-> (a, b, c, A, back) with A > 0 after the swap, or None for a zero-area face"""
    a, b, c = (int(i) for i in face)
    A = (int(X[b]) - int(X[a])) * (int(Y[c]) - int(Y[a])) - (int(Y[b]) - int(Y[a])) * (int(X[c]) - int(X[a]))
    if A == 0:
        return None
    return (a, c, b, -A, False) if A < 0 else (a, b, c, A, True)


def _edge(X, Y, p, q, PX, PY):
    """the edge function of p -> q at the pixel centres and its inside test with the tie rule"""
    dx, dy = int(X[q]) - int(X[p]), int(Y[q]) - int(Y[p])
    e = dx * (PY - int(Y[p])) - dy * (PX - int(X[p]))
    tie = dy > 0 or (dy == 0 and dx < 0)
    return e, (e > 0) | ((e == 0) & tie)


def face_cover(X, Y, tri, H, W):
    """tri = (a, b, c) oriented with A > 0 -> (i0, j0, inside [h,w] bool, e0, e1, e2 int64 [h,w]) over the face's box of
    pixel centres clipped to the image, or None if the box is empty"""
    a, b, c = tri
    xs, ys = [int(X[k]) for k in tri], [int(Y[k]) for k in tri]
    i0, i1 = max(0, -((128 - min(xs)) // 256)), min(W - 1, (max(xs) - 128) // 256)
    j0, j1 = max(0, -((128 - min(ys)) // 256)), min(H - 1, (max(ys) - 128) // 256)
    if i1 < i0 or j1 < j0:
        return None
    PX = (256 * np.arange(i0, i1 + 1, dtype=np.int64) + 128)[None, :]
    PY = (256 * np.arange(j0, j1 + 1, dtype=np.int64) + 128)[:, None]
    e0, in0 = _edge(X, Y, b, c, PX, PY)
    e1, in1 = _edge(X, Y, c, a, PX, PY)
    e2, in2 = _edge(X, Y, a, b, PX, PY)
    return i0, j0, in0 & in1 & in2, e0, e1, e2


def raster(verts, cam, faces, H, W, img=None, cull=False, base_rgb=BASE_RGB, ambient=AMBIENT, lights=LIGHTS):
    """One sample.  -> dict: X, Y, valid; normals [V,3]; face_id [H,W] int32; depth [H,W] fp64 (+inf background);
    depth32 [H,W]: the same formula in numpy fp32 for the visible face; rgb [H,W,3] uint8; count [H,W]: how many faces
    cover the pixel; ambiguous [H,W] bool."""
    verts = np.asarray(verts, dtype=np.float32)
    faces = np.asarray(faces, dtype=np.int64)
    X, Y, valid = project(verts, cam, H, W)
    z32 = verts[:, 2]
    z = z32.astype(np.float64)
    normals = vertex_normals(verts, faces, valid)
    face_id = np.full((H, W), -1, dtype=np.int32)
    depth, second = np.full((H, W), np.inf), np.full((H, W), np.inf)
    depth32 = np.full((H, W), np.inf, dtype=np.float32)
    count = np.zeros((H, W), dtype=np.int32)
    nrm = np.zeros((H, W, 3))
    back = np.zeros((H, W), dtype=bool)
    f32 = np.float32
    for f, face in enumerate(faces):
        if not valid[face].all():
            continue
        o = orient(X, Y, face)
        if o is None or (cull and o[4]):
            continue
        a, b, c, A, bk = o
        cov = face_cover(X, Y, (a, b, c), H, W)
        if cov is None:
            continue
        i0, j0, inside, e0, e1, e2 = cov
        if not inside.any():
            continue
        h, w = inside.shape
        sl = (slice(j0, j0 + h), slice(i0, i0 + w))
        zf = (e0 * z[a] + e1 * z[b] + e2 * z[c]) / A
        with np.errstate(all="ignore"):
            zf32 = ((e0.astype(f32) * z32[a] + e1.astype(f32) * z32[b]) + e2.astype(f32) * z32[c]) / f32(A)
        assert zf32.dtype == f32
        count[sl] += inside
        d, s2, fid = depth[sl], second[sl], face_id[sl]
        win = inside & ((fid < 0) | (zf < d))      # ascending faces: an equal z keeps the lower index
        lose = inside & ~win
        second[sl] = np.where(win, d, np.where(lose, np.minimum(s2, zf), s2))
        depth[sl] = np.where(win, zf, d)
        depth32[sl] = np.where(win, zf32, depth32[sl])
        face_id[sl] = np.where(win, f, fid)
        back[sl] = np.where(win, bk, back[sl])
        bl = (e0[..., None] * normals[a] + e1[..., None] * normals[b] + e2[..., None] * normals[c]) / A
        nrm[sl] = np.where(win[..., None], bl, nrm[sl])
    covered = face_id >= 0
    zr = float(z[valid].max() - z[valid].min()) if valid.any() else 0.0
    ln = np.linalg.norm(nrm, axis=2)
    with np.errstate(invalid="ignore"):      # inf - inf on the background
        ambiguous = covered & ((second - depth <= DEPTH_BAND * zr) | (ln < SHORT_NORMAL))
    n = np.where((ln > 0)[..., None], nrm / np.where(ln > 0, ln, 1.0)[..., None], np.array([0.0, 0.0, -1.0]))
    n = np.where(back[..., None], -n, n)
    lights = np.asarray(lights, dtype=np.float64).reshape(-1, 4)
    shade = np.full((H, W), float(ambient))
    for d in lights:
        shade += d[3] * np.maximum(n @ d[:3], 0.0)
    shade = np.minimum(shade, 1.0)
    col = np.rint(255.0 * np.clip(shade[..., None] * np.asarray(base_rgb, dtype=np.float64), 0.0, 1.0)).astype(np.uint8)
    bg = np.zeros((H, W, 3), dtype=np.uint8) if img is None else np.asarray(img, dtype=np.uint8)
    rgb = np.where(covered[..., None], col, bg)
    return dict(X=X, Y=Y, valid=valid, normals=normals, face_id=face_id, depth=depth, depth32=depth32, rgb=rgb, count=count,
                ambiguous=ambiguous)


def render(verts, cam, faces, H, W, img=None, **kw):
    """A batch: verts [B,V,3], cam [B,3], img [B,H,W,3] or None -> the dict of raster() with a leading batch axis"""
    outs = [raster(verts[b], cam[b], faces, H, W, None if img is None else img[b], **kw) for b in range(len(verts))]
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}


def depth_formula_error(out, verts):
    """max |fp32 formula - fp64| / max |z| of the sample over the covered pixels of a raster() result"""
    c = out["face_id"] >= 0
    if not c.any():
        return 0.0
    return float(np.abs(out["depth32"][c].astype(np.float64) - out["depth"][c]).max() / np.abs(np.asarray(verts)[:, 2]).max())


def skeleton(rgb, j2d, bones, colors, radius_bone, radius_joint):
    """One image [H,W,3] uint8, j2d [J,2], bones [NB,2], colors [NB+J,3] -> (rgb, painted [H,W] bool, ambiguous [H,W]
    bool), fp64: bones ascending, then joints ascending, the last one wins"""
    rgb = np.array(rgb, dtype=np.uint8)
    H, W = rgb.shape[:2]
    j = np.asarray(j2d, dtype=np.float64).reshape(-1, 2)
    bones = np.asarray(bones, dtype=np.int64).reshape(-1, 2)
    cx, cy = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    win = np.full((H, W), -1)
    amb = np.zeros((H, W), dtype=bool)

    def paint(dist, r, k):
        nonlocal win, amb
        win = np.where(dist <= r, k, win)
        amb |= np.abs(dist - r) < SKELETON_BAND

    for k, (ia, ib) in enumerate(bones):
        a, b = j[ia], j[ib]
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            continue
        d = b - a
        l2 = d @ d
        t = np.clip(((cx - a[0]) * d[0] + (cy - a[1]) * d[1]) / l2, 0.0, 1.0) if l2 > 0 else np.zeros_like(cx)
        paint(np.hypot(cx - a[0] - t * d[0], cy - a[1] - t * d[1]), radius_bone, k)
    for k, a in enumerate(j):
        if np.isfinite(a).all():
            paint(np.hypot(cx - a[0], cy - a[1]), radius_joint, len(bones) + k)
    painted = win >= 0
    rgb[painted] = np.asarray(colors, dtype=np.uint8)[win[painted]]
    return rgb, painted, amb


# ------------------------------------------------------------------------------------------------ shared test scenes
VIEWS = (("front", None, 0.0, (8.0, 0.0, 0.0)), ("tilt", (1, 1, 0), 0.9, (7.0, 0.02, -0.01)),
         ("side", (0, 1, 0), 1.5, (9.0, 0.0, 0.0)), ("back", (1, 0, 0), 3.0, (5.0, 0.05, 0.05)),
         ("clip", (0, 0, 1), 0.5, (14.0, 0.06, 0.0)), ("small", None, 0.0, (1.0, 0.3, 0.2)))


def views(v):
    """the six views of the hand mesh: verts [6,V,3] fp32 (v . R^T, the rotation in fp64, cast once), cam [6,3] fp32"""
    vs, cams = [], []
    for _, axis, angle, cam in VIEWS:
        R = np.eye(3) if axis is None else rotation(axis, angle)
        vs.append((np.asarray(v, dtype=np.float64) @ R.T).astype(np.float32))
        cams.append(cam)
    return np.stack(vs), np.asarray(cams, dtype=np.float32)


def fan_square(seed=0, n=8, side=10, origin=3):
    """a fan of n randomly wound triangles tiling a side x side-pixel square whose vertices sit on pixel centres: ->
    verts [n+1,3] fp32, faces [n,3], cam, (H, W); the fan must cover side x side pixels, each exactly once.  cam =
    (1, 0, 0) at H = W = 2 * (origin + side + 3): u = x * hw + hw, so a vertex for pixel centre c sits at (c - hw) / hw,
    chosen among the values that project back to c exactly."""
    rng = np.random.RandomState(seed)
    H = W = 2 * (origin + side + 3)
    hw = W / 2
    lo, hi = origin, origin + side      # the square [lo + 0.5, hi + 0.5]^2 in pixels, corners on pixel centres
    ring = [(lo + k, lo) for k in range(0, side, 5)] + [(hi, lo + k) for k in range(0, side, 5)] + \
           [(hi - k, hi) for k in range(0, side, 5)] + [(lo, hi - k) for k in range(0, side, 5)]
    assert len(ring) == n
    hub = (lo + 4, lo + 7)
    px = np.array(ring + [hub], dtype=np.float64) + 0.5
    verts = np.concatenate([(px - hw) / hw, rng.uniform(0.5, 1.5, (n + 1, 1))], axis=1).astype(np.float32)
    faces = []
    for k in range(n):
        tri = [k, (k + 1) % n, n]
        if rng.rand() < 0.5:
            tri = [tri[0], tri[2], tri[1]]
        r = rng.randint(3)
        faces.append(tri[r:] + tri[:r])
    cam = np.array([1.0, 0.0, 0.0], dtype=np.float32)
    X, Y, ok = project(verts, cam, H, W)
    assert ok.all() and np.array_equal(X, (px[:, 0] * 256).astype(np.int64)) and np.array_equal(Y, (px[:, 1] * 256).astype(np.int64))
    return verts, np.asarray(faces, dtype=np.int32), cam, (H, W)


def pixel_verts(px, z, H, W):
    """vertices that the camera (1, 0, 0) projects to the pixel coordinates px [n,2] (exactly, when W/2 and H/2 are powers
    of two and px are multiples of 1/256): [n,3] fp32"""
    px = np.asarray(px, dtype=np.float64)
    return np.stack([(px[:, 0] - W / 2) / (W / 2), (px[:, 1] - H / 2) / (H / 2), np.asarray(z, dtype=np.float64)], axis=1).astype(np.float32)


UNIT_CAM = np.array([1.0, 0.0, 0.0], dtype=np.float32)


def small_meshes():
    """{name: (verts [V,3], faces [F,3], (H, W))}, all seen by the camera (1, 0, 0): the edge cases of the coverage rules"""
    c = 0.5      # pixel centres
    m = {}
    v, f, _, hw = fan_square(0)
    m["fan square"] = (v, f, hw)
    quad = [(4 + c, 4 + c), (12 + c, 4 + c), (12 + c, 12 + c), (4 + c, 12 + c)]
    m["shared edge through centres"] = (pixel_verts(quad, [1, 2, 3, 2], 32, 32), [[0, 1, 2], [0, 2, 3]], (32, 32))
    m["shared edge, mixed winding"] = (pixel_verts(quad, [1, 2, 3, 2], 32, 32), [[2, 1, 0], [0, 2, 3]], (32, 32))
    m["vertex on a pixel centre"] = (pixel_verts([(5 + c, 5 + c), (20 + c, 7 + c), (9 + c, 18 + c)], [1, 1.5, 2], 32, 32),
                                     [[0, 1, 2]], (32, 32))
    m["off-screen face"] = (pixel_verts([(-50, 3), (-20, 5), (-30, 25), (3.2, 4.1), (25.7, 9.3), (11.4, 27.9)], [1] * 6, 32, 32),
                            [[0, 1, 2], [3, 4, 5]], (32, 32))
    strip = pixel_verts([(2.3, 3.1), (12.2, 2.4), (3.7, 14.9), (14.1, 15.6), (25.3, 4.2), (27.8, 17.3)], [1, 2, 1, 2, 1, 2], 32, 32)
    strip[4] = np.nan
    m["NaN vertex"] = (strip, [[0, 1, 2], [1, 3, 2], [1, 4, 3], [4, 5, 3]], (32, 32))
    two = pixel_verts([(3.3, 3.3), (28.1, 5.2), (8.4, 27.7), (6.3, 2.3), (29.1, 9.2), (4.4, 25.7)], [1, 1, 1, 2, 2, 2], 32, 32)
    m["near face first"] = (two, [[0, 1, 2], [3, 4, 5]], (32, 32))
    m["near face second"] = (two, [[3, 4, 5], [0, 1, 2]], (32, 32))
    one = pixel_verts([(3.3, 3.3), (28.1, 5.2), (8.4, 27.7)], [1, 2, 3], 32, 32)
    m["coincident faces"] = (one, [[0, 1, 2], [0, 1, 2], [0, 1, 2]], (32, 32))      # the same arithmetic: exactly equal z
    m["coincident faces, opposite winding"] = (one, [[0, 2, 1], [0, 1, 2]], (32, 32))
    m["one face"] = (one, [[0, 1, 2]], (32, 32))
    m["zero-area face"] = (pixel_verts([(3 + c, 3 + c), (13 + c, 13 + c), (23 + c, 23 + c), (3.3, 20.2)], [1, 2, 3, 1], 32, 32),
                           [[0, 1, 2], [0, 1, 1], [0, 3, 2]], (32, 32))
    m["tiles over the border"] = (pixel_verts([(-4.2, -3.1), (40.3, 2.2), (15.6, 30.4), (1.1, 16.9)], [1, 2, 3, 4], 17, 33),
                                  [[0, 1, 2], [0, 2, 3]], (17, 33))
    return {k: (np.asarray(v, dtype=np.float32), np.asarray(f, dtype=np.int32), hw) for k, (v, f, hw) in m.items()}


def joints_of(verts):
    """21 stand-in joints for a view of the hand mesh: every 37th vertex"""
    return np.asarray(verts)[::37][:21]


def project_joints(j3, cam, H, W):
    """fp64: [J,3], (s, tx, ty) -> [J,2] pixels"""
    j3, cam = np.asarray(j3, dtype=np.float64), np.asarray(cam, dtype=np.float64)
    return (cam[0] * (j3[:, :2] + cam[1:])) * np.array([W / 2, H / 2]) + np.array([W / 2, H / 2])
