"""The mesh and skeleton renderer, the parts that need no GPU: the fourth public header and its binding, argument errors
of the three entry points, the numpy oracle of tests/_render_oracle.py checked against the coverage rules themselves, host
validation of MeshRenderer / SkeletonOverlay, and the conditions the GPU tests rest on (the share of ambiguous pixels of
every view, the depth gate)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_oracle as RO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RENDER_H = os.path.join(ROOT, "include", "scat_render.h")
H = W = 224
AMBIGUOUS_CAP = 0.005       # of the covered pixels of a view: a condition on the views, not a measurement
SKELETON_CAP = 0.01         # of the painted pixels
# max over the covered pixels of |the header's depth formula in numpy fp32 - the same in fp64| / max |z| of the sample, the
# largest of the six views (view "clip"); the GPU gate is 4 x this (tests/test_gpu_render.py)
E_DEPTH = 1.702e-07


@pytest.fixture(scope="module")
def built():
    from scat_amd import build

    return build.build(verbose=False)


@functools.lru_cache(maxsize=None)
def mesh():
    g = np.load(os.path.join(ROOT, "tests", "golden", "hand_mesh.npz"))
    return g["v"], g["f"]


@functools.lru_cache(maxsize=None)
def view_refs():
    v, f = mesh()
    vs, cams = RO.views(v)
    return vs, cams, [RO.raster(vs[b], cams[b], f, H, W) for b in range(len(vs))]


def test_render_header_is_bound(built):
    from scat_amd._lib import HEADERS, RENDER_HEADER, lib, parse_header

    assert os.path.samefile(HEADERS[-2], RENDER_H) and os.path.samefile(RENDER_HEADER, RENDER_H)
    protos = parse_header(RENDER_H)
    assert list(protos) == ["scat_render_project", "scat_render_raster", "scat_render_skeleton"]
    L = lib()
    for name, (rt, args) in protos.items():
        assert hasattr(L.cdll, name), name
        assert callable(getattr(L, name)), name
        assert rt is ctypes.c_int and args[-1][1] == "stream", name
        names = [an for _, an in args]
        assert "ws" not in names and "ws_bytes" not in names and not name.endswith("_ws")
    assert L.by_header[RENDER_HEADER] == protos and list(L.by_header) == list(HEADERS) and not set(protos) & set(L.protos)
    assert not set(protos) & set(parse_header())
    # the base colour travels by value
    by_name = {an: ty for ty, an in protos["scat_render_raster"][1]}
    assert [by_name[k] for k in ("base_r", "base_g", "base_b", "ambient")] == [ctypes.c_float] * 4
    src = open(RENDER_H).read()
    assert src.count("render.py:") >= 5 and "NO pixel parity" in src
    from scat_amd import render

    for macro, value in (("MAX_V", render.MAX_V), ("MAX_F", render.MAX_F), ("MAX_HW", render.MAX_HW),
                         ("MAX_LIGHTS", render.MAX_LIGHTS), ("MAX_J", render.MAX_J), ("MAX_BONES", render.MAX_BONES),
                         ("SNAP_LIMIT", RO.SNAP_LIMIT)):
        assert f"#define SCAT_RENDER_{macro} {value}" in src, macro


def test_render_errors_surface_without_a_gpu(built):
    """argument validation happens before any HIP call: made-up pointers are never followed, each refusal carries its
    SCAT_E_* code and names the entry point, and the kernel label does not move"""
    from scat_amd._lib import ScatError, lib

    L = lib()
    label = L.scat_last_kernel()
    P = [8 * (i + 1) for i in range(8)]

    def project(ptrs=P[:6], B=2, V=778, F=1538, H=224, W=224):
        return L.scat_render_project(*ptrs, B, V, F, H, W, 0)

    def raster(ptrs=P[:7], B=2, V=778, F=1538, H=224, W=224, nl=3, cull=0):
        return L.scat_render_raster(*ptrs, B, V, F, H, W, nl, 1.0, 1.0, 0.9, 0.3, cull, 0)

    def skeleton(ptrs=P[:4], B=2, J=21, NB=20, H=224, W=224):
        return L.scat_render_skeleton(*ptrs, B, J, NB, H, W, 1.5, 2.5, 0)

    def refused(fn, code, pattern, **kw):
        name = "scat_render_" + fn.__name__
        with pytest.raises(ScatError, match=rf"{name} failed \({code}\): {name}: .*{pattern}"):
            fn(**kw)
        assert L.scat_last_kernel() == label

    for i in range(6):
        refused(project, -2, "null pointer", ptrs=[0 if k == i else p for k, p in enumerate(P[:6])])
    refused(project, -2, "4-byte aligned", ptrs=[10] + P[1:6])
    for fn in (project, raster, skeleton):
        refused(fn, -1, "batch 0 must be positive", B=0)
        refused(fn, -1, r"image 0 x 224 outside 1\.\.1024", H=0)
        refused(fn, -1, r"image 224 x 1025 outside 1\.\.1024", W=1025)
    for fn in (project, raster):
        refused(fn, -1, "0 vertices outside", V=0)
        refused(fn, -1, r"1537 vertices outside 1\.\.1536", V=1537)
        refused(fn, -1, "0 faces outside", F=0)
        refused(fn, -1, r"4097 faces outside 1\.\.4096", F=4097)
    for i in (0, 1, 3, 4, 5):      # img (2) and rgb (6) are optional
        refused(raster, -2, "null pointer", ptrs=[0 if k == i else p for k, p in enumerate(P[:7])])
    refused(raster, -1, r"5 lights outside 0\.\.4", nl=5)
    refused(raster, -1, "-1 lights outside", nl=-1)
    refused(raster, -2, "cull 2 must be 0 or 1", cull=2)
    refused(raster, -2, "4-byte aligned", ptrs=P[:4] + [42] + P[5:7])
    for i in range(4):
        refused(skeleton, -2, "null pointer", ptrs=[0 if k == i else p for k, p in enumerate(P[:4])])
    refused(skeleton, -1, r"0 joints outside 1\.\.32", J=0)
    refused(skeleton, -1, r"33 joints outside 1\.\.32", J=33)
    refused(skeleton, -1, r"33 bones outside 0\.\.32", NB=33)
    refused(skeleton, -1, "-1 bones outside", NB=-1)


# ------------------------------------------------------------------------------------------------ the oracle itself
@pytest.mark.parametrize("seed", range(6))
def test_oracle_fan_covers_every_pixel_once(seed):
    """8 randomly wound and rotated triangles around a hub tile a 10 x 10-pixel square whose corners sit on pixel centres:
    every interior edge passes through pixel centres, and each of the 100 pixels belongs to exactly one face"""
    v, f, cam, (h, w) = RO.fan_square(seed)
    o = RO.raster(v, cam, f, h, w)
    # which 10 of the 11 centres per axis the tie rule keeps is fixed by the rule, not by the windings
    v0, f0, _, _ = RO.fan_square(0)
    first = RO.raster(v0, cam, f0, h, w)["count"]
    assert o["count"].sum() == 100 and o["count"].max() == 1 and np.array_equal(o["count"], first)
    assert np.array_equal(o["count"] > 0, o["face_id"] >= 0)
    rows, cols = np.nonzero(o["count"])
    assert rows.max() - rows.min() == 9 and cols.max() - cols.min() == 9 and (o["count"] > 0).sum() == 100
    assert len(np.unique(o["face_id"])) == 9      # every face of the fan and the background


def test_oracle_winding_does_not_change_coverage():
    v, f, hw = RO.small_meshes()["vertex on a pixel centre"]
    a = RO.raster(v, RO.UNIT_CAM, f, *hw)
    b = RO.raster(v, RO.UNIT_CAM, f[:, [0, 2, 1]], *hw)
    assert (a["face_id"] >= 0).sum() > 50 and np.array_equal(a["face_id"], b["face_id"])
    assert np.allclose(a["depth"], b["depth"], rtol=1e-12)


def test_oracle_zero_area_faces_cover_nothing():
    v, f, hw = RO.small_meshes()["zero-area face"]
    o = RO.raster(v, RO.UNIT_CAM, f, *hw)
    assert set(np.unique(o["face_id"])) == {-1, 2}
    o = RO.raster(v, RO.UNIT_CAM, f[:2], *hw)
    assert (o["face_id"] == -1).all() and o["count"].sum() == 0 and np.isinf(o["depth"]).all()


def test_oracle_quad_diagonals_give_the_same_mask():
    v, _, hw = RO.small_meshes()["shared edge through centres"]
    a = RO.raster(v, RO.UNIT_CAM, np.array([[0, 1, 2], [0, 2, 3]]), *hw)
    b = RO.raster(v, RO.UNIT_CAM, np.array([[0, 1, 3], [1, 2, 3]]), *hw)
    assert a["count"].max() == 1 and b["count"].max() == 1 and a["count"].sum() == 64
    assert np.array_equal(a["count"], b["count"])


def test_oracle_cull_drops_exactly_the_back_faces():
    v, f = mesh()
    vs, cams = RO.views(v)
    X, Y, ok = RO.project(vs[1], cams[1], H, W)
    assert ok.all()
    area = np.array([0 if (o := RO.orient(X, Y, face)) is None else (o[3] if o[4] else -o[3]) for face in f])
    assert (area > 0).sum() > 300 and (area < 0).sum() > 300
    culled = RO.raster(vs[1], cams[1], f, H, W, cull=True)
    front_only = RO.raster(vs[1], cams[1], f[area < 0], H, W)
    ids = np.nonzero(area < 0)[0]
    assert np.array_equal(culled["face_id"] >= 0, front_only["face_id"] >= 0)
    assert np.array_equal(culled["face_id"][culled["face_id"] >= 0], ids[front_only["face_id"][front_only["face_id"] >= 0]])
    assert not np.isin(culled["face_id"], np.nonzero(area >= 0)[0]).any()


def test_oracle_projection_is_fp32_and_flags_invalid_vertices():
    v = np.array([[0.01, 0.02, 0.5], [np.nan, 0, 1], [0, np.inf, 1], [0, 0, -np.inf], [200.0, 0, 1], [0, -200.0, 1],
                  [1e38, 0, 1]], dtype=np.float32)
    X, Y, ok = RO.project(v, np.array([8.0, 0.1, -0.1], dtype=np.float32), H, W)
    assert ok.tolist() == [True, False, False, False, False, False, False]
    assert X[0] == round(((8 * (0.01 + 0.1)) * 112 + 112) * 256) and (X[1:] == 0).all() and (Y[1:] == 0).all()
    # the limit itself is valid: u * 256 = 2^22 exactly
    edge = np.array([[(2.0 ** 14 - 112) / 112, 0, 1], [(2.0 ** 14 - 112 + 0.5) / 112, 0, 1]], dtype=np.float32)
    X, _, ok = RO.project(edge, RO.UNIT_CAM, H, W)
    assert ok.tolist() == [True, False] and X[0] == RO.SNAP_LIMIT


# ------------------------------------------------------------------------------------------------ conditions of the GPU tests
def test_views_are_unambiguous_enough():
    """the oracle alone: the ambiguity mask of every view covers at most 0.5 % of the covered pixels"""
    _, _, refs = view_refs()
    covered = {}
    for (name, *_), o in zip(RO.VIEWS, refs):
        c, a = int((o["face_id"] >= 0).sum()), int(o["ambiguous"].sum())
        covered[name] = c
        print(f"{name}: {c} covered pixels, {a} ambiguous ({100.0 * a / c:.3f} %)")
        assert o["valid"].all() and c > 100 and a <= AMBIGUOUS_CAP * c, name
    assert covered == {"front": 6997, "tilt": 6571, "side": 7020, "back": 2716, "clip": 7629, "small": 107}


def test_depth_gate_constant_is_the_formulas_own_fp32_error():
    vs, _, refs = view_refs()
    errs = [RO.depth_formula_error(o, vs[b]) for b, o in enumerate(refs)]
    print("depth formula, numpy fp32 against fp64, per view: " + " ".join(f"{e:.3e}" for e in errs))
    assert abs(max(errs) / E_DEPTH - 1.0) < 5e-3


def test_skeleton_scenes_are_unambiguous_enough():
    vs, cams, _ = view_refs()
    for b in (0, 1):
        j2d = RO.project_joints(RO.joints_of(vs[b]), cams[b], H, W)
        colors = np.arange(41 * 3, dtype=np.uint8).reshape(41, 3)
        _, painted, amb = RO.skeleton(np.zeros((H, W, 3), np.uint8), j2d, RO.MANO_BONES, colors, 1.5, 2.5)
        print(f"view {b}: {painted.sum()} painted, {amb.sum()} within the band")
        assert painted.sum() > 500 and amb.sum() <= SKELETON_CAP * painted.sum()


def test_oracle_skeleton_order_and_nan():
    colors = np.array([[10, 0, 0], [20, 0, 0], [30, 0, 0], [40, 0, 0], [50, 0, 0]], dtype=np.uint8)      # 2 bones, 3 joints
    j2d = np.array([[4.5, 4.5], [20.5, 4.5], [20.5, 20.5]])
    out, painted, _ = RO.skeleton(np.zeros((32, 32, 3), np.uint8), j2d, [(0, 1), (1, 2)], colors, 1.0, 2.0)
    assert out[4, 12, 0] == 10 and out[12, 20, 0] == 20 and out[4, 4, 0] == 30 and out[4, 20, 0] == 40 and out[20, 20, 0] == 50
    assert out[4, 18, 0] == 40 and out[7, 20, 0] == 20      # the joint over both bones; the later bone beyond the joint's disc
    j2d[1] = np.nan
    out, painted, _ = RO.skeleton(np.zeros((32, 32, 3), np.uint8), j2d, [(0, 1), (1, 2)], colors, 1.0, 2.0)
    assert set(np.unique(out[..., 0])) == {0, 30, 50}


# ------------------------------------------------------------------------------------------------ host validation
def test_mesh_renderer_validates_on_the_host():
    from scat_amd._lib import ScatError
    from scat_amd.render import MAX_F, MAX_V, MeshRenderer

    v, f = mesh()
    r = MeshRenderer(f, 778)
    assert (r.V, r.F, r.H, r.W) == (778, 1538, 224, 224) and r.device is None and r.faces.dtype == np.int32
    assert MeshRenderer(f.tolist(), 778).F == 1538 and MeshRenderer(torch.from_numpy(f).long(), 778).F == 1538
    assert MeshRenderer.from_arrays({"f": f.astype(np.uint32), "v_template": v}).V == 778
    bad = f.copy()
    bad[7, 1] = 778
    for kw, pattern in ((dict(faces=bad), "outside 0..777"), (dict(faces=-f - 1), "outside 0..777"),
                        (dict(n_vertices=777), "outside 0..776"), (dict(n_vertices=0), "0 vertices outside"),
                        (dict(n_vertices=MAX_V + 1), f"{MAX_V + 1} vertices outside"),
                        (dict(faces=np.zeros((MAX_F + 1, 3), np.int32)), f"{MAX_F + 1} faces outside"),
                        (dict(faces=np.zeros((0, 3), np.int32)), "0 faces outside"),
                        (dict(faces=f.astype(np.float32)), "integer indices"), (dict(faces=f[:, :2]), "shape"),
                        (dict(size=(0, 224)), "size 0 x 224"), (dict(size=(224, 1025)), "size 224 x 1025"),
                        (dict(lights=np.zeros((5, 4))), "5 lights")):
        with pytest.raises(ValueError, match=pattern):
            MeshRenderer(**dict(dict(faces=f, n_vertices=778), **kw))
    with pytest.raises(ScatError, match="no CPU fallback"):
        MeshRenderer(f, 778, device="cpu")
    verts, cam = torch.zeros(1, 778, 3), torch.zeros(1, 3)
    with pytest.raises(ScatError, match="no CPU fallback"):
        r.render(verts, cam)
    with pytest.raises(ScatError, match="no CPU fallback"):
        r.overlay_outputs(torch.zeros(1, 799, 3), cam)
    with pytest.raises(ValueError, match="unknown outputs"):
        r.render(verts, cam, want=("rgb", "normals"))


def test_vertex_face_table_lists_every_face_three_times_ascending():
    from scat_amd.render import MeshRenderer

    _, f = mesh()
    r = MeshRenderer(f, 778)
    off, idx = r.vf_off, r.vf_idx
    assert off.dtype == np.int32 and idx.dtype == np.int32 and off.shape == (779,) and idx.shape == (3 * 1538,)
    assert off[0] == 0 and off[-1] == 3 * 1538 and (np.diff(off) >= 1).all()
    assert np.array_equal(np.bincount(idx, minlength=1538), np.full(1538, 3))
    for v in range(778):
        mine = idx[off[v]:off[v + 1]]
        assert (np.diff(mine) > 0).all() and (f[mine] == v).any(axis=1).all(), v
    # a vertex no face names gets an empty row
    r = MeshRenderer([[0, 1, 3]], 5)
    assert r.vf_off.tolist() == [0, 1, 2, 2, 3, 3] and r.vf_idx.tolist() == [0, 0, 0]


def test_skeleton_overlay_validates_on_the_host():
    from scat_amd._lib import ScatError
    from scat_amd.render import MANO_BONES, SkeletonOverlay

    assert MANO_BONES == RO.MANO_BONES and len(MANO_BONES) == 20
    assert MANO_BONES[:3] == ((0, 1), (1, 2), (2, 3)) and MANO_BONES[15:] == ((3, 16), (6, 17), (9, 18), (12, 19), (15, 20))
    s = SkeletonOverlay()
    assert (s.J, s.NB) == (21, 20) and s.colors.shape == (41, 3) and s.colors.dtype == np.uint8 and s.bones.dtype == np.int32
    assert SkeletonOverlay(bones=(), n_joints=1).NB == 0
    for kw, pattern in ((dict(bones=((0, 21),)), "outside 0..20"), (dict(bones=((-1, 2),)), "outside 0..20"),
                        (dict(n_joints=33), "33 joints"), (dict(n_joints=0), "0 joints"),
                        (dict(bones=((0, 1),) * 33), "33 bones"), (dict(bones=((0.5, 1.0),)), "integer indices"),
                        (dict(colors=np.zeros((41, 3), np.float32)), "colors must be uint8"),
                        (dict(colors=np.zeros((40, 3), np.uint8)), "colors must be uint8")):
        with pytest.raises(ValueError, match=pattern):
            SkeletonOverlay(**kw)
    rgb = torch.zeros(1, 224, 224, 3, dtype=torch.uint8)
    with pytest.raises(ScatError, match="no CPU fallback"):
        s.draw(rgb, torch.zeros(1, 21, 2))
    with pytest.raises(ScatError, match="no CPU fallback"):
        s.draw_outputs(rgb, torch.zeros(1, 66))
    with pytest.raises(ScatError, match="no CPU fallback"):
        s.to("cpu")


def test_ops_wrappers_have_no_cpu_fallback():
    from scat_amd import ops
    from scat_amd._lib import ScatError

    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises(ScatError, match="no CPU fallback"):
        ops.render_project(torch.zeros(1, 3, 3), torch.zeros(1, 3), i32(1, 3), i32(4), i32(3), 16, 16)
    with pytest.raises(ScatError, match="no CPU fallback"):
        ops.render_raster(i32(1, 3, 8), i32(1, 3), 16, 16)
    with pytest.raises(ScatError, match="no CPU fallback"):
        ops.render_skeleton(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), torch.zeros(1, 1, 2), None,
                            torch.zeros(1, 3, dtype=torch.uint8), 1.0, 1.0)
