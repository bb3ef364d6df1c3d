"""The mesh and skeleton renderer on a real MI355X (include/scat_render.h, scat_amd/render.py) against the numpy oracle of
tests/_render_oracle.py: the real MANO topology of tests/golden/hand_mesh.npz in six views, small meshes built for the
coverage rules, the skeleton overlay, the same bytes twice and inside guard bands, and the chain ManoLayer -> MeshRenderer
-> SkeletonOverlay on one stream."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_oracle as RO  # noqa: E402
from _guard import GUARD_NAN_BITS, Arena  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = W = 224
# The header's depth formula evaluated in numpy fp32 against fp64 on the covered pixels of the six views, max |z32 - z64| /
# max |z| of the sample: 1.407e-07 1.350e-07 1.153e-07 8.935e-08 1.702e-07 8.059e-08 (tests/test_render.py recomputes the
# largest).  The kernel's gate is 4 x the largest, the factor DESIGN.md 10 gives the MANO gates for device rounding and
# operation order: 6.808e-07.
E_DEPTH = 1.702e-07
DEPTH_GATE = 4.0 * E_DEPTH
SKELETON_CAP = 0.01      # share of the painted pixels that may sit within 1e-3 px of a radius
T_ = lambda a: torch.from_numpy(np.array(a))      # a copy: the shared references are read-only


def frozen(d):
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def mesh():
    g = np.load(os.path.join(ROOT, "tests", "golden", "hand_mesh.npz"))
    return g["v"], g["f"]


@functools.lru_cache(maxsize=None)
def frames(B, h=H, w=W, seed=7):
    a = np.random.RandomState(seed).randint(0, 256, (B, h, w, 3)).astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def views_case(with_img):
    """the six views in one batch and the oracle's answer, computed once (the frame only shows where no face covers)"""
    v, f = mesh()
    vs, cams = RO.views(v)
    if not with_img:
        return frozen(dict(verts=vs, cam=cams, img=None)), frozen(RO.render(vs, cams, f, H, W, None))
    inp, want = views_case(False)
    img = frames(6)
    rgb = np.where((want["face_id"] >= 0)[..., None], want["rgb"], img)
    return frozen(dict(inp, img=img)), frozen(dict(want, rgb=rgb))


@pytest.fixture(scope="module")
def renderer():
    from scat_amd._lib import lib
    from scat_amd.render import MeshRenderer

    lib().scat_check_device()
    return functools.lru_cache(maxsize=None)(lambda h=H, w=W: MeshRenderer(mesh()[1], 778, size=(h, w), device=DEV))


ALL = ("rgb", "mask", "depth", "face_id", "proj")


def run(r, verts, cam, img=None, cull=False):
    out = r.render(T_(verts).to(DEV), T_(cam).to(DEV), None if img is None else T_(img).to(DEV), cull=cull, want=ALL)
    assert all(t.is_cuda for t in out.values())
    return {k: t.cpu().numpy() for k, t in out.items()}


def held(tag, got, want, verts, img, exact_ids=False):
    """proj, coverage and background exact; face_id exact outside the ambiguity mask (everywhere with exact_ids); depth
    within the gate and rgb within one level on the clear pixels"""
    B, V = verts.shape[:2]
    proj = got["proj"]
    assert proj.shape == (B, V, 8) and proj.dtype == np.int32
    assert np.array_equal(proj[..., 0], want["X"]) and np.array_equal(proj[..., 1], want["Y"]), tag
    assert np.array_equal(proj[..., 6], want["valid"].astype(np.int32)) and (proj[..., 7] == 0).all(), tag
    assert np.array_equal(proj[..., 2].view(np.float32), np.where(want["valid"], verts[..., 2], 0).astype(np.float32)), tag
    e_n = float(np.abs(proj[..., 3:6].view(np.float32) - want["normals"]).max())
    covered = want["face_id"] >= 0
    assert got["mask"].dtype == np.bool_ and np.array_equal(got["mask"], covered), tag
    assert np.array_equal(got["face_id"] >= 0, covered), tag
    clear = covered & (np.ones_like(covered) if exact_ids else ~want["ambiguous"])
    wrong = int((got["face_id"] != want["face_id"])[clear].sum())
    assert np.isposinf(got["depth"][~covered]).all() and np.isfinite(got["depth"][covered]).all(), tag
    same = clear & (got["face_id"] == want["face_id"])
    zmax = np.abs(np.where(want["valid"][..., None], verts, 0)[..., 2]).max(axis=1)
    with np.errstate(invalid="ignore"):      # inf - inf on the background
        d_z = np.abs(got["depth"].astype(np.float64) - want["depth"]) / zmax[:, None, None]
    e_z = float(d_z[same].max()) if same.any() else 0.0
    d_rgb = np.abs(got["rgb"].astype(np.int32) - want["rgb"].astype(np.int32))
    e_rgb = int(d_rgb[same].max()) if same.any() else 0
    print(f"{tag}: {int(covered.sum())} covered, {int(want['ambiguous'].sum())} ambiguous, {wrong} wrong ids on clear pixels, "
          f"depth {e_z:.3e} (gate {DEPTH_GATE:.3e}), rgb off by {e_rgb} levels, {int((d_rgb[same] > 0).sum())} channel values "
          f"differ, normals {e_n:.2e}")
    assert wrong == 0, tag
    assert e_z <= DEPTH_GATE, (tag, e_z)
    assert e_rgb <= 1, (tag, e_rgb)
    bg = np.zeros_like(got["rgb"]) if img is None else img
    assert np.array_equal(got["rgb"][~covered], bg[~covered]), tag


# ------------------------------------------------------------------------------------------------ the hand mesh
@pytest.mark.parametrize("with_img", [True, False])
def test_six_views_match_the_oracle(renderer, with_img):
    inp, want = views_case(with_img)
    got = run(renderer(), inp["verts"], inp["cam"], inp["img"])
    for b, (name, *_) in enumerate(RO.VIEWS):
        held(name, {k: a[b:b + 1] for k, a in got.items()}, {k: a[b:b + 1] for k, a in want.items()}, inp["verts"][b:b + 1],
             None if inp["img"] is None else inp["img"][b:b + 1])
    assert (got["face_id"][4][:, -1] >= 0).any() and (got["face_id"][5] >= 0).sum() == 107      # "clip" leaves the image


def test_front_view_alone(renderer):
    inp, want = views_case(True)
    got = run(renderer(), inp["verts"][:1], inp["cam"][:1], inp["img"][:1])
    held("front, B = 1", got, {k: a[:1] for k, a in want.items()}, inp["verts"][:1], inp["img"][:1])


def test_cull_on_the_hand(renderer):
    v, f = mesh()
    inp, _ = views_case(True)
    vs, cams = inp["verts"][1:3], inp["cam"][1:3]
    want = RO.render(vs, cams, f, H, W, None, cull=True)
    got = run(renderer(), vs, cams, None, cull=True)
    held("tilt and side, cull", got, want, vs, None)
    assert (got["face_id"] >= 0).sum() > 5000


def test_want_selects_the_outputs(renderer):
    inp, want = views_case(False)
    r = renderer()
    out = r.render(T_(inp["verts"][:1]).to(DEV), T_(inp["cam"][:1]).to(DEV), want=("face_id",))
    assert list(out) == ["face_id"] and np.array_equal(out["face_id"].cpu().numpy() >= 0, want["face_id"][:1] >= 0)


# ------------------------------------------------------------------------------------------------ small meshes
@pytest.mark.parametrize("cull", [0, 1])
@pytest.mark.parametrize("name", list(RO.small_meshes()))
def test_small_meshes_hold_to_equality(name, cull):
    from scat_amd.render import MeshRenderer

    verts, faces, (h, w) = RO.small_meshes()[name]
    img = frames(1, h, w)
    want = RO.render(verts[None], RO.UNIT_CAM[None], faces, h, w, img, cull=bool(cull))
    got = run(MeshRenderer(faces, len(verts), size=(h, w), device=DEV), verts[None], RO.UNIT_CAM[None], img, cull=bool(cull))
    assert np.array_equal(got["face_id"], want["face_id"]), name
    held(name, got, want, verts[None], img, exact_ids=True)
    if name == "fan square" and not cull:
        assert (got["face_id"] >= 0).sum() == 100 and len(np.unique(got["face_id"])) == 9
    if name == "NaN vertex" and not cull:
        assert set(np.unique(got["face_id"])) == {-1, 0, 1} and got["proj"][0, 4, 6] == 0
    if name.startswith("coincident") and not cull:
        assert set(np.unique(got["face_id"])) == {-1, 0}
    if name.startswith("near face") and not cull:
        near = 0 if name.endswith("first") else 1
        both = want["count"][0] == 2
        assert both.sum() > 100 and (got["face_id"][0][both] == near).all()


# ------------------------------------------------------------------------------------------------ skeleton
def skeleton_held(tag, got, base, j2d, overlay):
    """got [B,H,W,3] against the oracle painting ``base`` with j2d [B,J,2] (the fp32 values the kernel was given)"""
    painted_all, amb_all, wrong = 0, 0, 0
    for b in range(len(got)):
        want, painted, amb = RO.skeleton(base[b], j2d[b], overlay.bones, overlay.colors, overlay.radius_bone, overlay.radius_joint)
        wrong += int((got[b] != want).any(axis=2)[~amb].sum())
        painted_all, amb_all = painted_all + int(painted.sum()), amb_all + int(amb.sum())
    print(f"{tag}: {painted_all} painted, {amb_all} within the band, {wrong} wrong outside it")
    assert amb_all <= SKELETON_CAP * max(painted_all, 1), tag
    assert wrong == 0, tag
    return painted_all


def test_skeleton_over_the_rendered_hand_and_a_plain_frame(renderer):
    from scat_amd.render import MANO_BONES, SkeletonOverlay, project_outputs

    inp, _ = views_case(True)
    vs, cams = inp["verts"][:2], inp["cam"][:2]
    rgb = renderer().render(T_(vs).to(DEV), T_(cams).to(DEV), T_(inp["img"][:2]).to(DEV), want=("rgb",))["rgb"]
    rgb = torch.cat([rgb, T_(frames(1, seed=9)).to(DEV)])      # views "front" and "tilt", then a plain frame with "tilt"'s joints
    base = rgb.cpu().numpy()
    j3 = np.stack([RO.joints_of(vs[0]), RO.joints_of(vs[1]), RO.joints_of(vs[1])])
    cam3 = np.stack([cams[0], cams[1], cams[1]])
    out66 = T_(np.concatenate([cam3, j3.reshape(3, 63)], axis=1)).to(DEV)
    overlay = SkeletonOverlay(MANO_BONES)
    j2d = project_outputs(out66, H, W).cpu().numpy()
    want2d = np.stack([RO.project_joints(j3[b], cam3[b], H, W) for b in range(3)])
    # four fp32 operations on values below 224: a few ulp of 224 (1.5e-5 px each)
    assert j2d.shape == (3, 21, 2) and np.abs(j2d - want2d).max() < 1e-4
    ret = overlay.draw_outputs(rgb, out66)
    assert ret is rgb and rgb.is_cuda
    n = skeleton_held("hand and plain frame", rgb.cpu().numpy(), base, j2d, overlay)
    assert n > 1500


def test_skeleton_nan_joint_and_single_joint():
    from scat_amd.render import MANO_BONES, SkeletonOverlay

    v, _ = mesh()
    j2d = RO.project_joints(RO.joints_of(v), (8.0, 0.0, 0.0), H, W).astype(np.float32)[None]
    bad = j2d.copy()
    bad[0, 5] = (np.nan, 100.0)
    bad = np.concatenate([bad, j2d])
    bad[1, 16, 1] = np.inf
    base = frames(2, seed=11)
    overlay = SkeletonOverlay(MANO_BONES)
    got = overlay.draw(T_(base).to(DEV), T_(bad).to(DEV)).cpu().numpy()
    skeleton_held("NaN joint", got, base, bad, overlay)
    # the same picture as without joint 5 and its bones (4-5 and 5-6), drawn with the joints' own colours
    keep = [k for k, (a, b) in enumerate(MANO_BONES) if 5 not in (a, b)]
    assert len(keep) == 18
    far = j2d.copy()
    far[0, 5] = (-1000.0, -1000.0)      # finite but nowhere near the frame
    fewer = SkeletonOverlay([MANO_BONES[k] for k in keep], colors=overlay.colors[keep + list(range(20, 41))])
    assert np.array_equal(fewer.draw(T_(base[:1]).to(DEV), T_(far).to(DEV)).cpu().numpy(), got[:1])
    # J = 1, NB = 0, on a frame whose width is no multiple of anything
    one = SkeletonOverlay(bones=(), n_joints=1, colors=np.array([[9, 8, 7]], dtype=np.uint8), radius_joint=3.0)
    base = frames(1, 17, 33)
    p = np.array([[[20.25, 8.75]]], dtype=np.float32)
    got = one.draw(T_(base).to(DEV), T_(p).to(DEV)).cpu().numpy()
    assert skeleton_held("one joint", got, base, p, one) > 20


# ------------------------------------------------------------------------------------------------ determinism and memory
def test_same_call_same_bytes(renderer):
    inp, _ = views_case(True)
    a, b = (run(renderer(), inp["verts"], inp["cam"], inp["img"]) for _ in range(2))
    for k in ALL:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_all_three_kernels_inside_guard_bands(fill):
    """every operand of the three entry points between poisoned bands at pointer skews 0, 1 and 3: fp32 / int32 operands at
    4-byte-aligned addresses that are no multiple of 16, the byte images at odd addresses; bands intact, every output
    element written, results equal to the skew-0 run bit for bit and to the oracle"""
    from scat_amd._lib import lib
    from scat_amd.render import MANO_BONES, MeshRenderer, SkeletonOverlay

    L = lib()
    L.scat_check_device()
    _, f = mesh()
    inp, want = views_case(True)
    B, h, w = 2, H, W
    vs, cams, img = inp["verts"][3:5], inp["cam"][3:5], inp["img"][3:5]      # "back" and "clip"
    r, sk = MeshRenderer(f, 778), SkeletonOverlay(MANO_BONES)
    j2d = np.stack([RO.project_joints(RO.joints_of(vs[b]), cams[b], h, w) for b in range(B)]).astype(np.float32)
    stream = torch.cuda.current_stream().cuda_stream
    arena = Arena(DEV, fill, nbytes=16 << 20)
    runs = {}
    for skew in (0, 1, 3):
        arena.reset()
        words = [arena.place(T_(a), skew, name=n) for n, a in (("verts", vs), ("cam", cams), ("faces", r.faces),
                                                               ("vf_off", r.vf_off), ("vf_idx", r.vf_idx),
                                                               ("lights", r.lights), ("j2d", j2d), ("bones", sk.bones))]
        d_verts, d_cam, d_faces, d_off, d_idx, d_lights, d_j2d, d_bones = words
        proj = arena.place((B, 778, 8), skew, torch.int32, name="proj", out=True)
        face_id = arena.place((B, h, w), skew, torch.int32, name="face_id", out=True)
        depth = arena.place((B, h, w), skew, name="depth", out=True, finite=False)      # +inf is the background's depth
        assert all(t.data_ptr() % 16 == 4 * skew for t in words + [proj, face_id, depth])

        def bytes_at(a, name, out=False):
            """a byte tensor whose first element sits ``skew`` bytes into its slot: an odd address for skews 1 and 3"""
            n = int(np.prod(a if out else a.shape))
            slot = arena.place((n + skew,), skew, torch.uint8, name=name, out=True)
            lead = slot[:skew].clone()
            body = slot[skew:]
            if not out:
                body.copy_(T_(a).reshape(-1))
            assert body.data_ptr() % 4 == skew % 4
            return slot, lead, body

        s_img, l_img, d_img = bytes_at(img, "img")
        s_col, l_col, d_col = bytes_at(sk.colors, "colors")
        s_rgb, l_rgb, d_rgb = bytes_at((B, h, w, 3), "rgb", out=True)
        L.scat_render_project(d_verts.data_ptr(), d_cam.data_ptr(), d_faces.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(),
                              proj.data_ptr(), B, 778, 1538, h, w, stream)
        assert L.scat_last_kernel() == b"render_project_v778"
        L.scat_render_raster(proj.data_ptr(), d_faces.data_ptr(), d_img.data_ptr(), d_lights.data_ptr(), face_id.data_ptr(),
                             depth.data_ptr(), d_rgb.data_ptr(), B, 778, 1538, h, w, 3, *r.base_rgb, r.ambient, 0, stream)
        assert L.scat_last_kernel() == b"render_raster_f1538_rgb"
        torch.cuda.synchronize()
        mesh_rgb = d_rgb.cpu().numpy().reshape(B, h, w, 3).copy()
        L.scat_render_skeleton(d_j2d.data_ptr(), d_bones.data_ptr(), d_col.data_ptr(), d_rgb.data_ptr(), B, 21, 20, h, w,
                               sk.radius_bone, sk.radius_joint, stream)
        assert L.scat_last_kernel() == b"render_skeleton_j21_b20"
        torch.cuda.synchronize()
        arena.check()
        for slot, lead in ((s_img, l_img), (s_col, l_col), (s_rgb, l_rgb)):
            assert torch.equal(slot[:skew], lead)      # the bytes in front of an odd-address image are still the guard's
        for t in (proj, face_id, depth):
            assert not bool((t.view(torch.int32) == GUARD_NAN_BITS).any())      # every word written
        runs[skew] = dict(proj=proj.cpu().numpy().copy(), face_id=face_id.cpu().numpy().copy(), depth=depth.cpu().numpy().copy(),
                          rgb=mesh_rgb, drawn=d_rgb.cpu().numpy().reshape(B, h, w, 3).copy())
    got = dict(runs[0], mask=runs[0]["face_id"] >= 0)
    held(f"guard {fill}", got, {k: a[3:5] for k, a in want.items()}, vs, img)
    skeleton_held(f"guard {fill} skeleton", runs[0]["drawn"], runs[0]["rgb"], j2d, sk)
    for skew in (1, 3):
        for k, a in runs[0].items():
            assert a.tobytes() == runs[skew][k].tobytes(), (skew, k)


# ------------------------------------------------------------------------------------------------ composition
def test_mano_layer_to_renderer_to_skeleton_on_one_stream(renderer):
    """ManoModel.synthetic with the fixture's faces: ManoLayer -> MeshRenderer.overlay_outputs -> SkeletonOverlay
    .draw_outputs over a preprocess_u8 frame, all on a side stream and on the device; checked against the oracle fed the
    layer's own output"""
    from scat_amd import ops, synth
    from scat_amd.mano import ManoLayer, ManoModel
    from scat_amd.render import SkeletonOverlay, project_outputs, to_uint8_hwc

    _, f = mesh()
    B, seed = 2, 410
    layer = ManoLayer(ManoModel.synthetic(seed, V=778).to(DEV))
    rots, poses, betas = (T_(synth.normal_like(seed, n, (B, k), s)).to(DEV) for n, k, s in (("rots", 3, 0.8), ("poses", 45, 0.4),
                                                                                              ("betas", 10, 1.0)))
    cam = T_(np.array([[3.5, 0.02, -0.03], [2.5, -0.1, 0.05]], dtype=np.float32)).to(DEV)
    src = T_(frames(B, 96, 128, seed=13).transpose(0, 3, 1, 2).copy()).to(DEV)      # uint8 [B,3,96,128]
    overlay = SkeletonOverlay()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        x3d = layer(rots, poses, betas)
        frame = to_uint8_hwc(ops.preprocess_u8(src))
        out = renderer().overlay_outputs(x3d, cam, frame, want=ALL)
        mesh_rgb = out["rgb"].clone()
        out66 = torch.cat([cam, x3d[:, :21].reshape(B, 63)], dim=1)
        drawn = overlay.draw_outputs(out["rgb"], out66)
        j2d = project_outputs(out66, H, W)
    side.synchronize()
    assert all(t.is_cuda for t in (x3d, frame, mesh_rgb, drawn, *out.values()))
    assert frame.dtype == torch.uint8 and tuple(frame.shape) == (B, H, W, 3)
    verts, img = x3d[:, 21:].cpu().numpy(), frame.cpu().numpy()
    want = RO.render(verts, cam.cpu().numpy(), f, H, W, img)
    got = {k: t.cpu().numpy() for k, t in out.items()}
    got["rgb"] = mesh_rgb.cpu().numpy()
    held("composition", got, want, verts, img)
    assert (want["face_id"] >= 0).sum() > 1000
    skeleton_held("composition skeleton", drawn.cpu().numpy(), got["rgb"], j2d.cpu().numpy(), overlay)
