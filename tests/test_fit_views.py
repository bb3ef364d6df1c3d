"""The MANO fit to keypoints in calibrated views, the parts that need no GPU: the public header in include_ext/ and its
binding, every argument refusal of both entry points, the Python refusals, and the fp64 oracle of
tests/_fit_views_oracle.py against autograd and against itself: the kernel's per-joint 3 x 3 form against the stacked rows,
the triangulation on noise-free keypoints and on rays it must refuse, project_points against triangulate,
Cameras.weak_perspective against the pinhole, and that the fixed inputs of the GPU tests (tests/test_gpu_fit_views.py) are
fit for their gates."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_views_cases as C  # noqa: E402
import _fit_views_oracle as VO  # noqa: E402
from _fit_cases import JOINT_MAP, host_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS_H = os.path.join(ROOT, "include_ext", "scat_mano_fit_views.h")
PARENTS = sum(p << (4 * i) for i, p in enumerate((0, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)))
FIT, TRI = "scat_mano_fit_views", "scat_triangulate"


@pytest.fixture(scope="module")
def built():
    from scat_amd import build

    return build.build(verbose=False)


def test_views_header_declares_the_two_and_collides_with_no_other(built):
    from scat_amd import build, fit
    from scat_amd._lib import EXTENSION_HEADERS, HEADERS, lib, parse_header

    assert os.path.samefile(fit.FIT_VIEWS_HEADER, VIEWS_H)
    protos = parse_header(VIEWS_H)
    assert set(protos) == {FIT, TRI}
    others = list(HEADERS) + list(EXTENSION_HEADERS) + [os.path.join(ROOT, "include", h) for h in sorted(os.listdir(os.path.join(ROOT, "include")))]
    for h in others:
        assert not set(protos) & set(parse_header(h)), h
    names = {n: [an for _, an in protos[n][1]] for n in protos}
    by = {n: dict((an, ty) for ty, an in protos[n][1]) for n in protos}
    assert names[FIT][:15] == ["blend", "joint_t", "joint_s", "weights_t", "hands_mean", "cams", "cam_batch", "targets2", "weights2",
                               "joint_map", "pose_lo", "pose_hi", "p", "cost", "accepted"]
    assert names[FIT][15:18] == ["B", "C", "V"] and names[FIT][-1] == "stream" and "ws" not in names[FIT]
    assert names[TRI] == ["cams", "cam_batch", "targets2", "weights2", "points", "valid", "B", "C", "z_near", "stream"]
    assert by[FIT]["parents"] is ctypes.c_uint64 and by[FIT]["free_mask"] is ctypes.c_uint64 and by[FIT]["cam_batch"] is ctypes.c_int
    for n in ("lambda0", "w_pose", "w_beta", "w_limit", "sigma2", "z_near"):
        assert by[FIT][n] is ctypes.c_float, n
    assert by[TRI]["z_near"] is ctypes.c_float and protos[FIT][0] is ctypes.c_int and protos[TRI][0] is ctypes.c_int
    src = open(VIEWS_H).read()
    assert f"#define SCAT_FIT_VIEWS_MAX_C {fit.VIEWS_MAX_C}\n" in src and "CLAMPED" in src and "UNITS" in src and "theta^2 / 8" in src
    for doc in (fit.ManoFitter.fit_keypoints_views.__doc__,):
        assert "UNITS" in doc and "BEHIND THE CAMERA" in doc and "ot fitted" in doc
    # the second directory: named in build.py, refused when missing, a rebuild trigger of the library and of every object
    assert build.EXT_HEADERS == ("scat_mano_fit_views.h",) and os.path.samefile(build.INCLUDE_EXT, os.path.dirname(VIEWS_H))
    assert build._deps_mtime() >= build._ext_headers_mtime() >= os.path.getmtime(VIEWS_H)
    assert not os.path.exists(os.path.join(ROOT, "include", "scat_mano_fit_views.h"))
    L = lib()
    ns = L.bind(VIEWS_H)
    assert sorted(vars(ns)) == [FIT, TRI] and L.bind(VIEWS_H) is ns and all(callable(f) for f in vars(ns).values())
    assert hasattr(L.cdll, FIT) and hasattr(L.cdll, TRI)


GOOD = dict(cam_batch=1, B=4, C=3, V=778, parents=PARENTS, tips=[320, 443, 671, 554, 744], iters=20, init=1, lambda0=1e-3, w_pose=1e-2,
            w_beta=1e-2, w_limit=1e2, sigma2=10.0, z_near=1e-3, free=(1 << 62) - 1)
NPTR = 14      # blend .. hands_mean, cams, targets2, weights2, joint_map, pose_lo, pose_hi, p, cost, accepted
OPTIONAL = {7: "weights2", 9: "pose_lo", 10: "pose_hi"}


def _fit(ns, **kw):
    a = dict(GOOD, ptrs=[8 * (i + 1) for i in range(NPTR)])
    a.update(kw)
    p = a["ptrs"]
    return ns.scat_mano_fit_views(*p[:6], a["cam_batch"], *p[6:], a["B"], a["C"], a["V"], a["parents"], *a["tips"], a["iters"], a["init"],
                                  a["lambda0"], a["w_pose"], a["w_beta"], a["w_limit"], a["sigma2"], a["z_near"], a["free"], 0)


def _tri(ns, **kw):
    a = dict(cam_batch=1, B=4, C=3, z_near=1e-3, ptrs=[8 * (i + 1) for i in range(5)])      # cams, targets2, weights2, points, valid
    a.update(kw)
    p = a["ptrs"]
    return ns.scat_triangulate(p[0], a["cam_batch"], *p[1:], a["B"], a["C"], a["z_near"], 0)


def test_views_errors_surface_without_a_gpu(built):
    """argument validation happens before any HIP call: made-up pointers are never followed, each refusal carries its
    SCAT_E_* code and names the entry point and the argument, and the kernel label does not move"""
    from scat_amd import mano
    from scat_amd._lib import ScatError, lib

    L = lib()
    ns = L.bind(VIEWS_H)
    label = L.scat_last_kernel()

    def refused(call, entry, code, pattern, **kw):
        with pytest.raises(ScatError, match=rf"{entry} failed \({code}\): {entry}: .*{pattern}"):
            call(ns, **kw)
        assert L.scat_last_kernel() == label

    base = [8 * (i + 1) for i in range(NPTR)]
    without = lambda *idx: [0 if i in idx else v for i, v in enumerate(base)]
    for i in range(NPTR):
        if i not in OPTIONAL:
            refused(_fit, FIT, -2, "null pointer", ptrs=without(i))
        refused(_fit, FIT, -2, "4-byte aligned", ptrs=base[:i] + [base[i] + 2] + base[i + 1:])
    refused(_fit, FIT, -2, "pose_lo and pose_hi must both", ptrs=without(9))
    refused(_fit, FIT, -2, "pose_lo and pose_hi must both", ptrs=without(10))
    refused(_fit, FIT, -1, "batch 0 must be positive", B=0)
    refused(_fit, FIT, -1, "0 vertices outside", V=0)
    refused(_fit, FIT, -1, rf"{mano.MAX_V + 1} vertices outside 1\.\.{mano.MAX_V}", V=mano.MAX_V + 1)
    refused(_fit, FIT, -1, "tip 2 = 778", tips=[320, 443, 778, 554, 744])
    refused(_fit, FIT, -2, r"parent\[3\] = 7", parents=(PARENTS & ~(15 << 12)) | (7 << 12))
    refused(_fit, FIT, -2, r"0 iterations outside 1\.\.64", iters=0)
    refused(_fit, FIT, -2, r"65 iterations outside 1\.\.64", iters=65)
    refused(_fit, FIT, -2, "init 2 must be 0", init=2)
    refused(_fit, FIT, -2, "init -1 must be 0", init=-1)
    for lam in ("0", "-1", "nan", "inf"):
        refused(_fit, FIT, -2, f"lambda0 {lam} outside", lambda0=float(lam))
    for name in ("w_pose", "w_beta", "w_limit", "sigma2"):
        refused(_fit, FIT, -2, f"{name} -1 must be finite and not negative", **{name: -1.0})
        refused(_fit, FIT, -2, f"{name} inf must be finite", **{name: float("inf")})
        refused(_fit, FIT, -2, f"{name} nan must be finite", **{name: float("nan")})
    refused(_fit, FIT, -2, "free_mask has bits above 61 set", free=1 << 62)
    refused(_fit, FIT, -2, "free_mask has bits above 61 set", free=1 << 63)
    tbase = [8 * (i + 1) for i in range(5)]
    for i in range(5):
        if i != 2:
            refused(_tri, TRI, -2, "null pointer", ptrs=[0 if k == i else v for k, v in enumerate(tbase)])
        refused(_tri, TRI, -2, "4-byte aligned", ptrs=tbase[:i] + [tbase[i] + 2] + tbase[i + 1:])
    refused(_tri, TRI, -1, "batch 0 must be positive", B=0)
    for call, entry in ((_fit, FIT), (_tri, TRI)):      # what both check of the rig
        refused(call, entry, -1, r"0 views outside 1\.\.8", C=0)
        refused(call, entry, -1, r"9 views outside 1\.\.8", C=9)
        refused(call, entry, -1, "cam_batch 2 must be 1", cam_batch=2)
        refused(call, entry, -1, "cam_batch 0 must be 1", cam_batch=0)
        for z in ("0", "-1", "nan", "inf"):
            refused(call, entry, -2, f"z_near {z} must be positive and finite", z_near=float(z))


def _cameras(C_, Bc=1, dtype=torch.float32):
    from scat_amd.fit import Cameras

    c = C.rig(C_, Bc).to(dtype)
    return Cameras(c[:, :, :9].reshape(Bc, C_, 3, 3), c[:, :, 9:12], c[:, :, 12:16])


def test_python_refusals_and_no_cpu_fallback():
    from scat_amd._lib import ScatError
    from scat_amd.fit import Cameras, FitResult, ManoFitter
    from scat_amd.mano import ManoModel

    f = ManoFitter(ManoModel.synthetic(1, V=37), joint_map=JOINT_MAP)
    cams = _cameras(3)
    assert torch.equal(cams.packed(), C.rig(3)) and cams.check() == (1, 3)
    kp = torch.zeros(2, 3, 21, 2)
    for call in (lambda: f.fit_keypoints_views(kp, cams), lambda: f.triangulate(kp, cams)):
        with pytest.raises(ScatError, match="no CPU fallback"):
            call()
    p = torch.zeros(2, 62)
    with pytest.raises(ScatError, match="no CPU fallback"):
        f.project_views(FitResult(p[:, 0:3], p[:, 3:48], p[:, 48:58], p[:, 58:61], torch.exp(p[:, 61]), None, None, p), cams)
    with pytest.raises(ScatError, match="Cameras"):
        f.fit_keypoints_views(kp, C.rig(3))
    R, t, K = cams
    for bad, pat in ((Cameras(R.double(), t, K), "fp32"), (Cameras(R[:, :2], t, K), r"R \[Bc,C,3,3\]"), (Cameras(R, t, K[..., :3]), r"K \[Bc,C,4\]"),
                     (Cameras(R.repeat(1, 3, 1, 1), t.repeat(1, 3, 1), K.repeat(1, 3, 1)), r"C in 1\.\.8")):
        with pytest.raises(ScatError, match=pat):
            bad.packed()
        with pytest.raises(ScatError, match=pat):
            f.fit_keypoints_views(kp, bad)
    with pytest.raises(ScatError, match=r"view 3 outside 0\.\.2"):
        cams.weak_perspective(3, 0.5, (640, 640))
    with pytest.raises(ScatError, match="one scale"):      # fx = fy in a frame that is not square
        cams.weak_perspective(0, 0.5, (480, 640))
    with pytest.raises(ScatError, match="depth must be positive"):
        cams.weak_perspective(0, 0.0, (640, 640))


def test_oracle_jacobian_and_gradient_against_autograd():
    """the stacked rows' Jacobian is autograd's, and with the IRLS weights g is half the gradient of the robust cost with
    active limits; a frozen unknown is a unit row"""
    V, B, Cn = 37, 3, 3
    m, pr, P1 = host_model(V), C.problem("gm_limits", V, B, Cn), C.near_start(V, B, Cn)
    assert int((VO.excess(P1, pr) != 0).sum()) >= 3
    J, r, wr = VO.stacked_rows(m, P1, pr)
    assert J.shape == (B, 42 * Cn, 62) and float(wr.min()) < 0.1 and float(wr.max()) > 0.5      # outliers down, inliers not
    eps, k = 1e-6, 7      # one column by central differences as a check on the check
    d = torch.zeros_like(P1)
    d[:, k] = eps
    with torch.no_grad():
        fd = (VO.terms(m, P1 + d, pr)[0] - VO.terms(m, P1 - d, pr)[0]).reshape(B, -1) / (2 * eps)
    assert VO.rel(J[:, :, k].numpy(), fd.numpy()) < 1e-7
    _, g = VO.normal_equations(m, P1, pr)
    Pq = P1.clone().requires_grad_(True)
    VO.cost(m, Pq, pr).sum().backward()
    e = VO.rel(g.numpy(), 0.5 * Pq.grad.numpy())
    print(f"g against half the autograd gradient: {e:.3e}")
    assert e < 1e-12
    A, g = VO.normal_equations(m, P1, pr, free=C.ALL & ~(1 << 5))
    assert bool((g[:, 5] == 0).all()) and bool((A[:, 5, 5] == 1).all()) and bool((A[:, 5, :5] == 0).all())


@pytest.mark.parametrize("name,Cn,per", [("quad", 2, False), ("gm_limits", 3, True), ("gm", 8, False), ("quad", 1, False)])
def test_metric_form_equals_the_stacked_form(name, Cn, per):
    """A = sum_j G_j^T M_j G_j and g = sum_j G_j^T h_j, the kernel's form, are the stacked 42 C rows' normal equations"""
    V, B = 37, 3
    m, pr, P1 = host_model(V), C.problem(name, V, B, Cn, per), C.near_start(V, B, Cn, per)
    w2 = torch.ones(B, Cn, 21)
    w2[:, 0, 4], w2[1, Cn - 1, 9] = 0.0, 0.5
    pr = pr._replace(w2=w2)
    A, g = VO.normal_equations(m, P1, pr)
    A2, g2 = VO.metric_equations(m, P1, pr)
    ea, eg = VO.rel(A2.numpy(), A.numpy()), VO.rel(g2.numpy(), g.numpy())
    print(f"{name} C {Cn}: A {ea:.3e}, g {eg:.3e}")
    assert ea < 1e-12 and eg < 1e-12


def test_triangulation_returns_noise_free_joints_and_refuses_what_it_must():
    V, B = 37, 3
    for Cn, per in ((2, False), (3, True), (8, False)):
        _, X3, T2, _ = C.truth(V, B, Cn, per)
        pr = VO.Problem(JOINT_MAP, C.rig(Cn, B if per else 1, dtype=np.float64), T2)
        with torch.no_grad():      # cameras and pixels in fp64, so that the only error is the solve's
            pr = pr._replace(T2=VO.reproject(host_model(V), C.truth(V, B, Cn, per)[0], pr))
        pts, valid = VO.triangulate(pr)
        e = float((pts - X3).abs().max())
        print(f"C {Cn}: noise-free joints to {e:.3e} m")
        assert bool(valid.all()) and e < 1e-10
    # a joint seen by one view only, and by none; the others are not affected
    w2 = torch.ones(B, 3, 21)
    w2[0, 1:, 5], w2[1, :, 6] = 0.0, 0.0
    pr = C.problem("quad", V, B, 3)._replace(w2=w2)
    pts, valid = VO.triangulate(pr)
    want = torch.ones(B, 21, dtype=torch.bool)
    want[0, 5] = want[1, 6] = False
    assert torch.equal(valid, want) and bool((pts[0, 5] == 0).all()) and bool((pts[1, 6] == 0).all())
    # parallel rays: the same camera twice; 0.3 mrad apart is still refused (theta^2 / 8 = 1e-8 of the trace, and the pivot
    # is at most 12 times that here, where the rays are 0.3 rad off the x axis), 10 mrad is not
    for angle, ok in ((0.0, False), (3e-4, False), (1e-2, True)):
        a, b = C.look_at(0.3), C.look_at(0.3 + angle)
        cams = torch.tensor(np.stack([a, b])[None], dtype=torch.float64)
        X = torch.zeros(1, 21, 3, dtype=torch.float64)
        X[0, :, 1] = torch.linspace(-0.05, 0.05, 21)
        R, t, K = VO.rig(VO.Problem(JOINT_MAP, cams, torch.zeros(1, 2, 21, 2)), 1, torch.float64)
        T2 = VO.pinhole(VO.in_camera(X, R, t), K)
        _, valid = VO.triangulate(VO.Problem(JOINT_MAP, cams, T2))
        assert bool(valid.all()) == ok and bool(valid.any()) == ok, angle
    # a point behind its cameras: every camera turned by pi about its own y axis sees the same lines under pixels mirrored
    # in y, and the rays meet where they did, now at q.z < 0
    _, X3, T2, cams = C.truth(V, B, 2)
    back, T2b = cams.clone(), T2.clone()
    for k in (0, 1, 2, 6, 7, 8, 9, 11):      # rows 0 and 2 of R, t.x and t.z
        back[:, :, k] = -back[:, :, k]
    T2b[..., 1] = 2 * C.CENTRE[1] - T2b[..., 1]
    assert float((VO.triangulate(VO.Problem(JOINT_MAP, back, T2b, z_near=-10.0))[0] - VO.triangulate(VO.Problem(JOINT_MAP, cams, T2))[0]).abs().max()) < 1e-6
    pts, valid = VO.triangulate(VO.Problem(JOINT_MAP, back, T2b))
    assert not bool(valid.any()) and bool((pts == 0).all())
    # an unusable sample has no valid joint
    bad = T2.clone()
    bad[1, 0, 3, 0] = float("nan")
    _, valid = VO.triangulate(VO.Problem(JOINT_MAP, cams, bad))
    assert not bool(valid[1].any()) and bool(valid[0].all()) and bool(valid[2].all())


def test_project_points_inverts_triangulate():
    from scat_amd.fit import project_points

    V, B, Cn = 37, 3, 3
    for per in (False, True):
        _, X3, T2, _ = C.truth(V, B, Cn, per)
        cams = _cameras(Cn, B if per else 1, torch.float64)
        pts, valid = VO.triangulate(VO.Problem(JOINT_MAP, C.rig(Cn, B if per else 1), T2))
        uv = project_points(pts, cams)
        e = float((uv - T2.double()).abs().max())
        print(f"per-sample rigs {per}: reprojected triangulation against the pixels {e:.3e} px")
        assert uv.shape == (B, Cn, 21, 2) and bool(valid.all()) and e < 1e-3      # fp32 pixels of a 640 frame
        with torch.no_grad():
            assert float((uv - VO.reproject(host_model(V), C.truth(V, B, Cn, per)[0], C.problem("quad", V, B, Cn, per)._replace(
                cams=C.rig(Cn, B if per else 1))).double()).abs().max()) < 1e-3


def test_weak_perspective_matches_the_pinhole_on_its_plane():
    from scat_amd.render import project_outputs

    cams = _cameras(3)
    H, W, depth = 640, 640, 0.5      # fx = fy wants a square frame: the renderer's scale is per half frame
    R, t, cam = cams.weak_perspective(1, depth, (H, W))
    assert R.shape == (1, 3, 3) and t.shape == (1, 3) and cam.shape == (1, 3)
    assert abs(float(cam[0, 0]) - C.FOCAL / (depth * W / 2)) < 1e-6 and abs(float(cam[0, 1])) < 1e-6      # cx is the centre, cy is not
    q = torch.tensor([[0.03, -0.02, depth], [-0.05, 0.04, depth], [0.0, 0.0, depth]])      # camera frame, on the plane
    K = cams.K[0, 1]
    pin = torch.stack([K[0] * q[:, 0] / q[:, 2] + K[2], K[1] * q[:, 1] / q[:, 2] + K[3]], dim=1)
    weak = project_outputs(torch.cat([cam, q.reshape(1, 9)], dim=1), H, W)[0]
    assert float((weak - pin).abs().max()) < 1e-3
    off = cams._replace(K=cams.K + torch.tensor([0.0, 0.0, 12.0, -7.0]))      # a principal point off the centre
    _, _, cam = off.weak_perspective(1, depth, (H, W))
    weak = project_outputs(torch.cat([cam, q.reshape(1, 9)], dim=1), H, W)[0]
    assert float((weak - (pin + torch.tensor([12.0, -7.0]))).abs().max()) < 1e-3
    # off the plane the two differ, by the perspective
    far = q + torch.tensor([0.0, 0.0, 0.1])
    weak = project_outputs(torch.cat([cams.weak_perspective(1, depth, (H, W))[2], far.reshape(1, 9)], dim=1), H, W)[0]
    assert float((weak[:2] - torch.stack([K[0] * far[:, 0] / far[:, 2] + K[2], K[1] * far[:, 1] / far[:, 2] + K[3]], 1)[:2]).abs().max()) > 1.0


def test_conditions_on_the_fixed_inputs():
    """what the GPU gates lean on, on the oracle: every one-step case accepts its step, the fp64 oracle converges on the
    recovery case, and the outliers split the robust loss from the quadratic one"""
    import test_gpu_fit_views as G

    for name, V, B, Cn, per in G.STEPS:
        if B <= 3:
            assert C.run(name, V, B, Cn, per, 1)[2].tolist() == [1] * B, (name, V, B, Cn)
    _, j64, p64 = C.recovery("quad")
    print(f"recovery, fp64: joint RMS mm {1e3 * j64}, pixel RMS {p64}")
    assert (j64 < 1e-5).all() and (p64 < 1e-2).all()      # a hundredth of a millimetre, a hundredth of a pixel
    _, jg, pg = C.recovery("gm_outliers")
    _, jq, pq = C.recovery("quad_outliers")
    _, jg32, pg32 = C.recovery("gm_outliers", torch.float32)
    print(f"one view of outliers: joint RMS mm, Geman-McClure {1e3 * jg}, quadratic {1e3 * jq}")
    assert (jg <= 4 * jg32).all() and (pg <= 4 * pg32).all() and (jq > 4 * jg32).all() and (pq > 4 * pg32).all()
    pr, _, valid, _ = C.validity_case()
    assert not bool(valid[0, 5]) and not bool(valid[1, 6]) and not bool(valid[2, 8]) and int(valid.sum()) == 3 * 21 - 3
    assert math.isclose(C.RADIUS, 0.5) and C.FOCAL == 600.0 and C.CENTRE == (320.0, 240.0)
