"""The MANO fit to keypoints in calibrated views on a real MI355X (include_ext/scat_mano_fit_views.h, scat_amd/fit.py)
against the fp64 oracle of tests/_fit_views_oracle.py and inside guard bands.  Inputs come from tests/_fit_views_cases.py.

Every gate that compares fp32 with fp64 is 4 x the error of the oracle itself run in fp32 on the CPU against its fp64 run
on the same inputs (E32 below, printed by tools/fit_views_gates.py), max |a - b| / max |b|: the project's rule for the MANO
gates.  The recovery gates are on joints and reprojections, never on parameters, and are 4 x what the fp32 oracle reaches
on the same case, per sample."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_views_cases as C  # noqa: E402
import _fit_views_oracle as VO  # noqa: E402
from _fit_cases import JOINT_MAP, host_model  # noqa: E402
from _guard import Arena  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = C.ALL
# V = 37: less than one wavefront and odd; V = 778: MANO.  B = 65: more workgroups than one wave of them is wide.
# (V, B, C, a rig per sample)
STARTS = [(37, 1, 2, False), (778, 3, 3, True), (37, 65, 8, False), (37, 3, 2, True)]
# (problem, V, B, C, a rig per sample); C = 1 has no closed-form start and is entered with init = 0, as every step is
STEPS = [("quad", 37, 3, 2, False), ("gm", 37, 3, 3, True), ("limits", 37, 3, 8, False), ("quad", 37, 1, 1, False),
         ("quad", 778, 3, 3, False), ("gm", 37, 65, 3, True)]
COST = ("gm_limits", 37, 3, 3)
# The oracle in fp32 on the CPU against itself in fp64, max |a - b| / max |b|, as tools/fit_views_gates.py printed them.
#   tri      the triangulated joints of _fit_views_cases.start_case(V, B, C, per): the fp64 solve rounded to fp32
#            ("tri", "validity"): those of _fit_views_cases.validity_case()
#   start    p of the closed-form start of the same case
#   step     the accepted p after one LM step from near_start on problem(name, V, B, C, per) (lambda 1e-2)
#   cost     the oracle's cost function at its own iterate after k iterations of the gm_limits problem, V = 37, C = 3
E32 = {
    ("tri", 37, 1, 2, False): 3.242e-08, ("start", 37, 1, 2, False): 6.181e-08,
    ("tri", 778, 3, 3, True): 2.032e-08, ("start", 778, 3, 3, True): 2.879e-08,
    ("tri", 37, 65, 8, False): 4.375e-08, ("start", 37, 65, 8, False): 3.921e-08,
    ("tri", 37, 3, 2, True): 3.279e-08, ("start", 37, 3, 2, True): 5.734e-08,
    ("tri", "validity"): 3.277e-08,
    ("step", "quad", 37, 3, 2, False): 1.451e-06, ("step", "gm", 37, 3, 3, True): 2.506e-06,
    ("step", "limits", 37, 3, 8, False): 6.855e-06, ("step", "quad", 37, 1, 1, False): 3.577e-06,
    ("step", "quad", 778, 3, 3, False): 7.028e-06, ("step", "gm", 37, 65, 3, True): 4.314e-06,
    ("cost", 1): 6.217e-08, ("cost", 2): 7.433e-08, ("cost", 5): 5.044e-08, ("cost", 10): 9.754e-08,
}


def e32_keys():
    return [(k,) + s for s in STARTS for k in ("tri", "start")] + [("tri", "validity")] + [("step",) + s for s in STEPS] + \
        [("cost", k) for k in (1, 2, 5, 10)]


def model(V):
    m = host_model(V)
    return m if m.device is not None else m.to(DEV)


@pytest.fixture(scope="module", autouse=True)
def device():
    from scat_amd._lib import lib

    lib().scat_check_device()


d_ = lambda t: None if t is None else t.float().contiguous().to(DEV)


def vfit(V, pr, free, iters, P0=None, lambda0=1e-2):
    """the entry point as declared, on a Problem of the oracle -> p [B,62], cost [B], accepted [B] on the host"""
    from scat_amd.fit import mano_fit_views

    B = pr.T2.shape[0]
    p = torch.empty(B, 62, device=DEV) if P0 is None else P0.float().contiguous().to(DEV)
    jm = torch.tensor(pr.joint_map, dtype=torch.int32, device=DEV)
    cost, acc = mano_fit_views(model(V), d_(pr.cams), d_(pr.T2), d_(pr.w2), jm, d_(pr.lo), d_(pr.hi), p, iters, 0 if P0 is not None else 1,
                               lambda0, pr.w_pose, pr.w_beta, pr.w_limit, pr.sigma2, pr.z_near, free)
    return p.cpu(), cost.cpu(), acc.cpu()


def held(tag, got, want, e32):
    e = VO.rel(got.numpy(), want.numpy())
    print(f"{tag}: {e:.3e} (gate {4 * e32:.3e} = 4 x {e32:.3e})")
    assert torch.isfinite(got).all(), tag
    assert e <= 4 * e32, (tag, e, 4 * e32)


def test_e32_covers_the_cases():
    assert sorted(map(repr, E32)) == sorted(map(repr, e32_keys()))


@pytest.mark.parametrize("V,B,Cn,per", STARTS)
def test_triangulation_and_start_match_the_oracle(V, B, Cn, per):
    """scat_triangulate, and init = 1 with everything frozen, which returns the closed-form start; both forms of cam_batch"""
    from scat_amd.fit import triangulate_views

    pr, pts64, valid64, P64, _, _ = C.start_case(V, B, Cn, per)
    assert pr.cams.shape[0] == (B if per else 1) and bool(valid64.all())
    pts, valid = triangulate_views(d_(pr.cams), d_(pr.T2), None, pr.z_near)
    assert valid.dtype == torch.int32 and torch.equal(valid.cpu().bool(), valid64) and int(valid.max()) == 1
    held(f"triangulated joints V {V} B {B} C {Cn}", pts.cpu().double(), pts64, E32[("tri", V, B, Cn, per)])
    p, cost, acc = vfit(V, pr, 0, 1)
    assert acc.tolist() == [0] * B and bool(torch.isfinite(cost).all())
    held(f"start V {V} B {B} C {Cn}", p.double(), P64, E32[("start", V, B, Cn, per)])
    with torch.no_grad():      # the start's cost is the oracle's at the returned p
        want = VO.cost(host_model(V), p.double(), pr)
    assert VO.rel(cost.double().numpy(), want.numpy()) < 1e-4


def test_triangulation_validity_is_exact():
    """single-view joints, joints no view sees, rays 0.3 mrad apart and a NaN sample: valid is the oracle's, invalid points 0"""
    from scat_amd.fit import triangulate_views

    pr, pts64, valid64, _ = C.validity_case()
    assert not bool(valid64[0, 5]) and not bool(valid64[1, 6]) and not bool(valid64[2, 8]) and int(valid64.sum()) == 3 * 21 - 3
    pts, valid = triangulate_views(d_(pr.cams), d_(pr.T2), d_(pr.w2), pr.z_near)
    assert torch.equal(valid.cpu().bool(), valid64) and bool((pts.cpu()[~valid64] == 0).all())
    held("triangulated joints with weights", pts.cpu().double(), pts64, E32[("tri", "validity")])
    bad = pr.T2.clone()
    bad[1, 2, 3, 1] = float("nan")
    pts, valid = triangulate_views(d_(pr.cams), d_(bad), d_(pr.w2), pr.z_near)
    assert not bool(valid[1].any()) and bool((pts[1] == 0).all()) and torch.equal(valid.cpu().bool()[[0, 2]], valid64[[0, 2]])


@pytest.mark.parametrize("name,V,B,Cn,per", STEPS)
def test_one_step_matches_the_oracle(name, V, B, Cn, per):
    pr = C.problem(name, V, B, Cn, per)
    want, _, acc64 = C.run(name, V, B, Cn, per, 1)
    assert acc64.tolist() == [1] * B
    if name == "limits":
        assert bool(((VO.excess(C.near_start(V, B, Cn, per), pr) != 0).sum(1) >= 1).all())
    p, cost, acc = vfit(V, pr, ALL, 1, C.near_start(V, B, Cn, per))
    assert acc.tolist() == [1] * B
    held(f"one step {name} V {V} B {B} C {Cn}", p.double(), want, E32[("step", name, V, B, Cn, per)])


def test_cost_is_monotone_and_is_the_oracles():
    name, V, B, Cn = COST
    pr = C.problem(name, V, B, Cn)
    costs = []
    for k in (1, 2, 5, 10):
        p, c, acc = vfit(V, pr, ALL, k, C.near_start(V, B, Cn))
        assert bool((acc <= k).all()) and bool((acc >= 0).all())
        costs.append(c.double())
        with torch.no_grad():
            want = VO.cost(host_model(V), p.double(), pr)
        held(f"cost after {k} iterations {c.numpy()}", c.double(), want, E32[("cost", k)])
    for a, b in zip(costs, costs[1:]):
        assert bool((b <= a).all())
    assert bool((costs[-1] < costs[0]).all())


def gate(tag, name, p):
    """joint RMS and pixel RMS of p, per sample, within 4 x what the fp32 oracle reaches on the same case -> both, and the gates"""
    g3, g2 = C.figures(p, name)
    _, o3, o2 = C.recovery(name, torch.float32)
    for b in range(p.shape[0]):
        print(f"{tag} sample {b}: joints {1e3 * g3[b]:.6f} mm (fp32 oracle {1e3 * o3[b]:.6f}, gate {4e3 * o3[b]:.6f}), "
              f"pixels {g2[b]:.6f} (fp32 oracle {o2[b]:.6f}, gate {4 * o2[b]:.6f})")
    return g3, g2, 4 * o3, 4 * o2


def test_recovers_from_the_triangulated_start():
    """noise-free keypoints, C = 3, 20 iterations from init = 1"""
    pr = C.recovery_problem("quad")[0]
    p, cost, acc = vfit(C.RECOVERY["V"], pr, ALL, C.RECOVERY["iters"], lambda0=C.RECOVERY["lambda0"])
    assert bool((acc > 0).all()) and torch.isfinite(p).all()
    g3, g2, t3, t2 = gate("recovery", "quad", p)
    assert (g3 <= t3).all() and (g2 <= t2).all()


def test_one_view_of_outliers_is_voted_down():
    """view 1 replaced by outliers: with the robust loss the fit stays within the recovery gate, without it it does not"""
    V, P0 = C.RECOVERY["V"], C.recovery_near()
    p, _, acc = vfit(V, C.recovery_problem("gm_outliers")[0], ALL, C.RECOVERY["iters"], P0, C.RECOVERY["lambda0"])
    g3, g2, t3, t2 = gate("Geman-McClure", "gm_outliers", p)
    assert bool((acc > 0).all()) and (g3 <= t3).all() and (g2 <= t2).all()
    q, _, _ = vfit(V, C.recovery_problem("quad_outliers")[0], ALL, C.RECOVERY["iters"], P0, C.RECOVERY["lambda0"])
    q3, q2 = C.figures(q, "quad_outliers")
    print(f"quadratic: joints mm {1e3 * q3}, pixels {q2}")
    assert (q3 > t3).all() and (q2 > t2).all()


RULES = dict(V=37, B=4, Cn=3, iters=6)


def rules_problem():
    V, B, Cn = RULES["V"], RULES["B"], RULES["Cn"]
    return C.problem("gm", V, B, Cn)._replace(w2=torch.ones(B, Cn, 21)), C.near_start(V, B, Cn).float()


@functools.lru_cache(maxsize=None)
def alone(b, with_init):
    """sample b of rules_problem() fitted alone"""
    pr, P0 = rules_problem()
    one = pr._replace(T2=pr.T2[b:b + 1], w2=pr.w2[b:b + 1])
    return vfit(RULES["V"], one, ALL, RULES["iters"], P0[b:b + 1] if with_init else None)


def others_are_as_alone(r, skipped, with_init):
    for b in range(RULES["B"]):
        if b != skipped:
            for x, y in zip(r, alone(b, with_init)):
                assert x[b:b + 1].numpy().tobytes() == y.numpy().tobytes(), b


def not_fitted(r, b, start):
    assert float(r[1][b]) == float("inf") and int(r[2][b]) == 0 and r[0][b].numpy().tobytes() == start.numpy().tobytes()


def test_a_joint_behind_a_camera_at_the_start_is_not_fitted():
    pr, P0 = rules_problem()
    P0 = P0.clone()
    cam0 = pr.cams[0, 0]
    P0[1, 58:61] = -1.2 * (cam0[:9].reshape(3, 3).T @ cam0[9:12])      # the hand 0.1 m behind camera 0's centre
    with torch.no_grad():
        assert bool(VO.terms(host_model(RULES["V"]), P0.double(), pr)[2][1])
    r = vfit(RULES["V"], pr, ALL, RULES["iters"], P0)
    not_fitted(r, 1, P0[1])
    others_are_as_alone(r, 1, True)
    assert bool((r[2][[0, 2, 3]] > 0).all())


@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("what", ["nan_keypoint", "negative_weight", "inf_camera"])
def test_unusable_samples_are_not_fitted(what, with_init):
    pr, P0 = rules_problem()
    T2, w2, cams = pr.T2.clone(), pr.w2.clone(), pr.cams
    if what == "nan_keypoint":
        T2[1, 2, 7, 1] = float("nan")
    elif what == "negative_weight":
        w2[1, 0, 3] = -1.0
    else:      # a rig per sample, so that only sample 1 has the bad camera
        cams = cams.expand(RULES["B"], -1, -1).clone()
        cams[1, 1, 12] = float("inf")
    r = vfit(RULES["V"], pr._replace(T2=T2, w2=w2, cams=cams), ALL, RULES["iters"], P0 if with_init else None)
    not_fitted(r, 1, P0[1] if with_init else torch.zeros(62))
    others_are_as_alone(r, 1, with_init)
    assert torch.isfinite(r[0]).all()


def test_too_few_triangulated_joints_are_not_fitted():
    pr, _ = rules_problem()
    w2 = pr.w2.clone()
    w2[2, 1:] = 0.0      # sample 2 is seen by one view: nothing is triangulated
    w2[3, :, 2:] = 0.0   # sample 3 has two joints
    r = vfit(RULES["V"], pr._replace(w2=w2), ALL, RULES["iters"])
    not_fitted(r, 2, torch.zeros(62))
    not_fitted(r, 3, torch.zeros(62))
    assert bool((r[2][:2] > 0).all())


def test_frozen_unknowns_keep_their_bits():
    from scat_amd.fit import free_mask

    pr, P0 = rules_problem()
    p, cost, acc = vfit(RULES["V"], pr, free_mask(betas=False, log_scale=False), 8, P0)
    assert torch.equal(p[:, 48:58], P0[:, 48:58]) and torch.equal(p[:, 61], P0[:, 61])
    assert not torch.equal(p[:, 3:48], P0[:, 3:48]) and not torch.equal(p[:, 58:61], P0[:, 58:61]) and bool((acc > 0).all())
    p, _, acc = vfit(RULES["V"], pr, 0, 8, P0)
    assert torch.equal(p, P0)


def test_zero_weight_view_joints_do_not_count():
    pr, P0 = rules_problem()
    w2, far = pr.w2.clone(), pr.T2.clone()
    w2[:, 0, 4], w2[2, :, 9], w2[1, 2, 0] = 0.0, 0.0, 0.0
    far[:, 0, 4], far[2, :, 9], far[1, 2, 0] = 1e6, -1e6, 3e4
    for start in (P0, None):      # the closed-form start as well
        a = vfit(RULES["V"], pr._replace(w2=w2), ALL, RULES["iters"], start)
        b = vfit(RULES["V"], pr._replace(w2=w2, T2=far), ALL, RULES["iters"], start)
        for x, y in zip(a, b):
            assert x.numpy().tobytes() == y.numpy().tobytes()
        assert bool((a[2] > 0).all())


def test_same_call_same_bits():
    V, B, Cn = 778, 3, 8
    pr = C.problem("gm_limits", V, B, Cn, True)
    a, b = vfit(V, pr, ALL, 12), vfit(V, pr, ALL, 12)
    for x, y in zip(a, b):
        assert x.numpy().tobytes() == y.numpy().tobytes()
    assert bool((a[2] > 0).all())


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_inside_guard_bands(fill):
    """every pointer operand of both entry points between poisoned bands at pointer skews 0, 1 and 3 floats, with and without
    the optional pointers, a rig per sample and one for the batch: bands intact, every output word written, results bit for
    bit those of the plain run outside the arena"""
    from scat_amd._lib import lib
    from scat_amd.fit import FIT_VIEWS_HEADER, triangulate_views

    L, V, B, Cn = lib(), 37, 3, 3
    ns = L.bind(FIT_VIEWS_HEADER)
    m = model(V)
    w2 = torch.ones(B, Cn, 21)
    w2[0, 1:, 5], w2[1, 0, 2] = 0.0, 0.5
    full = C.problem("gm_limits", V, B, Cn, True)._replace(w2=w2)
    bare = C.problem("quad", V, B, Cn, False)
    P0 = C.near_start(V, B, Cn).float()
    stream = torch.cuda.current_stream().cuda_stream
    plain = []
    for pr in (full, bare):
        plain += [t.cpu() for t in triangulate_views(d_(pr.cams), d_(pr.T2), d_(pr.w2), pr.z_near)]
        for init in (1, 0):
            plain += list(vfit(V, pr, ALL, 4, None if init else P0, lambda0=1e-3))
    arena = Arena(DEV, fill, nbytes=16 << 20)
    for skew in (0, 1, 3):
        arena.reset()
        mp = [arena.place(t.cpu(), skew, name=n).data_ptr() for n, t in (("blend", m.blend), ("joint_t", m.joint_t), ("joint_s", m.joint_s),
                                                                         ("weights_t", m.weights_t), ("hands_mean", m.hands_mean_d))]
        jm = arena.place(torch.tensor(JOINT_MAP, dtype=torch.int32), skew, name="joint_map")
        outs = []
        for pr in (full, bare):
            ptr = lambda t, n: 0 if t is None else arena.place(t.float(), skew, name=n).data_ptr()
            cams, T2, wp = ptr(pr.cams, "cams"), ptr(pr.T2, "targets2"), ptr(pr.w2, "weights2")
            lo, hi = ptr(pr.lo, "pose_lo"), ptr(pr.hi, "pose_hi")
            pts = arena.place((B, 21, 3), skew, name="points", out=True)
            valid = arena.place((B, 21), skew, dtype=torch.int32, name="valid", out=True)
            ns.scat_triangulate(cams, pr.cams.shape[0], T2, wp, pts.data_ptr(), valid.data_ptr(), B, Cn, pr.z_near, stream)
            assert L.scat_last_kernel() == b"triangulate_c3"
            outs += [pts, valid]
            for init in (1, 0):
                p = arena.place((B, 62), skew, name="p", out=True) if init else arena.place(P0, skew, name="p0", out=True)
                cost = arena.place((B,), skew, name="cost", out=True)
                acc = arena.place((B,), skew, dtype=torch.int32, name="accepted", out=True)
                ns.scat_mano_fit_views(*mp, cams, pr.cams.shape[0], T2, wp, jm.data_ptr(), lo, hi, p.data_ptr(), cost.data_ptr(),
                                       acc.data_ptr(), B, Cn, V, m.parents_packed, *m.tips, 4, init, 1e-3, pr.w_pose, pr.w_beta,
                                       pr.w_limit, pr.sigma2, pr.z_near, ALL, stream)
                assert L.scat_last_kernel() == b"mano_fit_views_v37_c3_i4"
                outs += [p, cost, acc]
        torch.cuda.synchronize()
        arena.check()
        for got, want in zip(outs, plain):
            assert got.cpu().numpy().tobytes() == want.numpy().tobytes(), skew
        assert all(bool(((o == 0) | (o == 1)).all()) for o in outs if o.dtype == torch.int32 and o.dim() == 2)      # every word of valid


def test_fit_keypoints_views_to_projection_to_renderer():
    """the public API: fit_keypoints_views -> FitResult that mesh(), joints() and another fit's init take, project_views lands
    on the keypoints, triangulate gives the joints, and weak_perspective lets the renderer overlay the mesh in one view"""
    from scat_amd._lib import ScatError
    from scat_amd.fit import Cameras, FitResult, ManoFitter
    from scat_amd.render import MeshRenderer

    V, B, Cn = 778, 3, 3
    m = model(V)
    _, X3, T2, cams = C.truth(V, B, Cn, pose_sd=0.5)
    cams = cams.to(DEV)
    cameras = Cameras(cams[:, :, :9].reshape(1, Cn, 3, 3), cams[:, :, 9:12], cams[:, :, 12:16])
    assert torch.equal(cameras.packed(), cams)
    f = ManoFitter(m, joint_map=JOINT_MAP, iters=20, w_pose=1e-2, w_beta=1e-2)
    kp = T2.to(DEV)
    r = f.fit_keypoints_views(kp, cameras, sigma2=10.0)
    assert isinstance(r, FitResult) and r.p.shape == (B, 62) and bool((r.accepted > 0).all()) and bool(torch.isfinite(r.cost).all())
    uv = f.project_views(r, cameras)
    px = ((uv - kp) ** 2).sum(3).flatten(1).mean(1).sqrt()
    mm = 1e3 * ((f.joints(r).cpu().double() - X3) ** 2).sum(2).mean(1).sqrt()
    print(f"after 20 iterations: pixel RMS {px.cpu().numpy()}, joint RMS mm {mm.numpy()}")
    assert uv.shape == (B, Cn, 21, 2) and bool((px < 0.5).all()) and bool((mm < 0.5).all())
    want = VO.reproject(host_model(V), r.p.cpu().double(), VO.Problem(JOINT_MAP, cams.cpu(), T2))
    assert float((uv.cpu().double() - want).abs().max()) < 2e-3      # pixels of a 640 frame in fp32
    pts, valid = f.triangulate(kp, cameras)
    assert valid.dtype == torch.bool and bool(valid.all()) and float((pts.cpu().double() - X3).abs().max()) < 1e-5
    again = f.fit_keypoints_views(kp, cameras, init=r, iters=2)      # a result is a start, for this fit and for the others
    assert bool(torch.isfinite(again.p).all()) and bool((f.fit(pts, init=r, iters=1).accepted >= 0).all())
    one = Cameras(cameras.R[:, :1], cameras.t[:, :1], cameras.K[:, :1])
    single = f.fit_keypoints_views(kp[:, :1].contiguous(), one, init=r, iters=2)
    assert bool(torch.isfinite(single.cost).all())
    verts = f.mesh(r)
    assert verts.shape == (B, V, 3)
    R, t, cam = cameras.weak_perspective(0, 0.5, (640, 640))
    faces = np.load(os.path.join(ROOT, "tests", "golden", "hand_mesh.npz"))["f"]
    out = MeshRenderer(faces, V, size=(640, 640), device=DEV).render((verts @ R[0].T + t[0]).contiguous(), cam.expand(B, 3).contiguous())
    assert out["rgb"].shape == (B, 640, 640, 3) and bool(out["mask"].any())
    for bad, pat in ((dict(joints2d=kp.double()), "fp32"), (dict(joints2d=kp[:, :2].contiguous()), "joints2d"),
                     (dict(w2=torch.ones(B, Cn, 20, device=DEV)), "weights"), (dict(limits=(torch.zeros(44), torch.zeros(45))), "limits"),
                     (dict(init=torch.zeros(B, 65, device=DEV)), "start"), (dict(iters=65), "iterations"), (dict(z_near=0.0), "z_near"),
                     (dict(sigma2=-1.0), "sigma2"), (dict(joints2d=kp[:, :1].contiguous(), cameras=one), "one view needs a start"),
                     (dict(cameras=Cameras(cameras.R.expand(2, -1, -1, -1), cameras.t.expand(2, -1, -1), cameras.K.expand(2, -1, -1))),
                      "2 rigs for a batch of 3")):
        with pytest.raises(ScatError, match=pat):
            f.fit_keypoints_views(**dict(dict(joints2d=kp, cameras=cameras), **bad))
