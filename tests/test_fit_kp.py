"""The MANO fit to keypoints, the parts that need no GPU: the public header and its binding, every argument refusal of the
entry point, ManoFitter.fit_keypoints' refusal of CPU tensors, the fp64 oracle of tests/_fit_kp_oracle.py against itself
and against _fit_oracle, and the conditions (a), (b), (c) on the fixed inputs that the GPU tests gate
(tests/test_gpu_fit_kp.py), which shows those inputs fit for the gates."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_kp_cases as C  # noqa: E402
import _fit_kp_oracle as KO  # noqa: E402
import _fit_oracle as FO  # noqa: E402
from _fit_cases import JOINT_MAP, host_model, step_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP_H = os.path.join(ROOT, "include", "scat_mano_fit_kp.h")
PARENTS = sum(p << (4 * i) for i, p in enumerate((0, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)))
ENTRY = "scat_mano_fit_kp"


@pytest.fixture(scope="module")
def built():
    from scat_amd import build

    return build.build(verbose=False)


def test_keypoint_fit_header_is_bound(built):
    from scat_amd import build, fit
    from scat_amd._lib import EVAL_HEADER, FIT_HEADER, FIT_KP_HEADER, HEADER, HEADERS, lib, parse_header

    assert os.path.samefile(FIT_KP_HEADER, KP_H)
    assert HEADERS[0] == HEADER and HEADERS.index(FIT_KP_HEADER) == HEADERS.index(EVAL_HEADER) + 1 == HEADERS.index(FIT_HEADER) - 1
    protos = parse_header(KP_H)
    assert set(protos) == {ENTRY}
    L = lib()
    rt, args = protos[ENTRY]
    assert hasattr(L.cdll, ENTRY) and callable(getattr(L, ENTRY)) and rt is ctypes.c_int
    names = [an for _, an in args]
    assert names[-1] == "stream" and "ws" not in names and "ws_bytes" not in names
    by = dict((an, ty) for ty, an in args)
    assert by["parents"] is ctypes.c_uint64 and by["free_mask"] is ctypes.c_uint64 and by["free_cam"] is ctypes.c_int
    assert [ty for ty, an in args if an.startswith("tip")] == [ctypes.c_int] * 5
    for n in ("lambda0", "w_pose", "w_beta", "w_limit", "sigma3", "sigma2", "half_w", "half_h"):
        assert by[n] is ctypes.c_float, n
    assert names[:15] == ["blend", "joint_t", "joint_s", "weights_t", "hands_mean", "targets3", "weights3", "targets2", "weights2",
                          "joint_map", "pose_lo", "pose_hi", "p", "cost", "accepted"]
    assert L.by_header[FIT_KP_HEADER] == protos and list(L.by_header) == list(HEADERS) and not set(protos) & set(L.protos)
    for h in HEADERS:
        if not os.path.samefile(h, KP_H):
            assert not set(protos) & set(parse_header(h)), h
    src = open(KP_H).read()
    assert f"#define SCAT_FIT_KP_UNKNOWNS {fit.KP_UNKNOWNS}\n" in src and "CLAMPED" in src
    assert "UNITS" in src and "1e-6" in src      # how the caller balances metres against pixels is stated
    assert "1e-6" in fit.ManoFitter.fit_keypoints.__doc__ and "UNITS" in fit.ManoFitter.fit_keypoints.__doc__
    assert build._public_headers_mtime() >= os.path.getmtime(KP_H)      # the header is a rebuild trigger
    assert "scat_mano_fit_kp.h" in open(build.__file__).read()


GOOD = dict(B=4, V=778, parents=PARENTS, tips=[320, 443, 671, 554, 744], iters=20, init=1, lambda0=1e-3, w_pose=1e-6, w_beta=1e-6,
            w_limit=1e-2, sigma3=0.01, sigma2=10.0, half_w=112.0, half_h=112.0, free=(1 << 62) - 1, free_cam=7)
NPTR = 15
OPTIONAL = {5: "targets3", 6: "weights3", 7: "targets2", 8: "weights2", 10: "pose_lo", 11: "pose_hi"}


def _call(L, **kw):
    a = dict(GOOD, ptrs=[8 * (i + 1) for i in range(NPTR)])
    a.update(kw)
    return L.scat_mano_fit_kp(*a["ptrs"], a["B"], a["V"], a["parents"], *a["tips"], a["iters"], a["init"], a["lambda0"], a["w_pose"],
                              a["w_beta"], a["w_limit"], a["sigma3"], a["sigma2"], a["half_w"], a["half_h"], a["free"], a["free_cam"], 0)


def test_keypoint_fit_errors_surface_without_a_gpu(built):
    """argument validation happens before any HIP call: made-up pointers are never followed, each refusal carries its
    SCAT_E_* code and names the entry point, and the kernel label does not move"""
    from scat_amd import mano
    from scat_amd._lib import ScatError, lib

    L = lib()
    label = L.scat_last_kernel()

    def refused(code, pattern, **kw):
        with pytest.raises(ScatError, match=rf"{ENTRY} failed \({code}\): {ENTRY}: .*{pattern}"):
            _call(L, **kw)
        assert L.scat_last_kernel() == label

    base = [8 * (i + 1) for i in range(NPTR)]
    without = lambda *idx: [0 if i in idx else v for i, v in enumerate(base)]
    for i in range(NPTR):
        if i not in OPTIONAL:
            refused(-2, "null pointer", ptrs=without(i))
    for i in range(NPTR):
        refused(-2, "4-byte aligned", ptrs=base[:i] + [base[i] + 2] + base[i + 1:])
    refused(-2, "no targets", ptrs=without(5, 6, 7, 8))
    refused(-2, "weights3 given without targets3", ptrs=without(5))
    refused(-2, "weights2 given without targets2", ptrs=without(7))
    refused(-2, "pose_lo and pose_hi must both", ptrs=without(10))
    refused(-2, "pose_lo and pose_hi must both", ptrs=without(11))
    refused(-1, "batch 0 must be positive", B=0)
    refused(-1, "0 vertices outside", V=0)
    refused(-1, rf"{mano.MAX_V + 1} vertices outside 1\.\.{mano.MAX_V}", V=mano.MAX_V + 1)
    refused(-1, "tip 2 = 778", tips=[320, 443, 778, 554, 744])
    refused(-2, r"parent\[3\] = 7", parents=(PARENTS & ~(15 << 12)) | (7 << 12))
    refused(-2, r"0 iterations outside 1\.\.64", iters=0)
    refused(-2, r"65 iterations outside 1\.\.64", iters=65)
    refused(-2, "init 2 must be 0", init=2)
    refused(-2, "init -1 must be 0", init=-1)
    refused(-2, "lambda0 0 outside", lambda0=0.0)
    refused(-2, "lambda0 -1 outside", lambda0=-1.0)
    refused(-2, "lambda0 nan outside", lambda0=float("nan"))
    refused(-2, "lambda0 inf outside", lambda0=float("inf"))
    for name in ("w_pose", "w_beta", "w_limit", "sigma3", "sigma2"):
        refused(-2, f"{name} -1 must be finite and not negative", **{name: -1.0})
        refused(-2, f"{name} inf must be finite", **{name: float("inf")})
        refused(-2, f"{name} nan must be finite", **{name: float("nan")})
    for name in ("half_w", "half_h"):
        refused(-2, f"{name} 0 must be positive", **{name: 0.0})
        refused(-2, f"{name} -112 must be positive", **{name: -112.0})
        refused(-2, f"{name} nan must be positive", **{name: float("nan")})
        refused(-2, f"{name} inf must be positive and finite", **{name: float("inf")})
    refused(-2, "free_mask has bits above 61 set", free=1 << 62)
    refused(-2, "free_mask has bits above 61 set", free=1 << 63)
    refused(-2, r"free_cam 8 outside 0\.\.7", free_cam=8)
    refused(-2, r"free_cam -1 outside 0\.\.7", free_cam=-1)


def test_fit_keypoints_has_no_cpu_fallback():
    from scat_amd._lib import ScatError
    from scat_amd.fit import KP_UNKNOWNS, KeypointFitResult, ManoFitter
    from scat_amd.mano import ManoModel

    f = ManoFitter(ManoModel.synthetic(1, V=37), joint_map=JOINT_MAP)
    with pytest.raises(ScatError, match="no CPU fallback"):
        f.fit_keypoints(joints2d=torch.zeros(2, 21, 2))
    with pytest.raises(ScatError, match="no CPU fallback"):
        f.fit_keypoints(torch.zeros(2, 21, 3), torch.zeros(2, 21, 2))
    with pytest.raises(ScatError, match="joints3d, joints2d or both"):
        f.fit_keypoints()
    p = torch.zeros(2, 65)
    r = KeypointFitResult(p[:, 0:3], p[:, 3:48], p[:, 48:58], p[:, 58:61], torch.exp(p[:, 61]), p[:, 62:65], None, None, p)
    with pytest.raises(ScatError, match="no CPU fallback"):
        f.project(r)
    assert KP_UNKNOWNS == 65 and KeypointFitResult._fields == ("rots", "poses", "betas", "trans", "scale", "cam", "cost", "accepted", "p")


def test_oracle_gradient_is_twice_g_with_robust_loss_and_active_limits():
    """the IRLS weight is rho', so g of the normal equations is half the gradient of the robust cost, limits included"""
    V = 37
    m = host_model(V)
    pr, _, _ = C.problem("gm_limits", V)
    P1 = C.near_start(V)
    ex = KO.excess(P1, pr)
    assert int((ex > 0).sum()) > 10 and int((ex < 0).sum()) > 10      # limits active on both sides
    _, g = KO.normal_equations(m, P1, pr)
    Pq = P1.clone().requires_grad_(True)
    KO.cost(m, Pq, pr).sum().backward()
    e = KO.rel(g.numpy(), 0.5 * Pq.grad.numpy())
    print(f"g against half the autograd gradient: {e:.3e}")
    assert e < 1e-12
    r3, _ = KO.residuals(m, P1, pr)
    w = KO.rho_prime((r3 * r3).sum(2), pr.sigma3)
    assert float(w.min()) < 0.1 and float(w.max()) > 0.5      # the outliers are down-weighted, the inliers are not
    # a limit entry that is not finite is no limit
    lo = pr.lo.clone()
    lo[::2] = float("nan")
    ex2 = KO.excess(P1, pr._replace(lo=lo, hi=torch.full((45,), float("inf"))))
    assert bool((ex2[:, ::2] == 0).all()) and bool((ex2 <= 0).all()) and bool((ex2[:, 1::2] == ex.clamp_max(0)[:, 1::2]).all())


@pytest.mark.parametrize("V", [37])
def test_oracle_reproduces_the_quadratic_oracle(V):
    """no 2-D term, sigma = 0, no limits, frozen camera: _fit_oracle.lm's p, cost and accepted"""
    m = host_model(V)
    T, P1, Ps, c = step_case(V)
    ones = torch.ones(6, 21, dtype=torch.float64)
    pr = KO.Problem(JOINT_MAP, T3=T, half=C.HALF)
    cam = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64).repeat(6, 1)
    for iters, lam in ((1, 1e-2), (6, 1e-3)):
        want = FO.lm(m, T.double(), ones, JOINT_MAP, P1, iters, lambda0=lam)
        got = KO.lm(m, pr, torch.cat([P1, cam], 1), iters, lam, free_cam=0)
        assert torch.equal(got[0][:, 62:], cam) and got[2].tolist() == want[2].tolist()
        assert FO.rel(got[0][:, :62].numpy(), want[0].numpy()) < 1e-9 and FO.rel(got[1].numpy(), want[1].numpy()) < 1e-9
    P0 = KO.start(m, pr, 6)
    assert FO.rel(P0[:, :62].numpy(), FO.procrustes_start(m, T, ones, JOINT_MAP).numpy()) < 1e-12 and torch.equal(P0[:, 62:], cam)


def test_oracle_two_d_start_mirrored_and_rotated():
    """a mirrored hand makes the 2-D start choose the second candidate; an in-plane rotation beyond pi / 2 is recovered by
    phi; both reproduce the keypoints exactly, since the hands are at the zero pose"""
    V = 37
    m = host_model(V)
    P, T2 = C.mirrored_targets(V)
    pr = KO.Problem(JOINT_MAP, T2=T2, half=C.HALF)
    info = []
    P0 = KO.start(m, pr, 4, info=info)
    assert info == [0, 0, 1, 1]
    assert float(P0[1, :3].norm()) > np.pi / 2 and abs(float(P0[1, 2]) - 2.5) < 1e-6
    assert float((P0 - P).abs().max()) < 1e-5 and bool((P0[:, 58:62] == 0).all())
    assert float(KO.rms2(m, P0, T2, JOINT_MAP, C.HALF).max()) < 1e-3
    # with a 3-D term the start is the Procrustes one, and its camera reproduces the keypoints of the true hands
    pr, _, _ = C.problem("both", V)
    info = []
    P0 = KO.start(m, pr, 6, info=info)
    assert info == ["3d"] * 6
    s2 = KO.rms2(m, P0, pr.T2, JOINT_MAP, C.HALF)
    far = KO.rms2(m, torch.cat([P0[:, :62], torch.tensor([1.0, 0, 0], dtype=torch.float64).repeat(6, 1)], 1), pr.T2, JOINT_MAP, C.HALF)
    assert bool((s2 < 0.5 * far).all())


def test_conditions_on_the_fixed_inputs():
    """(a), (b), (c) on the fp64 oracle, so that no GPU failure can be blamed on the data, and every one-step case of the
    GPU tests accepts its step"""
    V = 37
    a3 = C.recovery_figures("gm", V, C.run("gm", V, 20)[0])[0]
    q3 = C.recovery_figures("quad_outliers", V, C.run("quad_outliers", V, 20)[0])[0]
    print(f"(a) inlier RMS, mm: Geman-McClure {1e3 * a3}, quadratic {1e3 * q3}")
    assert (a3 < 0.25 * q3).all()
    viol = {n: (C.run(n, V, 20)[0][:, 3:48].abs() - C.BOX).clamp_min(0).max(1).values.numpy() for n in ("limits", "both")}
    print(f"(b) largest violation, rad: with limits {viol['limits']}, without {viol['both']}")
    assert (viol["limits"] < viol["both"]).all()
    _, start, end = C.condition_c(V)
    print(f"(c) reprojection RMS, px: start {start}, after 40 iterations {end}")
    assert (end <= 0.5 * start).all()
    for name in ("both", "2d", "gm", "limits_wide"):
        assert C.run(name, V, 1)[2].tolist() == [1] * 6, name
    ex = KO.excess(C.near_start(V), C.problem("limits_wide", V)[0])
    assert bool(((ex != 0).sum(1) >= 1).all())      # every hand of the one-step limits case has an active limit
