"""The MANO fit to a track of keypoints in calibrated views, the parts that need no GPU: the public header in include_ext/
and its binding, the build's second tuple, every argument refusal of the entry point, the workspace query, the Python
refusals, the fp64 oracle of tests/_fit_seq_views_oracle.py against the frame's and the track's oracles, and that the fixed
inputs of the GPU tests (tests/test_gpu_fit_seq_views.py) are fit for their gates."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_seq_views_cases as C  # noqa: E402
import _fit_seq_views_oracle as QO  # noqa: E402
import _fit_views_cases as VC  # noqa: E402
import _fit_views_oracle as VO  # noqa: E402
import _lm_oracle as L  # noqa: E402
from _fit_cases import JOINT_MAP, host_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ_VIEWS_H = os.path.join(ROOT, "include_ext", "scat_mano_fit_seq_views.h")
PARENTS = sum(p << (4 * i) for i, p in enumerate((0, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)))
FIT, WS = "scat_mano_fit_seq_views", "scat_mano_fit_seq_views_ws"
S_NAMES = ("s_rots", "s_poses", "s_betas", "s_trans", "s_scale")


@pytest.fixture(scope="module")
def built():
    from scat_amd import build

    return build.build(verbose=False)


def test_header_declares_the_two_and_collides_with_no_other(built):
    from scat_amd import build, fit
    from scat_amd._lib import EXTENSION_HEADERS, HEADERS, lib, parse_header

    assert os.path.samefile(fit.FIT_SEQ_VIEWS_HEADER, SEQ_VIEWS_H)
    protos = parse_header(SEQ_VIEWS_H)
    assert set(protos) == {FIT, WS}
    others = list(HEADERS) + list(EXTENSION_HEADERS) + [os.path.join(ROOT, "include", h) for h in sorted(os.listdir(os.path.join(ROOT, "include")))]
    others += [os.path.join(ROOT, "include_ext", h) for h in sorted(os.listdir(os.path.join(ROOT, "include_ext"))) if h != os.path.basename(SEQ_VIEWS_H)]
    for h in others:
        assert not set(protos) & set(parse_header(h)), h
    names = [an for _, an in protos[FIT][1]]
    by = dict((an, ty) for ty, an in protos[FIT][1])
    assert names[:17] == ["blend", "joint_t", "joint_s", "weights_t", "hands_mean", "cams", "cam_batch", "targets2", "weights2", "joint_map",
                          "pose_lo", "pose_hi", "p", "cost", "accepted", "ws", "ws_bytes"]
    assert names[17:21] == ["S", "T", "C", "V"] and names[-1] == "stream" and names[-2] == "free_mask"
    assert names[names.index("z_near") + 1:-2] == list(S_NAMES)
    assert by["parents"] is ctypes.c_uint64 and by["free_mask"] is ctypes.c_uint64 and by["ws_bytes"] is ctypes.c_int64
    for n in ("lambda0", "w_pose", "w_beta", "w_limit", "sigma2", "z_near") + S_NAMES:
        assert by[n] is ctypes.c_float, n
    assert protos[FIT][0] is ctypes.c_int and protos[WS][0] is ctypes.c_int64 and [an for _, an in protos[WS][1]] == ["S", "T"]
    src = open(SEQ_VIEWS_H).read()
    assert "CLAMPED" in src and "UNITS" in src and "BEHIND THE CAMERA" in src and "w_pose = 1e2" in src
    assert '#include "scat_mano_fit_views.h"' in src and "scat_mano_fit_seq.h" in src
    doc = fit.ManoFitter.fit_keypoints_views_sequence.__doc__
    assert "UNITS" in doc and "BEHIND THE CAMERA" in doc and "ot fitted" in doc
    # the build: the first tuple as it was, the new header in a second one that build() checks the same way
    assert build.EXT_HEADERS == ("scat_mano_fit_views.h",) and build.EXT_HEADERS_MORE == ("scat_mano_fit_seq_views.h",)
    assert build._deps_mtime() >= build._ext_headers_mtime() >= os.path.getmtime(SEQ_VIEWS_H)
    assert not os.path.exists(os.path.join(ROOT, "include", "scat_mano_fit_seq_views.h"))
    L_ = lib()
    ns = L_.bind(SEQ_VIEWS_H)
    assert sorted(vars(ns)) == [FIT, WS] and L_.bind(SEQ_VIEWS_H) is ns and hasattr(L_.cdll, FIT) and hasattr(L_.cdll, WS)
    assert "scat_mano_fit_seq_views.h" in sys.modules["scat_amd._lib"].__doc__


def test_build_refuses_without_the_header(built, monkeypatch):
    from scat_amd import build

    monkeypatch.setattr(build, "EXT_HEADERS_MORE", ("scat_mano_fit_seq_views.h", "scat_no_such_header.h"))
    with pytest.raises(RuntimeError, match="scat_no_such_header.h"):
        build.build(verbose=False)


def test_workspace_query_is_the_tracks(built):
    from scat_amd._lib import lib

    L_ = lib()
    ns = L_.bind(SEQ_VIEWS_H)
    for S, T in ((1, 1), (3, 5), (65, 2), (1024, 16), (2, 256)):
        assert ns.scat_mano_fit_seq_views_ws(S, T) == L_.scat_mano_fit_seq_ws(S, T) == S * T * 7874 * 4
    for S, T in ((0, 4), (4, 0), (4, 257), (-1, 4)):
        assert ns.scat_mano_fit_seq_views_ws(S, T) == 0


GOOD = dict(cam_batch=1, S=4, T=5, C=3, V=778, parents=PARENTS, tips=[320, 443, 671, 554, 744], iters=20, init=1, lambda0=1e-3, w_pose=1e-2,
            w_beta=1e-2, w_limit=1e2, sigma2=10.0, z_near=1e-3, smooth=[1.0, 2.0, 3.0, 4.0, 5.0], free=(1 << 62) - 1, ws=4096, ws_bytes=None)
NPTR = 14      # blend .. hands_mean, cams, targets2, weights2, joint_map, pose_lo, pose_hi, p, cost, accepted
OPTIONAL = {7: "weights2", 9: "pose_lo", 10: "pose_hi"}


def _fit(ns, **kw):
    a = dict(GOOD, ptrs=[8 * (i + 1) for i in range(NPTR)])
    a.update(kw)
    p = a["ptrs"]
    nbytes = ns.scat_mano_fit_seq_views_ws(a["S"], a["T"]) if a["ws_bytes"] is None else a["ws_bytes"]
    return ns.scat_mano_fit_seq_views(*p[:6], a["cam_batch"], *p[6:], a["ws"], nbytes, a["S"], a["T"], a["C"], a["V"], a["parents"],
                                      *a["tips"], a["iters"], a["init"], a["lambda0"], a["w_pose"], a["w_beta"], a["w_limit"], a["sigma2"],
                                      a["z_near"], *a["smooth"], a["free"], 0)


def test_errors_surface_without_a_gpu(built):
    """argument validation happens before any HIP call: made-up pointers are never followed, each refusal carries its
    SCAT_E_* code and names the entry point and the argument, and the kernel label does not move"""
    from scat_amd import mano
    from scat_amd._lib import ScatError, lib

    L_ = lib()
    ns = L_.bind(SEQ_VIEWS_H)
    label = L_.scat_last_kernel()

    def refused(code, pattern, **kw):
        with pytest.raises(ScatError, match=rf"{FIT} failed \({code}\): {FIT}: .*{pattern}"):
            _fit(ns, **kw)
        assert L_.scat_last_kernel() == label

    base = [8 * (i + 1) for i in range(NPTR)]
    without = lambda *idx: [0 if i in idx else v for i, v in enumerate(base)]
    for i in range(NPTR):
        if i not in OPTIONAL:
            refused(-2, "null pointer", ptrs=without(i))
        refused(-2, "4-byte aligned", ptrs=base[:i] + [base[i] + 2] + base[i + 1:])
    refused(-2, "pose_lo and pose_hi must both", ptrs=without(9))
    refused(-2, "pose_lo and pose_hi must both", ptrs=without(10))
    refused(-1, "batch 0 must be positive", S=0)
    refused(-1, "0 vertices outside", V=0)
    refused(-1, rf"{mano.MAX_V + 1} vertices outside 1\.\.{mano.MAX_V}", V=mano.MAX_V + 1)
    refused(-1, "tip 2 = 778", tips=[320, 443, 778, 554, 744])
    refused(-2, r"parent\[3\] = 7", parents=(PARENTS & ~(15 << 12)) | (7 << 12))
    refused(-1, r"0 views outside 1\.\.8", C=0)
    refused(-1, r"9 views outside 1\.\.8", C=9)
    refused(-1, "cam_batch 2 must be 1", cam_batch=2)
    refused(-1, "cam_batch 0 must be 1", cam_batch=0)
    _fit_ok_cam_batch = dict(cam_batch=4)      # one rig per sequence is legal: the next refusal in line is the workspace's
    refused(-3, "workspace must be a 16-byte-aligned pointer", ws=0, **_fit_ok_cam_batch)
    for z in ("0", "-1", "nan", "inf"):
        refused(-2, f"z_near {z} must be positive and finite", z_near=float(z))
    refused(-1, r"0 frames outside 1\.\.256", T=0)
    refused(-1, r"257 frames outside 1\.\.256", T=257)
    refused(-2, r"0 iterations outside 1\.\.64", iters=0)
    refused(-2, r"65 iterations outside 1\.\.64", iters=65)
    refused(-2, "init 2 must be 0", init=2)
    refused(-2, "init -1 must be 0", init=-1)
    refused(-2, "init 1 needs C >= 2 views", C=1)
    for lam in ("0", "-1", "nan", "inf"):
        refused(-2, f"lambda0 {lam} outside", lambda0=float(lam))
    for name in ("w_pose", "w_beta", "w_limit", "sigma2"):
        refused(-2, f"{name} -1 must be finite and not negative", **{name: -1.0})
        refused(-2, f"{name} inf must be finite", **{name: float("inf")})
        refused(-2, f"{name} nan must be finite", **{name: float("nan")})
    for i, name in enumerate(S_NAMES):
        for v in ("-1", "inf", "nan"):
            sm = list(GOOD["smooth"])
            sm[i] = float(v)
            refused(-2, f"{name} {v} must be finite and not negative", smooth=sm)
    refused(-2, "free_mask has bits above 61 set", free=1 << 62)
    refused(-2, "free_mask has bits above 61 set", free=1 << 63)
    refused(-1, "8388608 sequences of 256 frames: more than 2147483647 frames", S=1 << 23, T=256)
    need = ns.scat_mano_fit_seq_views_ws(GOOD["S"], GOOD["T"])
    refused(-3, "workspace must be a 16-byte-aligned pointer", ws=0)
    refused(-3, "workspace must be a 16-byte-aligned pointer", ws=4096 + 4)
    refused(-3, f"workspace of {need - 1} bytes, {need} needed", ws_bytes=need - 1)
    # C = 1 with the caller's start passes every check up to the workspace's
    refused(-3, "workspace must be a 16-byte-aligned pointer", ws=0, C=1, init=0)


def _cameras(Cn, Sc=1):
    from scat_amd.fit import Cameras

    c = VC.rig(Cn, Sc)
    return Cameras(c[:, :, :9].reshape(Sc, Cn, 3, 3), c[:, :, 9:12], c[:, :, 12:16])


def test_python_refusals_and_no_cpu_fallback():
    from scat_amd._lib import ScatError
    from scat_amd.fit import ManoFitter, SequenceFitResult, _groups
    from scat_amd.mano import ManoModel

    f = ManoFitter(ManoModel.synthetic(1, V=37), joint_map=JOINT_MAP)
    cams = _cameras(3)
    kp = torch.zeros(2, 4, 3, 21, 2)
    for call in (lambda: f.fit_keypoints_views_sequence(kp, cams), lambda: f.triangulate(kp, cams)):
        with pytest.raises(ScatError, match="no CPU fallback"):
            call()
    p = torch.zeros(2, 4, 62)
    with pytest.raises(ScatError, match="no CPU fallback"):
        f.project_views(SequenceFitResult(*_groups(p), None, None, p), cams)
    with pytest.raises(ScatError, match="Cameras"):
        f.fit_keypoints_views_sequence(kp, VC.rig(3))
    with pytest.raises(ScatError, match="unknown smooth keys"):
        f.fit_keypoints_views_sequence(kp, cams, smooth=dict(cam_scale=1.0))
    with pytest.raises(ScatError, match=r"smooth\['rots'\]"):
        f.fit_keypoints_views_sequence(kp, cams, smooth=dict(rots=-1.0))


def test_frame_blocks_are_the_views_oracles_and_the_dense_system_is_their_chain():
    V, S, T, Cn = 37, 2, 3, 3
    m, pr, P1 = host_model(V), C.problem("gm_limits", V, S, T, Cn, True), C.near_start(V, S, T, Cn, True)
    A, g = QO.frame_equations(m, P1, pr)
    for s in range(S):
        for t in range(T):
            one = VO.Problem(JOINT_MAP, pr.cams[s:s + 1], pr.T2[s, t:t + 1], None, pr.lo, pr.hi, pr.w_pose, pr.w_beta, pr.w_limit, pr.sigma2)
            A1, g1 = VO.normal_equations(m, P1[s, t:t + 1], one)
            assert VO.rel(A[s, t].numpy(), A1[0].numpy()) < 1e-13 and VO.rel(g[s, t].numpy(), g1[0].numpy()) < 1e-13
    free = C.ALL & ~(1 << 5)
    A, g = QO.frame_equations(m, P1, pr, free)
    H, G = QO.equations(m, P1, pr, free)
    d = QO.dvec(pr.smooth, torch.float64) * L.mask_vec(free, 62, torch.float64)
    H2, G2 = L.chain(A, g, P1, d)
    assert torch.equal(H, H2) and torch.equal(G, G2) and H.shape == (S, 62 * T, 62 * T)
    assert bool((H[:, 62:124, 0:62] == torch.diag(-d)).all()) and float(d[5]) == 0.0 and bool((H[:, 5, 5] == 1).all())
    # g is half the gradient of the cost, smoothness included
    Pq = P1.clone().requires_grad_(True)
    QO.cost(m, Pq, pr).sum().backward()
    _, G = QO.equations(m, P1, pr)
    e = VO.rel(G.numpy(), 0.5 * Pq.grad.reshape(S, -1).numpy())
    print(f"g against half the autograd gradient: {e:.3e}")
    assert e < 1e-12


def test_one_frame_without_smoothness_is_the_views_oracle():
    V, S, Cn = 37, 3, 3
    m = host_model(V)
    pr = C.problem("gm_limits", V, S, 1, Cn)._replace(smooth=(0.0,) * 5)
    P1 = C.near_start(V, S, 1, Cn)
    a = QO.lm(m, pr, P1, 6, 1e-2)
    b = VO.lm(m, QO.frames(pr), P1[:, 0], 6, 1e-2)
    assert torch.equal(a[0][:, 0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and bool((a[2] > 0).all())
    # all five zero decouples longer tracks too: the cost is the sum of the frames'
    pr5 = C.problem("quad", V, S, 5, Cn)._replace(smooth=(0.0,) * 5)
    P5 = C.near_start(V, S, 5, Cn)
    with torch.no_grad():
        assert VO.rel(QO.cost(m, P5, pr5).numpy(), VO.cost(m, P5.flatten(0, 1), QO.frames(pr5)).reshape(S, 5).sum(1).numpy()) < 1e-15


def test_oracle_not_fitted_rules():
    V, S, T, Cn = 37, 3, 3, 3
    m, pr, P1 = host_model(V), C.problem("gm", V, S, T, Cn), C.near_start(V, S, T, Cn)
    bad = pr.T2.clone()
    bad[1, 2, 0, 4, 1] = float("nan")
    P, c, acc = QO.lm(m, pr._replace(T2=bad), P1, 3, 1e-2)
    assert torch.equal(P[1], P1[1]) and float(c[1]) == float("inf") and acc.tolist()[1] == 0 and acc.tolist()[0] > 0
    Pb = P1.clone()
    cam0 = pr.cams[0, 0].double()
    Pb[2, 1, 58:61] = -1.2 * (cam0[:9].reshape(3, 3).T @ cam0[9:12])
    P, c, acc = QO.lm(m, pr, Pb, 3, 1e-2)
    assert torch.equal(P[2], Pb[2]) and float(c[2]) == float("inf") and acc.tolist() == [acc.tolist()[0], acc.tolist()[1], 0] and acc.tolist()[0] > 0
    w2 = torch.ones(S, T, Cn, 21)
    w2[0, :, 1:] = 0.0      # sequence 0 is seen by one camera in every frame: no start anywhere
    P, has, fitted = QO.start(m, pr._replace(w2=w2))
    assert fitted.tolist() == [False, True, True] and bool((P[0] == 0).all()) and not bool(has[0].any())


def test_conditions_on_the_fixed_inputs():
    """what the GPU gates lean on, on the oracle: every one-step case accepts its step; the start case has scanned frames and
    an unwrapped rotation; in fp64 the oracle converges on every sequence of every recovery case; the single-view frame and
    the unseen frame are bridged; the track's acceleration error is below the frame-by-frame fit's on the noisy case"""
    import test_gpu_fit_seq_views as G

    for name, V, S, T, Cn, per in G.STEPS:
        if S <= 3:
            assert C.run(name, V, S, T, Cn, per, 1)[2].tolist() == [1] * S, (name, V, S, T, Cn)
    V, S, T, Cn, per = G.SCAN_START
    pr, P64, has, _ = C.start_case(V, S, T, Cn, per)
    assert has.tolist()[0][1] is False and has.tolist()[1][0] is False and int((~has).sum()) == 2
    raw = VO.start(host_model(V), QO.frames(pr))[0].reshape(S, T, 62)
    assert torch.equal(P64[0, 1, 58:62], P64[0, 0, 58:62]) and torch.equal(P64[1, 0, :3], P64[1, 1, :3]) and bool((raw[0, 1] == 0).all())
    jump = (P64[S - 1, :, :3] - raw[S - 1, :, :3]).norm(dim=1)
    print(f"unwrapped frames of the last sequence: the scan moved rots by {jump.numpy()} rad")
    assert bool((jump > 6.0).any()) and float((P64[S - 1, 1:, :3] - P64[S - 1, :-1, :3]).norm(dim=1).max()) < 1.0
    # 1 px of noise is 1 / 1200 m at the rig's fx / z (the header's UNITS): 0.83 mm per view-joint before any averaging;
    # the noise-free cases end at the bias of the smoothness on an accelerating truth, hundredths of a millimetre
    bound = dict(clean=(5e-5, 0.05), outliers=(2e-4, 0.2), noise=(2e-3, 2.0), single_view=(2e-3, 2.0), unseen=(2e-3, 2.0))
    for name in C.RECOVERY_CASES:
        _, j64, p64, gap64, hist = C.recovery(name)
        print(f"recovery {name}, fp64: joint RMS mm {1e3 * j64}, pixel RMS {p64}, frame {C.GAP_FRAME} joint RMS mm {1e3 * gap64}")
        assert (j64 < bound[name][0]).all() and (p64 < bound[name][1]).all(), name
        assert bool(((hist[0] - hist[1]) <= 1e-2 * hist[1]).all()), name      # the last iteration moves the cost by under a percent
        if name in ("single_view", "unseen"):
            assert (gap64 < 2.5e-3).all(), name      # bridged: the frame without a start of its own is as good as the others
    m = host_model(C.RECOVERY["V"])
    X3 = C.recovery_problem("noise")[1]
    a_track = QO.accel(m, C.recovery("noise")[0], JOINT_MAP, X3)
    a_frames = QO.accel(m, C.per_frame("noise"), JOINT_MAP, X3)
    print(f"acceleration error mm / frame^2, noisy case: track {1e3 * a_track.numpy()}, frame by frame {1e3 * a_frames.numpy()}")
    assert bool((a_track < a_frames).all())
