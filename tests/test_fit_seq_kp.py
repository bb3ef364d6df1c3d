"""The MANO fit to a track of keypoints, the parts that need no GPU: the public header and its binding by _Lib.bind, every
refusal of the entry point, the workspace query, ManoFitter.fit_keypoints_sequence's own refusals, the fp64 oracle of
tests/_fit_seq_kp_oracle.py against autograd and against the two oracles it composes, and the conditions on the fixed
inputs the GPU tests gate (tests/test_gpu_fit_seq_kp.py), so that no failure there can be blamed on the data."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_kp_oracle as KO  # noqa: E402
import _fit_seq_cases as SC  # noqa: E402
import _fit_seq_kp_cases as G  # noqa: E402
import _fit_seq_kp_oracle as QO  # noqa: E402
import _fit_seq_oracle as SO  # noqa: E402
from _fit_cases import JOINT_MAP, host_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ_KP_H = os.path.join(ROOT, "include", "scat_mano_fit_seq_kp.h")
PARENTS = sum(p << (4 * i) for i, p in enumerate((0, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)))
ENTRY = "scat_mano_fit_seq_kp"
S_NAMES = ("s_rots", "s_poses", "s_betas", "s_trans", "s_scale", "s_cs", "s_ct")


@pytest.fixture(scope="module")
def built():
    from scat_amd import build

    return build.build(verbose=False)


def test_header_parses_and_collides_with_no_other():
    from scat_amd import build, fit
    from scat_amd._lib import EXTENSION_HEADERS, HEADERS, parse_header

    assert os.path.samefile(fit.FIT_SEQ_KP_HEADER, SEQ_KP_H)
    assert "scat_mano_fit_seq_kp.h" in build.PUBLIC_HEADERS
    assert not any(os.path.samefile(h, SEQ_KP_H) for h in (*HEADERS, *EXTENSION_HEADERS))
    protos = parse_header(SEQ_KP_H)
    assert set(protos) == {"scat_mano_fit_seq_kp_ws", ENTRY}
    assert protos["scat_mano_fit_seq_kp_ws"][0] is ctypes.c_int64
    assert [ty for ty, _ in protos["scat_mano_fit_seq_kp_ws"][1]] == [ctypes.c_int, ctypes.c_int]
    rt, args = protos[ENTRY]
    by = dict((an, ty) for ty, an in args)
    assert rt is ctypes.c_int and args[-1][1] == "stream"
    assert by["ws"] is ctypes.c_void_p and by["ws_bytes"] is ctypes.c_int64 and by["free_mask"] is ctypes.c_uint64
    assert all(by[k] is ctypes.c_int for k in ("S", "T", "V", "iters", "init", "free_cam")) and by["parents"] is ctypes.c_uint64
    assert tuple(an for _, an in args if an.startswith("s_")) == S_NAMES
    assert all(by[k] is ctypes.c_float for k in S_NAMES + ("lambda0", "w_pose", "w_beta", "w_limit", "sigma3", "sigma2", "half_w",
                                                            "half_h"))
    # scat_mano_fit_kp's arguments, in its order, with the workspace, T and the smoothness let in
    kp = [an for _, an in parse_header(fit.FIT_KP_HEADER if hasattr(fit, "FIT_KP_HEADER") else
                                       os.path.join(ROOT, "include", "scat_mano_fit_kp.h"))["scat_mano_fit_kp"][1]]
    mine = [an for _, an in args if an not in ("ws", "ws_bytes", "T") + S_NAMES]
    assert mine == ["S" if an == "B" else an for an in kp]
    for h in (*HEADERS, *EXTENSION_HEADERS, fit.FIT_VERTS_HEADER, fit.FIT_POINTS_HEADER):
        assert not set(protos) & set(parse_header(h)), h
    src = " ".join(open(SEQ_KP_H).read().replace(" * ", " ").split())
    for said in ("UNITS", "axis-angle", "CONSTANT SHAPE", "no hard constraint", "NOT revisited", "before any HIP call",
                 "every pivot of every frame is positive", "every pivot of every frame is finite",
                 "every trial unknown of every frame is finite", "no floating-point atomic", "no data-dependent exit",
                 "depend neither on S nor on its index", "at the current iterate", "weights are all zero",
                 "p is written only after an accepted step", "a pure number squared for s_cs"):
        assert said in src, said
    doc = " ".join(fit.ManoFitter.fit_keypoints_sequence.__doc__.split())
    for said in ("UNITS", "axis-angle", "no hard constraint", "not revisited", "weights are all zero"):
        assert said in doc, said
    assert build._public_headers_mtime() >= os.path.getmtime(SEQ_KP_H)      # the header is a rebuild trigger


def test_bind_binds_the_header_and_leaves_the_tables(built):
    from scat_amd import _lib
    from scat_amd._lib import EXTENSION_HEADERS, FIT_SEQ_HEADER, HEADERS, lib, parse_header
    from scat_amd.fit import FIT_SEQ_KP_HEADER

    L = lib()
    before = (tuple(HEADERS), tuple(EXTENSION_HEADERS), dict(L.by_header), dict(L.by_extension), dict(L.protos))
    ns = L.bind(FIT_SEQ_KP_HEADER)
    assert sorted(vars(ns)) == sorted(parse_header(SEQ_KP_H))
    assert L.bind(FIT_SEQ_KP_HEADER) is ns and L.bound[FIT_SEQ_KP_HEADER] is ns
    assert (tuple(_lib.HEADERS), tuple(_lib.EXTENSION_HEADERS), L.by_header, L.by_extension, L.protos) == before
    assert len(HEADERS) == 7 and EXTENSION_HEADERS == (FIT_SEQ_HEADER,) and list(L.by_header) == list(HEADERS)
    for name in vars(ns):
        assert hasattr(L.cdll, name) and not hasattr(L, name)
    assert ns.scat_mano_fit_seq_kp.__name__ == ENTRY      # the checked wrapper


def test_workspace_query(built):
    from scat_amd._lib import lib
    from scat_amd.fit import FIT_SEQ_KP_HEADER

    q = lib().bind(FIT_SEQ_KP_HEADER).scat_mano_fit_seq_kp_ws
    sizes = [(1, 1), (1, 2), (2, 2), (2, 5), (3, 5), (3, 256), (1024, 16)]
    got = [int(q(S, T)) for S, T in sizes]
    assert got == sorted(got) and len(set(got)) == len(got)
    for (S, T), g in zip(sizes, got):      # L_t with y_t (66 x 65), M_t^T (65 x 65), two copies of the 65 unknowns
        assert g == 4 * S * T * (66 * 65 + 65 * 65 + 2 * 65)
    for S, T in ((0, 5), (-1, 5), (2, 0), (2, -1), (2, 257)):
        assert int(q(S, T)) == 0, (S, T)


def test_both_track_queries_share_one_layout(built):
    """scat_mano_fit_seq_ws and scat_mano_fit_seq_kp_ws are one piece of arithmetic at 62 and at 65 unknowns (L_t with
    y_t, M_t^T, two copies of the unknowns, fp32): 31,496 and 34,580 bytes per frame, 0 outside 1..256 frames"""
    from scat_amd._lib import lib
    from scat_amd.fit import FIT_SEQ_KP_HEADER

    L = lib()
    for q, per_frame in ((L.scat_mano_fit_seq_ws, 31496), (L.bind(FIT_SEQ_KP_HEADER).scat_mano_fit_seq_kp_ws, 34580)):
        for S, T in ((1, 1), (2, 5), (1, 256)):
            assert int(q(S, T)) == S * T * per_frame, (S, T)
        assert int(q(1, 0)) == 0 and int(q(1, 257)) == 0


GOOD = dict(S=2, T=5, V=778, parents=PARENTS, tips=[320, 443, 671, 554, 744], iters=20, init=1, lambda0=1e-3, w_pose=1e-6,
            w_beta=1e-6, w_limit=1e-2, sigma3=0.01, sigma2=10.0, half=[112.0, 112.0], s=[1e-3, 1e-4, 1e-2, 1e-1, 1e-1, 1e-3, 1e-1],
            free=(1 << 62) - 1, free_cam=7, ws=4096, ws_bytes=None)
# blend, joint_t, joint_s, weights_t, hands_mean, targets3, weights3, targets2, weights2, joint_map, pose_lo, pose_hi, p, cost, accepted
NPTR, OPTIONAL = 15, (5, 6, 7, 8, 10, 11)


def _call(ns, **kw):
    a = dict(GOOD)
    a["ptrs"] = [8 * (i + 1) for i in range(NPTR)]
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(int(ns.scat_mano_fit_seq_kp_ws(a["S"], a["T"])), 16)
    return ns.scat_mano_fit_seq_kp(*a["ptrs"], a["ws"], a["ws_bytes"], a["S"], a["T"], a["V"], a["parents"], *a["tips"], a["iters"],
                                   a["init"], a["lambda0"], a["w_pose"], a["w_beta"], a["w_limit"], a["sigma3"], a["sigma2"],
                                   *a["half"], *a["s"], a["free"], a["free_cam"], 0)


def test_errors_surface_without_a_gpu(built):
    """argument validation happens before any HIP call: made-up pointers are never followed, each refusal carries its
    SCAT_E_* code and names the entry point, and the kernel label does not move"""
    from scat_amd import mano
    from scat_amd._lib import ScatError, lib
    from scat_amd.fit import FIT_SEQ_KP_HEADER

    L = lib()
    ns = L.bind(FIT_SEQ_KP_HEADER)
    label = L.scat_last_kernel()

    def refused(code, pattern, **kw):
        with pytest.raises(ScatError, match=rf"{ENTRY} failed \({code}\): {ENTRY}: .*{pattern}"):
            _call(ns, **kw)
        assert L.scat_last_kernel() == label

    base = [8 * (i + 1) for i in range(NPTR)]
    without = lambda *idx: [0 if i in idx else v for i, v in enumerate(base)]
    for i in range(NPTR):
        if i not in OPTIONAL:
            refused(-2, "null pointer", ptrs=without(i))
        refused(-2, "4-byte aligned", ptrs=base[:i] + [base[i] + 2] + base[i + 1:])
    refused(-2, "no targets: targets3 and targets2 are both null", ptrs=without(5, 6, 7, 8))
    refused(-2, "weights3 given without targets3", ptrs=without(5))
    refused(-2, "weights2 given without targets2", ptrs=without(7))
    refused(-2, "pose_lo and pose_hi must both be given or both be null", ptrs=without(10))
    refused(-2, "pose_lo and pose_hi must both be given or both be null", ptrs=without(11))
    refused(-1, "batch 0 must be positive", S=0)
    refused(-1, r"0 frames outside 1\.\.256", T=0)
    refused(-1, r"257 frames outside 1\.\.256", T=257)
    refused(-1, "0 vertices outside", V=0)
    refused(-1, rf"{mano.MAX_V + 1} vertices outside", V=mano.MAX_V + 1)
    refused(-1, "tip 2 = 778", tips=[320, 443, 778, 554, 744])
    refused(-2, r"0 iterations outside 1\.\.64", iters=0)
    refused(-2, r"65 iterations outside 1\.\.64", iters=65)
    refused(-2, "init 2 must be 0", init=2)
    refused(-2, "lambda0 0 outside", lambda0=0.0)
    refused(-2, "w_pose -1 must be finite and not negative", w_pose=-1.0)
    refused(-2, "w_beta inf must be finite", w_beta=float("inf"))
    refused(-2, "w_limit -1 must be finite and not negative", w_limit=-1.0)
    refused(-2, "sigma3 nan must be finite", sigma3=float("nan"))
    refused(-2, "sigma2 -2 must be finite and not negative", sigma2=-2.0)
    refused(-2, "half_w 0 must be positive and finite", half=[0.0, 112.0])
    refused(-2, "half_h inf must be positive and finite", half=[112.0, float("inf")])
    for i, name in enumerate(S_NAMES):
        for bad, text in ((-1.0, "-1"), (float("inf"), "inf"), (float("nan"), "nan")):
            s = list(GOOD["s"])
            s[i] = bad
            refused(-2, f"{name} {text} must be finite and not negative", s=s)
    refused(-2, "free_mask has bits above 61 set", free=1 << 62)
    refused(-2, "free_mask has bits above 61 set", free=1 << 63)
    refused(-2, r"free_cam 8 outside 0\.\.7", free_cam=8)
    refused(-2, r"free_cam -1 outside 0\.\.7", free_cam=-1)
    need = int(ns.scat_mano_fit_seq_kp_ws(GOOD["S"], GOOD["T"]))
    refused(-3, "workspace must be a 16-byte-aligned pointer", ws=0)
    refused(-3, "workspace must be a 16-byte-aligned pointer", ws=4096 + 4)
    refused(-3, f"workspace of {need - 1} bytes, {need} needed", ws_bytes=need - 1)


def test_fit_keypoints_sequence_refuses_before_the_library():
    from scat_amd._lib import ScatError
    from scat_amd.fit import SMOOTH_KP_KEYS, KeypointSequenceFitResult, ManoFitter
    from scat_amd.mano import ManoModel

    f = ManoFitter(ManoModel.synthetic(1, V=37), joint_map=JOINT_MAP)
    x3, x2 = torch.zeros(2, 3, 21, 3), torch.zeros(2, 3, 21, 2)
    with pytest.raises(ScatError, match="needs joints3d, joints2d or both"):
        f.fit_keypoints_sequence()
    with pytest.raises(ScatError, match="no CPU fallback"):
        f.fit_keypoints_sequence(x3, x2)
    with pytest.raises(ScatError, match="no CPU fallback"):
        f.fit_keypoints_sequence(joints2d=x2)
    with pytest.raises(ScatError, match=r"unknown smooth keys \['cam'\]"):
        f.fit_keypoints_sequence(joints2d=x2, smooth=dict(rots=1.0, cam=1.0))
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ScatError, match=r"smooth\['cam_scale'\] = .* must be finite and not negative"):
            f.fit_keypoints_sequence(joints2d=x2, smooth=dict(cam_scale=bad))
    with pytest.raises(ScatError, match=r"unknown smooth keys \['cam_scale'\]"):      # fit_sequence keeps its five
        f.fit_sequence(x3, smooth=dict(cam_scale=1.0))
    assert SMOOTH_KP_KEYS == ("rots", "poses", "betas", "trans", "scale", "cam_scale", "cam_trans") == QO.KEYS
    assert KeypointSequenceFitResult._fields == ("rots", "poses", "betas", "trans", "scale", "cam", "cost", "accepted", "p")


@pytest.mark.gpu
def test_fit_keypoints_sequence_refuses_shapes_and_dtypes():
    from scat_amd._lib import ScatError
    from scat_amd.fit import ManoFitter

    f = ManoFitter(host_model(37).to("cuda"), joint_map=JOINT_MAP)
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)
    for x in (z(2, 21, 2), z(0, 3, 21, 2), z(2, 257, 21, 2)):
        with pytest.raises(ScatError, match=r"needs fp32 joints3d \[S,T,21,3\] and / or joints2d \[S,T,21,2\]"):
            f.fit_keypoints_sequence(joints2d=x)
    for kw in (dict(joints2d=z(2, 3, 20, 2)), dict(joints2d=z(2, 3, 21, 2, dtype=torch.float64)),
               dict(joints3d=z(2, 3, 21, 3), joints2d=z(2, 4, 21, 2)), dict(joints2d=z(2, 3, 21, 2), w2=z(2, 21)),
               dict(joints3d=z(2, 3, 21, 3), w3=z(2, 3, 21, dtype=torch.float64))):
        with pytest.raises(ScatError, match=r"needs fp32 (joints3d|joints2d|w3|w2) \["):
            f.fit_keypoints_sequence(**kw)
    with pytest.raises(ScatError, match="weights given without their joints"):
        f.fit_keypoints_sequence(joints2d=z(2, 3, 21, 2), w3=z(2, 3, 21))
    with pytest.raises(ScatError, match=r"needs limits \(lo\[45\], hi\[45\]\)"):
        f.fit_keypoints_sequence(joints2d=z(2, 3, 21, 2), limits=(torch.zeros(44), torch.zeros(45)))
    with pytest.raises(ScatError, match="needs an fp32 start"):
        f.fit_keypoints_sequence(joints2d=z(2, 3, 21, 2), init=z(2, 3, 62))
    with pytest.raises(ScatError, match="free_cam is outside"):
        f.fit_keypoints_sequence(joints2d=z(2, 3, 21, 2), free_cam=8)
    with pytest.raises(ScatError, match="must not be negative"):
        f.fit_keypoints_sequence(joints2d=z(2, 3, 21, 2), sigma2=-1.0)
    with pytest.raises(ScatError, match="iterations outside"):
        f.fit_keypoints_sequence(joints2d=z(2, 3, 21, 2), iters=65)


# ------------------------------------------------------------------ the oracle against autograd and its two parents
def test_oracle_normal_equations_are_a_dense_autograd_jacobian():
    """the stacked residual vector of a sequence, sqrt of the IRLS weights, priors, active limits and smoothness included,
    differentiated by autograd as one dense [rows, 65 T] Jacobian: H = J^T J and g = J^T r in the free unknowns"""
    m = host_model(37)
    S, T = 2, 3
    pr, free, fc, P1, _, _, _ = G.step_case("robust", 37, S, T)
    free &= ~(0x3FF << 48)      # betas frozen as well, and ctx
    fc = 5
    s7 = QO.sm(G.SMOOTH)
    H, g, _ = QO.normal_equations(m, P1, pr, s7, free, fc)
    fp = QO.flat(pr)
    _, w3, _, w2 = KO._terms(fp, S * T, torch.float64)
    with torch.no_grad():
        r3, r2 = KO.residuals(m, P1.reshape(S * T, 65), fp)
        k3 = (w3 * KO.rho_prime((r3 * r3).sum(2), pr.sigma3)).sqrt().reshape(S, T, 21, 1)
        k2 = (w2 * KO.rho_prime((r2 * r2).sum(2), pr.sigma2)).sqrt().reshape(S, T, 21, 1)
        act = (KO.excess(P1.reshape(S * T, 65), fp) != 0).reshape(S, T, 45)
    assert bool(act.any()) and bool((k2 < 0.9 * k2.max()).any())      # limits are active and outliers are down-weighted
    d = QO.dvec(s7, torch.float64)

    def rows(q):      # [S, rows] of sequence-wise stacked residuals at q [S, 65 T]
        Q = q.reshape(S, T, 65)
        a3, a2 = KO.residuals(m, Q.reshape(S * T, 65), fp)
        ex = KO.excess(Q.reshape(S * T, 65), fp).reshape(S, T, 45)
        parts = [(k3 * a3.reshape(S, T, 21, 3)).reshape(S, -1), (k2 * a2.reshape(S, T, 21, 2)).reshape(S, -1),
                 (pr.w_pose ** 0.5 * Q[:, :, 3:48]).reshape(S, -1), (pr.w_beta ** 0.5 * Q[:, :, 48:58]).reshape(S, -1),
                 (pr.w_limit ** 0.5 * ex * act).reshape(S, -1), (d.sqrt() * (Q[:, 1:] - Q[:, :-1])).reshape(S, -1)]
        return torch.cat(parts, dim=1)

    q0 = P1.reshape(S, T * 65)
    J = torch.autograd.functional.jacobian(lambda q: rows(q).sum(0), q0, vectorize=True).permute(1, 0, 2)      # [S,rows,65T]
    with torch.no_grad():
        r = rows(q0)
    fr = QO.free_vec(free, fc, torch.float64).repeat(T)
    keep = fr[:, None] * fr[None, :]
    Hd = J.transpose(1, 2) @ J * keep + torch.diag(1.0 - fr)
    gd = (J.transpose(1, 2) @ r.unsqueeze(2)).squeeze(2) * fr
    assert QO.rel(H.numpy(), Hd.numpy()) < 1e-12 and QO.rel(g.numpy(), gd.numpy()) < 1e-12
    B = H.reshape(S, T, 65, T, 65)
    assert float(B[:, 0, :, 2].abs().max()) == 0.0      # block-tridiagonal
    assert torch.equal(B[:, 1, :, 0], torch.diag(-d * QO.free_vec(free, fc, torch.float64)).expand(S, 65, 65))
    L = torch.linalg.cholesky(H).reshape(S, T, 65, T, 65)      # the dense factor has the kernel's blocks
    assert float(L[:, 2, :, 0].abs().max()) == 0.0


def test_oracle_single_frames_without_smoothness_are_the_keypoint_oracle():
    m = host_model(37)
    for name in ("both", "2d", "robust"):
        pr, free, fc, P1, _, _, _ = G.step_case(name, 37, 2, 1)
        a = QO.lm(m, pr, P1, 3, (0.0,) * 7, 1e-2, free, fc, history=True)
        b = KO.lm(m, QO.flat(pr), P1[:, 0], 3, 1e-2, free, fc, history=True)
        assert a[2].tolist() == b[2].tolist() and min(a[2].tolist()) >= 1, name
        for k in range(3):      # step for step
            assert float((a[4][k][:, 0] - b[4][k]).abs().max()) < 1e-11 and float((a[3][k] - b[3][k]).abs().max()) < 1e-14, (name, k)


def test_oracle_without_2d_robust_loss_limits_and_camera_is_the_sequence_oracle():
    m = host_model(37)
    S, T = 2, 3
    X, P1, _, _ = SC.step_case(37, S, T)
    pr = KO.Problem(JOINT_MAP, T3=X, half=G.HALF)
    P65 = torch.cat([P1, torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64).expand(S, T, 3)], dim=2)
    s5 = SC.sm(SC.SMOOTH)
    a = QO.lm(m, pr, P65, 3, s5 + (0.0, 0.0), 1e-2, G.ALL, 0, history=True)
    b = SO.lm(m, X.double(), SC.ones(S, T), JOINT_MAP, P1, 3, s5, lambda0=1e-2, history=True)
    assert a[2].tolist() == b[2].tolist() and min(a[2].tolist()) >= 1
    assert float((a[0][..., :62] - b[0]).abs().max()) < 1e-11 and torch.equal(a[0][..., 62:], P65[..., 62:])
    assert float((a[3] - b[3]).abs().max()) < 1e-14      # the costs, step for step


def test_oracle_start_is_the_keypoint_oracles_then_the_sequence_scan():
    m = host_model(37)
    pr, S, T, P0, _ = G.start_case("pi")
    n = P0[0, :, :3].norm(dim=1)
    assert float(n[0]) < torch.pi < float(n[-1]) and float((P0[0, 1:, :3] - P0[0, :-1, :3]).norm(dim=1).max()) < 0.5
    per = KO.start(m, QO.flat(pr), S * T).reshape(S, T, 65)
    assert torch.equal(per[:, :, 3:], P0[:, :, 3:]) and not torch.equal(per[:, :, :3], P0[:, :, :3])
    pr, S, T, P0, _ = G.start_case("gap0")
    per = KO.start(m, QO.flat(pr), S * T).reshape(S, T, 65)
    assert torch.equal(P0[:, 0], P0[:, 1]) and torch.equal(P0[:, 1:, 3:], per[:, 1:, 3:]) and float(per[:, 0, :62].abs().max()) == 0.0
    pr, S, T, P0, _ = G.start_case("gap_mid")
    assert torch.equal(P0[:, 2], P0[:, 1]) and not torch.equal(P0[:, 3], P0[:, 2])
    none = pr._replace(w3=torch.zeros(S, T, 21), w2=torch.zeros(S, T, 21))
    Z = QO.start(m, none, S, T)
    assert float(Z[..., :62].abs().max()) == 0.0 and torch.equal(Z[..., 62:], torch.tensor([1.0, 0.0, 0.0]).double().expand(S, T, 3))


# ------------------------------------------------------------------ conditions on the fixed inputs
def test_step_cases_are_accepted_and_the_robust_one_has_active_limits():
    for name in ("both", "2d", "robust"):
        for T in (1, 2, 3, 5):
            assert G.step_case(name, 37, 2, T)[6].tolist() == [1, 1], (name, T)


def test_condition_noisy_tracks():
    """1 px of noise on 2-D-only tracks of 8 frames, 8 iterations: the oracle's sequence fit has a smaller accel_error against
    the truth than its per-frame fits on every track, in fp64 and in fp32 (tools/fit_seq_kp_gates.py: 0.52 / 0.92 mm against
    114 / 39 mm), and its steps are accepted"""
    assert (G.NOISE_PX, G.NOISE_T, G.NOISE_S, G.NOISE_ITERS) == (1.0, 8, 2, 8)
    X, T2n, out = G.noisy_case()
    for dt in ("fp64", "fp32"):
        print(dt, "sequence", out["seq", dt], "per frame", out["frame", dt])
        assert (2 * out["seq", dt] + 1e-5 < out["frame", dt]).all(), dt      # the GPU gate's bound is still a win


def test_condition_gap_and_outliers():
    X, pr, r0, rf = G.gap_case()
    print(f"gap: start {1e3 * r0:.3f} mm, bridged {1e3 * rf:.4f} mm")
    assert float(pr.w3[0, G.GAP_AT].abs().max()) == 0.0 and float(pr.w2[0, G.GAP_AT].abs().max()) == 0.0
    assert rf < 0.1 * r0 and r0 > 5e-3
    _, _, _, inl, r = G.robust_case()
    at = G.outlier_frame(G.ROBUST_T)
    print("outliers: inlier reprojection RMS in px, robust", r["gm"], "quadratic", r["quad"])
    assert int((~inl).sum()) == 3 * G.ROBUST_S and bool((~inl[:, at]).sum(1).eq(3).all())
    assert (r["quad"][:, at] > 2 * r["gm"][:, at] + G.px_floor(G.ROBUST_S)).all()      # worse by more than the GPU gate's slack
