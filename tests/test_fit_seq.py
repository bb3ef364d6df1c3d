"""The MANO fit to a track of frames, the parts that need no GPU: the public header and its binding beside HEADERS, every
refusal of the entry point, the workspace query, ManoFitter.fit_sequence's own refusals, the fp64 oracle of
tests/_fit_seq_oracle.py against itself, and the conditions on the fixed inputs the GPU tests gate
(tests/test_gpu_fit_seq.py), so that no failure there can be blamed on the data."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_oracle as FO  # noqa: E402
import _fit_seq_cases as G  # noqa: E402
import _fit_seq_oracle as SO  # noqa: E402
from _fit_cases import JOINT_MAP, host_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ_H = os.path.join(ROOT, "include", "scat_mano_fit_seq.h")
PARENTS = sum(p << (4 * i) for i, p in enumerate((0, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)))
ENTRY = "scat_mano_fit_seq"


@pytest.fixture(scope="module")
def built():
    from scat_amd import build

    return build.build(verbose=False)


def test_seq_header_is_bound_beside_the_seven(built):
    from scat_amd import build, fit
    from scat_amd._lib import EXTENSION_HEADERS, FIT_SEQ_HEADER, HEADERS, lib, parse_header

    assert os.path.samefile(FIT_SEQ_HEADER, SEQ_H) and EXTENSION_HEADERS == (FIT_SEQ_HEADER,)
    assert len(HEADERS) == 7 and FIT_SEQ_HEADER not in HEADERS
    protos = parse_header(SEQ_H)
    assert set(protos) == {"scat_mano_fit_seq_ws", "scat_mano_fit_seq"}
    L = lib()
    assert L.by_extension == {FIT_SEQ_HEADER: protos} and list(L.by_header) == list(HEADERS)
    assert not set(protos) & set(L.protos) and all(not set(protos) & set(p) for p in L.by_header.values())
    for name in protos:
        assert hasattr(L.cdll, name) and callable(getattr(L, name)), name
    assert protos["scat_mano_fit_seq_ws"][0] is ctypes.c_int64
    assert [ty for ty, _ in protos["scat_mano_fit_seq_ws"][1]] == [ctypes.c_int, ctypes.c_int]
    rt, args = protos[ENTRY]
    by = dict((an, ty) for ty, an in args)
    assert rt is ctypes.c_int and args[-1][1] == "stream" and getattr(L, ENTRY).__name__ == ENTRY      # the checked wrapper
    assert by["ws"] is ctypes.c_void_p and by["ws_bytes"] is ctypes.c_int64 and by["free_mask"] is ctypes.c_uint64
    assert by["S"] is ctypes.c_int and by["T"] is ctypes.c_int and by["parents"] is ctypes.c_uint64
    assert [an for _, an in args if an.startswith("s_")] == ["s_rots", "s_poses", "s_betas", "s_trans", "s_scale"]
    assert all(by[k] is ctypes.c_float for k in ("s_rots", "s_poses", "s_betas", "s_trans", "s_scale", "lambda0", "w_pose", "w_beta"))
    src = open(SEQ_H).read()
    assert f"#define SCAT_FIT_SEQ_MAX_T {fit.SEQ_MAX_T}\n" in src
    for word in ("UNITS", "axis-angle"):
        assert word in src and word in fit.ManoFitter.fit_sequence.__doc__, word
    assert "weights are all zero" in fit.ManoFitter.fit_sequence.__doc__      # the zero-weight-frame rule
    assert build._public_headers_mtime() >= os.path.getmtime(SEQ_H)      # the header is a rebuild trigger
    newest = max(os.path.getmtime(os.path.join(ROOT, "include", h)) for h in os.listdir(os.path.join(ROOT, "include")))
    assert build._public_headers_mtime() == newest


def test_a_missing_symbol_raises(built, monkeypatch, tmp_path):
    """an extension header that declares what the library lacks fails the binding, like a header of HEADERS"""
    from scat_amd import _lib

    h = tmp_path / "scat_nothing.h"
    h.write_text("int scat_no_such_entry_point(int a, void* stream);\n")
    monkeypatch.setattr(_lib, "EXTENSION_HEADERS", (str(h),))
    with pytest.raises(AttributeError, match="scat_no_such_entry_point"):
        _lib._Lib()


GOOD = dict(S=2, T=5, V=778, parents=PARENTS, tips=[320, 443, 671, 554, 744], iters=20, init=1, lambda0=1e-3, w_pose=1e-6,
            w_beta=1e-6, s=[1e-3, 1e-4, 1e-2, 1e-1, 1e-1], free=(1 << 62) - 1, ws=4096, ws_bytes=None)


def _call(L, **kw):
    a = dict(GOOD)
    a["ptrs"] = [8 * (i + 1) for i in range(11)]
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(int(L.scat_mano_fit_seq_ws(a["S"], a["T"])), 16)
    return L.scat_mano_fit_seq(*a["ptrs"], a["ws"], a["ws_bytes"], a["S"], a["T"], a["V"], a["parents"], *a["tips"], a["iters"],
                               a["init"], a["lambda0"], a["w_pose"], a["w_beta"], *a["s"], a["free"], 0)


def test_seq_errors_surface_without_a_gpu(built):
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

    base = [8 * (i + 1) for i in range(11)]
    for i in range(11):
        if i != 6:      # weights: null means all ones
            refused(-2, "null pointer", ptrs=base[:i] + [0] + base[i + 1:])
        refused(-2, "4-byte aligned", ptrs=base[:i] + [base[i] + 2] + base[i + 1:])
    refused(-1, "batch 0 must be positive", S=0)
    refused(-1, "batch -3 must be positive", S=-3)
    refused(-1, r"0 frames outside 1\.\.256", T=0)
    refused(-1, r"257 frames outside 1\.\.256", T=257)
    refused(-1, "0 vertices outside", V=0)
    refused(-1, rf"{mano.MAX_V + 1} vertices outside", V=mano.MAX_V + 1)
    refused(-1, "tip 2 = 778", tips=[320, 443, 778, 554, 744])
    refused(-2, r"parent\[3\] = 7", parents=(PARENTS & ~(15 << 12)) | (7 << 12))
    refused(-2, r"0 iterations outside 1\.\.64", iters=0)
    refused(-2, r"65 iterations outside 1\.\.64", iters=65)
    refused(-2, "init 2 must be 0", init=2)
    refused(-2, "lambda0 0 outside", lambda0=0.0)
    refused(-2, "lambda0 nan outside", lambda0=float("nan"))
    refused(-2, "w_pose -1 must be finite and not negative", w_pose=-1.0)
    refused(-2, "w_beta inf must be finite", w_beta=float("inf"))
    for i, name in enumerate(("s_rots", "s_poses", "s_betas", "s_trans", "s_scale")):
        for bad, text in ((-1.0, "-1"), (float("inf"), "inf"), (float("nan"), "nan")):
            s = list(GOOD["s"])
            s[i] = bad
            refused(-2, f"{name} {text} must be finite and not negative", s=s)
    refused(-2, "free_mask has bits above 61 set", free=1 << 62)
    refused(-2, "free_mask has bits above 61 set", free=1 << 63)
    need = int(L.scat_mano_fit_seq_ws(GOOD["S"], GOOD["T"]))
    refused(-3, "workspace must be a 16-byte-aligned pointer", ws=0)
    refused(-3, "workspace must be a 16-byte-aligned pointer", ws=4096 + 4)
    refused(-3, f"workspace of {need - 1} bytes, {need} needed", ws_bytes=need - 1)


def test_workspace_query():
    from scat_amd._lib import lib

    q = lib().scat_mano_fit_seq_ws
    sizes = [(1, 1), (1, 2), (2, 2), (2, 5), (3, 5), (3, 256), (1024, 16)]
    got = [int(q(S, T)) for S, T in sizes]
    assert all(g > 0 and g % 4 == 0 for g in got) and got == sorted(got) and len(set(got)) == len(got)
    assert int(q(2, 5)) == 2 * 5 * int(q(1, 1))
    for S, T in ((0, 5), (-1, 5), (2, 0), (2, -1), (2, 257)):
        assert int(q(S, T)) == 0, (S, T)


def test_fit_sequence_refuses_before_the_library():
    from scat_amd._lib import ScatError
    from scat_amd.fit import SEQ_MAX_T, ManoFitter, SequenceFitResult
    from scat_amd.mano import ManoModel

    f = ManoFitter(ManoModel.synthetic(1, V=37), joint_map=JOINT_MAP)
    x = torch.zeros(2, 3, 21, 3)
    with pytest.raises(ScatError, match="no CPU fallback"):
        f.fit_sequence(x)
    with pytest.raises(ScatError, match="no CPU fallback"):
        f.fit_outputs_sequence(torch.zeros(2, 3, 66))
    with pytest.raises(ScatError, match=r"unknown smooth keys \['twist'\]"):
        f.fit_sequence(x, smooth=dict(rots=1.0, twist=1.0))
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ScatError, match=r"smooth\['betas'\] = .* must be finite and not negative"):
            f.fit_sequence(x, smooth=dict(betas=bad))
    assert SEQ_MAX_T == 256 and SequenceFitResult._fields == ("rots", "poses", "betas", "trans", "scale", "cost", "accepted", "p")


@pytest.mark.gpu
def test_fit_sequence_refuses_shapes_and_dtypes():
    from scat_amd._lib import ScatError
    from scat_amd.fit import ManoFitter

    f = ManoFitter(host_model(37).to("cuda"), joint_map=JOINT_MAP)
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)
    for x in (z(2, 21, 3), z(0, 3, 21, 3), z(2, 257, 21, 3), z(2, 3, 20, 3), z(2, 3, 21, 3, dtype=torch.float64)):
        with pytest.raises(ScatError, match=r"needs fp32 joints \[S,T,21,3\]"):
            f.fit_sequence(x)
    with pytest.raises(ScatError, match="needs fp32 weights"):
        f.fit_sequence(z(2, 3, 21, 3), z(2, 21))
    with pytest.raises(ScatError, match="needs an fp32 start"):
        f.fit_sequence(z(2, 3, 21, 3), init=z(2, 62))
    with pytest.raises(ScatError, match="needs the network's outputs"):
        f.fit_outputs_sequence(z(2, 66))


# ------------------------------------------------------------------ the oracle against itself
def small():
    m = host_model(37)
    X, P1, _, _ = G.step_case(37, 2, 3)
    return m, X.double(), P1, G.ones(2, 3)


def test_oracle_gradient_is_half_the_central_difference_of_the_cost():
    """g of the dense normal equations against central differences of the cost in fp64, every unknown of every frame:
    the smoothness couples the frames, so the middle frame's g holds both neighbours"""
    m, X, P, w = small()
    s5 = G.sm(G.SMOOTH_NOISY)      # the strong one, so that the smoothness is no rounding error of the data term
    _, g, _ = SO.normal_equations(m, P, X, w, JOINT_MAP, 1e-6, 1e-6, s5)
    h, fd = 1e-6, torch.zeros(2, 3 * 62, dtype=torch.float64)
    with torch.no_grad():
        for i in range(3 * 62):
            e = torch.zeros(2, 3 * 62, dtype=torch.float64)
            e[:, i] = h
            e = e.reshape(2, 3, 62)
            fd[:, i] = (SO.cost(m, P + e, X, w, JOINT_MAP, 1e-6, 1e-6, s5) - SO.cost(m, P - e, X, w, JOINT_MAP, 1e-6, 1e-6, s5)) / (2 * h)
    assert FO.rel(g.numpy(), 0.5 * fd.numpy()) < 1e-7
    for t in range(3):      # frame by frame as well
        sl = slice(62 * t, 62 * (t + 1))
        assert FO.rel(g[:, sl].numpy(), 0.5 * fd[:, sl].numpy()) < 1e-7, t


def test_oracle_single_frame_without_smoothness_is_the_frame_oracle():
    m = host_model(37)
    X, P1, _, _ = G.step_case(37, 2, 1)
    a = SO.lm(m, X.double(), G.ones(2, 1), JOINT_MAP, P1, 1, (0.0,) * 5, lambda0=1e-2)
    b = FO.lm(m, X[:, 0].double(), torch.ones(2, 21, dtype=torch.float64), JOINT_MAP, P1[:, 0], 1, lambda0=1e-2)
    assert a[2].tolist() == [1, 1] == b[2].tolist()
    assert float((a[0][:, 0] - b[0]).abs().max()) < 1e-12 and float((a[1] - b[1]).abs().max()) < 1e-15


def test_oracle_matrix_is_block_tridiagonal():
    from scat_amd.fit import free_mask

    m, X, P, w = small()
    s5 = G.sm(G.SMOOTH)
    free = free_mask(betas=False)
    H, g, _ = SO.normal_equations(m, P, X, w, JOINT_MAP, 1e-6, 1e-6, s5, free)
    d = SO.dvec(s5, torch.float64) * SO.free_vec(free, torch.float64)
    assert float(d[48:58].abs().max()) == 0.0 and float(d.max()) > 0.0
    B = H.reshape(2, 3, 62, 3, 62)
    assert float(B[:, 0, :, 2].abs().max()) == 0.0 and float(B[:, 2, :, 0].abs().max()) == 0.0
    for t in (0, 1):
        assert torch.equal(B[:, t + 1, :, t], torch.diag(-d).expand(2, 62, 62)) and torch.equal(B[:, t, :, t + 1], B[:, t + 1, :, t])
    assert torch.equal(H, H.transpose(1, 2))
    A, _, _ = FO.normal_equations(m, P.reshape(6, 62), X.reshape(6, 21, 3), w.reshape(6, 21), JOINT_MAP, 1e-6, 1e-6, free)
    for t, nb in enumerate((1, 2, 1)):
        assert torch.equal(B[:, t, :, t], A.reshape(2, 3, 62, 62)[:, t] + torch.diag(nb * d))
    # frozen: unit rows, nothing in g
    assert torch.equal(B[:, 1, 48:58, 1, 48:58], torch.eye(10, dtype=torch.float64).expand(2, 10, 10))
    assert float(g.reshape(2, 3, 62)[:, :, 48:58].abs().max()) == 0.0
    # the dense factor has the kernel's blocks: nothing below the first sub-diagonal block
    L = torch.linalg.cholesky(H).reshape(2, 3, 62, 3, 62)
    assert float(L[:, 2, :, 0].abs().max()) == 0.0


def test_oracle_start_is_the_frame_oracles_and_fills_frames_without_weight():
    m = host_model(37)
    P, X, P0 = G.start_case()
    per = FO.procrustes_start(m, X.reshape(10, 21, 3), torch.ones(10, 21), JOINT_MAP).reshape(2, 5, 62)
    assert float((P0 - per).abs().max()) < 1e-12      # no frame of this case crosses pi
    w = G.ones(2, 5)
    w[0, 0], w[0, 1], w[0, 3], w[1] = 0.0, 0.0, 0.0, 0.0
    Q = SO.start(m, X, w, JOINT_MAP)
    assert torch.equal(Q[0, 0], P0[0, 2]) and torch.equal(Q[0, 1], P0[0, 2]) and torch.equal(Q[0, 3], P0[0, 2])
    assert torch.equal(Q[0, 4], P0[0, 4]) and float(Q[1].abs().max()) == 0.0
    Pp, Xp, P0p = G.pi_case()
    n = P0p[0, :, :3].norm(dim=1)
    assert float(n[0]) < np.pi < float(n[-1]) and float((P0p[0, 1:, :3] - P0p[0, :-1, :3]).norm(dim=1).max()) < 0.5
    jp = SO.frame_joints(m, P0p, JOINT_MAP)      # the longer axis-angle is the same rotation: the start still fits
    assert float((jp - Xp.double()).abs().max()) < 0.05


# ------------------------------------------------------------------ conditions on the fixed inputs
def test_condition_a_smoothing_case():
    """(a) noise 2 mm, T = 8, S = 2, 6 iterations, smooth rots 3e-2, poses 1e-2, betas 1e-1, trans 3, scale 1: the
    oracle's sequence fit has an accel_error against the truth below half that of its per-frame fits with a factor 1.5
    to spare, in fp64 and in fp32 (tools/fit_seq_gates.py: 1.37 / 1.44 mm against 22.8 / 11.3 mm)"""
    assert (G.NOISE, G.NOISE_T, G.NOISE_S, G.NOISE_ITERS) == (2e-3, 8, 2, 6) and G.NOISE_T <= 8
    assert G.SMOOTH_NOISY == dict(rots=3e-2, poses=1e-2, betas=1e-1, trans=3.0, scale=1.0)
    X, Xn, out = G.noisy_case()
    for dt in ("fp64", "fp32"):
        print(dt, "sequence", out["seq", dt], "per frame", out["frame", dt])
        assert (1.5 * out["seq", dt] < 0.5 * out["frame", dt]).all(), dt


def test_condition_b_gap_case():
    """(b) the oracle's bridged frame is closer to the truth than the frame's start, which is its neighbour's"""
    X, w, r0, rf = G.gap_case()
    print(f"start {1e3 * r0:.3f} mm, bridged {1e3 * rf:.4f} mm")
    assert float(w[0, G.GAP_AT].abs().max()) == 0.0 and float(w.sum()) == 21.0 * (G.GAP_T - 1)
    assert rf < 0.1 * r0 and r0 > 5e-3
