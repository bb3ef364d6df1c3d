"""The MANO fit, the parts that need no GPU: the public header and its binding, argument errors of both entry points,
ManoFitter's refusal of CPU tensors, and the fp64 oracle of tests/_fit_oracle.py converging on the fixed cases the GPU
tests gate (tests/test_gpu_fit.py), which shows those inputs fit for the gates."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_oracle as FO  # noqa: E402
import _mano_oracle as MO  # noqa: E402

from _fit_cases import JOINT_MAP  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT_H = os.path.join(ROOT, "include", "scat_mano_fit.h")
PARENTS = sum(p << (4 * i) for i, p in enumerate((0, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)))


@pytest.fixture(scope="module")
def built():
    from scat_amd import build

    return build.build(verbose=False)


def test_fit_header_is_bound(built):
    from scat_amd import fit
    from scat_amd._lib import FIT_HEADER, HEADERS, RENDER_HEADER, lib, parse_header

    assert os.path.samefile(FIT_HEADER, FIT_H) and FIT_HEADER in HEADERS
    assert HEADERS.index(FIT_HEADER) == HEADERS.index(RENDER_HEADER) - 1      # inserted before the renderer's
    protos = parse_header(FIT_H)
    assert set(protos) == {"scat_mano_joints_jac", "scat_mano_fit"}
    L = lib()
    for name, (rt, args) in protos.items():
        assert hasattr(L.cdll, name) and callable(getattr(L, name)), name
        assert rt is ctypes.c_int and args[-1][1] == "stream", name
        names = [an for _, an in args]
        assert "ws" not in names and "ws_bytes" not in names and not name.endswith("_ws")
        assert dict((an, ty) for ty, an in args)["parents"] is ctypes.c_uint64
        assert [ty for ty, an in args if an.startswith("tip")] == [ctypes.c_int] * 5
    by = dict((an, ty) for ty, an in protos["scat_mano_fit"][1])
    assert by["free_mask"] is ctypes.c_uint64 and by["w_pose"] is ctypes.c_float and by["w_beta"] is ctypes.c_float
    assert by["lambda0"] is ctypes.c_float and by["iters"] is ctypes.c_int and by["init"] is ctypes.c_int
    assert L.by_header[FIT_HEADER] == protos and list(L.by_header) == list(HEADERS) and not set(protos) & set(L.protos)
    for h in HEADERS:
        if not os.path.samefile(h, FIT_H):
            assert not set(protos) & set(parse_header(h)), h
    src = open(FIT_H).read()
    assert f"#define SCAT_FIT_UNKNOWNS {fit.UNKNOWNS}\n" in src and f"#define SCAT_FIT_MAX_ITERS {fit.MAX_ITERS}\n" in src
    assert "CLAMPED" in src      # what happens to joint_map entries outside 0..20 is stated
    from scat_amd import build

    saved = os.path.getmtime(FIT_H)
    assert build._public_headers_mtime() >= saved      # the header is a rebuild trigger


GOOD = dict(B=4, V=778, parents=PARENTS, tips=[320, 443, 671, 554, 744])
FIT_TAIL = dict(iters=20, init=1, lambda0=1e-3, w_pose=1e-6, w_beta=1e-6, free=(1 << 62) - 1)


def _call(L, entry, **kw):
    a = dict(GOOD, **FIT_TAIL)
    a["ptrs"] = [8 * (i + 1) for i in range(10 if entry == "scat_mano_joints_jac" else 11)]
    a.update(kw)
    tail = () if entry == "scat_mano_joints_jac" else (a["iters"], a["init"], a["lambda0"], a["w_pose"], a["w_beta"], a["free"])
    return getattr(L, entry)(*a["ptrs"], a["B"], a["V"], a["parents"], *a["tips"], *tail, 0)


def _with_parent(i, p):
    return (PARENTS & ~(15 << (4 * i))) | (p << (4 * i))


@pytest.mark.parametrize("entry", ["scat_mano_joints_jac", "scat_mano_fit"])
def test_fit_errors_surface_without_a_gpu(built, entry):
    """argument validation happens before any HIP call: made-up pointers are never followed, each refusal carries its
    SCAT_E_* code and names the entry point, and the kernel label does not move"""
    from scat_amd import mano
    from scat_amd._lib import ScatError, lib

    L = lib()
    label = L.scat_last_kernel()
    nptr = 10 if entry == "scat_mano_joints_jac" else 11

    def refused(code, pattern, **kw):
        with pytest.raises(ScatError, match=rf"{entry} failed \({code}\): {entry}: .*{pattern}"):
            _call(L, entry, **kw)
        assert L.scat_last_kernel() == label

    base = [8 * (i + 1) for i in range(nptr)]
    for i in range(nptr):
        if entry == "scat_mano_fit" and i == 6:      # weights: null means all ones
            continue
        refused(-2, "null pointer", ptrs=base[:i] + [0] + base[i + 1:])
    for i in range(nptr):
        refused(-2, "4-byte aligned", ptrs=base[:i] + [base[i] + 2] + base[i + 1:])
    refused(-1, "batch 0 must be positive", B=0)
    refused(-1, "batch -3 must be positive", B=-3)
    refused(-1, "0 vertices outside", V=0)
    refused(-1, rf"{mano.MAX_V + 1} vertices outside 1\.\.{mano.MAX_V}", V=mano.MAX_V + 1)
    for j in range(5):
        tips = list(GOOD["tips"])
        tips[j] = 778
        refused(-1, rf"tip {j} = 778", tips=tips)
    refused(-1, "tip 0 = -1", tips=[-1, 443, 671, 554, 744])
    for i, p in ((1, 1), (3, 7), (15, 15)):
        refused(-2, rf"parent\[{i}\] = {p}", parents=_with_parent(i, p))
    refused(-2, r"parent\[0\] = 5", parents=_with_parent(0, 5))
    if entry == "scat_mano_fit":
        refused(-2, r"0 iterations outside 1\.\.64", iters=0)
        refused(-2, r"65 iterations outside 1\.\.64", iters=65)
        refused(-2, "init 2 must be 0", init=2)
        refused(-2, "lambda0 0 outside", lambda0=0.0)
        refused(-2, "lambda0 nan outside", lambda0=float("nan"))
        refused(-2, "w_pose -1 must be finite and not negative", w_pose=-1.0)
        refused(-2, "w_beta -0.5 must be finite and not negative", w_beta=-0.5)
        refused(-2, "w_beta inf must be finite", w_beta=float("inf"))
        refused(-2, "free_mask has bits above 61 set", free=1 << 62)
        refused(-2, "free_mask has bits above 61 set", free=1 << 63)


def test_fitter_has_no_cpu_fallback():
    from scat_amd._lib import ScatError
    from scat_amd.fit import ManoFitter, free_mask, mano_joints_jac
    from scat_amd.mano import ManoModel

    m = ManoModel.synthetic(1, V=37)
    f = ManoFitter(m, joint_map=JOINT_MAP)
    with pytest.raises(ScatError, match="no CPU fallback"):
        f.fit(torch.zeros(2, 21, 3))
    with pytest.raises(ScatError, match="no CPU fallback"):
        f.fit_outputs(torch.zeros(2, 66))
    with pytest.raises(ScatError, match="no CPU fallback"):
        mano_joints_jac(m, torch.zeros(2, 3), torch.zeros(2, 45), torch.zeros(2, 10))
    with pytest.raises(ScatError, match="permutation"):
        ManoFitter(m, joint_map=(0,) * 21)
    with pytest.raises(ScatError, match="iterations"):
        ManoFitter(m, iters=65)
    assert free_mask() == (1 << 62) - 1
    assert free_mask(betas=False, log_scale=False) == ((1 << 62) - 1) & ~(0x3FF << 48) & ~(1 << 61)


def test_oracle_joints_in_any_dtype_are_the_mano_oracles():
    """joints_any, the restatement the fp32 figures come from, against _mano_oracle.forward in fp64"""
    from scat_amd.mano import ManoModel

    m = ManoModel.synthetic(337, 37)
    P, _ = FO.seeded_case(5, 4, m, JOINT_MAP)
    a = FO.joints_any(m, P[:, :3], P[:, 3:48], P[:, 48:58])
    b = MO.forward(m, P[:, :3], P[:, 3:48], P[:, 48:58])[:, :21]
    assert float((a - b).abs().max()) < 1e-15
    a32 = FO.joints_any(m, P[:, :3].float(), P[:, 3:48].float(), P[:, 48:58].float())
    assert a32.dtype == torch.float32 and MO.rel(a32.numpy(), b.numpy()) < 1e-6


def test_oracle_jacobian_agrees_with_central_differences():
    from scat_amd.mano import ManoModel

    m = ManoModel.synthetic(337, 37)
    P, _ = FO.seeded_case(5, 2, m, JOINT_MAP)
    x, jac = FO.joints_jac(m, P)
    h, fd = 1e-6, torch.zeros(2, 63, 58, dtype=torch.float64)
    with torch.no_grad():
        for i in range(58):
            e = torch.zeros(2, 62, dtype=torch.float64)
            e[:, i] = h
            fd[:, :, i] = (FO.joints(m, P + e) - FO.joints(m, P - e)).reshape(2, 63) / (2 * h)
    assert MO.rel(fd.numpy(), jac.numpy()) < 1e-7


def test_oracle_axis_angle_at_zero_and_pi():
    for r in ([0.0, 0.0, 0.0], [1e-9, -2e-9, 0.0], [np.pi - 1e-9, 0.0, 0.0], [0.0, -(np.pi - 1e-7) / np.sqrt(2), (np.pi - 1e-7) / np.sqrt(2)],
              [0.3, -1.2, 2.0]):
        r = torch.tensor([r], dtype=torch.float64)
        back = FO.rot_to_axis_angle(MO.rodrigues(r))
        assert float((back - r).abs().max()) < 1e-7 * max(1.0, float(r.abs().max())), (r, back)


@pytest.mark.parametrize("V", [37, 778])
def test_oracle_converges_on_the_fixed_cases(V):
    """the recovery case of the GPU tests: from the Procrustes start the fp64 oracle brings every sample's joint RMS from
    centimetres to below 1.5 mm in 20 iterations, the cost never rises, and the one-step case accepts its step"""
    import _fit_cases as G

    P, T, P0, Pf, want, hist = G.recovery_case(V)
    m = G.host_model(V)
    start = FO.rms(m, P0, T, JOINT_MAP).numpy()
    print(f"V {V}: start {1e3 * start} mm, after 20 iterations {1e3 * want} mm")
    assert sorted(JOINT_MAP) == list(range(21)) and JOINT_MAP != tuple(range(21))
    assert (start > 5e-3).all() and (want < 1.5e-3).all() and (want < 0.1 * start).all()
    assert (np.diff(hist, axis=0) <= 0).all()
    T1, P1, Ps, c = G.step_case(V)
    c0 = FO.cost(m, P1, T1.double(), torch.ones(6, 21, dtype=torch.float64), JOINT_MAP, 1e-6, 1e-6)
    assert bool((c < c0).all())
