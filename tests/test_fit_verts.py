"""The MANO fit to a full mesh, the parts that need no GPU: the public header and _Lib.bind, argument errors of both entry
points, ManoFitter.fit_vertices' refusal of CPU tensors, and the fp64 oracle of tests/_fit_verts_oracle.py: its Jacobian
against central differences, and its convergence on the fixed cases that the GPU tests gate
(tests/test_gpu_fit_verts.py), which shows those inputs fit for the gates."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_verts_oracle as VO  # noqa: E402
import _mano_oracle as MO  # noqa: E402

from _fit_cases import T_, host_model, params  # noqa: E402
from _fit_verts_cases import FIT_V, NB, joints_case, layer_case, recovery_case, step_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERTS_H = os.path.join(ROOT, "include", "scat_mano_fit_verts.h")
PARENTS = sum(p << (4 * i) for i, p in enumerate((0, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)))
ENTRIES = ("scat_mano_verts_jac", "scat_mano_fit_verts")


@pytest.fixture(scope="module")
def built():
    from scat_amd import build

    return build.build(verbose=False)


def test_header_declares_the_two_entry_points():
    from scat_amd import build, fit
    from scat_amd._lib import EXTENSION_HEADERS, HEADERS, parse_header

    assert os.path.samefile(fit.FIT_VERTS_HEADER, VERTS_H)
    assert not any(os.path.samefile(h, VERTS_H) for h in (*HEADERS, *EXTENSION_HEADERS))
    protos = parse_header(VERTS_H)
    assert set(protos) == set(ENTRIES)
    for name, (rt, args) in protos.items():
        names = [an for _, an in args]
        assert rt is ctypes.c_int and names[-1] == "stream", name
        assert "ws" not in names and "ws_bytes" not in names and not any(n.startswith("tip") for n in names)
        assert dict((an, ty) for ty, an in args)["parents"] is ctypes.c_uint64
    by = dict((an, ty) for ty, an in protos["scat_mano_fit_verts"][1])
    assert by["free_mask"] is ctypes.c_uint64 and by["w_pose"] is ctypes.c_float and by["w_beta"] is ctypes.c_float
    assert by["lambda0"] is ctypes.c_float and by["iters"] is ctypes.c_int and by["init"] is ctypes.c_int
    assert "joint_map" not in by
    for h in (*HEADERS, *EXTENSION_HEADERS):
        assert not set(protos) & set(parse_header(h)), h
    src = open(VERTS_H).read()
    assert "UNITS" in src and "axis-angle" in src and "4-byte-aligned" in src and "No workspace" in src
    assert build._public_headers_mtime() >= os.path.getmtime(VERTS_H)      # the header is a rebuild trigger


def test_bind_binds_the_header_and_leaves_the_tables(built):
    from scat_amd import _lib
    from scat_amd._lib import EXTENSION_HEADERS, FIT_SEQ_HEADER, HEADERS, ScatError, lib, parse_header
    from scat_amd.fit import FIT_VERTS_HEADER

    L = lib()
    before = (tuple(HEADERS), tuple(EXTENSION_HEADERS), dict(L.by_header), dict(L.by_extension), dict(L.protos))
    ns = L.bind(FIT_VERTS_HEADER)
    assert sorted(vars(ns)) == sorted(ENTRIES)
    assert L.bind(FIT_VERTS_HEADER) is ns and L.bound[FIT_VERTS_HEADER] is ns      # cached by path
    assert (tuple(_lib.HEADERS), tuple(_lib.EXTENSION_HEADERS), L.by_header, L.by_extension, L.protos) == before
    assert len(HEADERS) == 7 and EXTENSION_HEADERS == (FIT_SEQ_HEADER,) and list(L.by_header) == list(HEADERS)
    assert L.by_extension == {FIT_SEQ_HEADER: parse_header(FIT_SEQ_HEADER)}
    for name in ENTRIES:
        fn = getattr(ns, name)
        assert hasattr(L.cdll, name) and fn.__name__ == name and not hasattr(L, name)
        assert len(getattr(L.cdll, name).argtypes) == len(parse_header(FIT_VERTS_HEADER)[name][1])
    # the checked wrapper: a refusal raises with the library's message
    with pytest.raises(ScatError, match=r"scat_mano_verts_jac failed \(-2\): scat_mano_verts_jac: null pointer"):
        ns.scat_mano_verts_jac(*([0] * 10), 1, 778, PARENTS, 0)


def test_bind_raises_on_a_declared_symbol_the_library_lacks(built, tmp_path):
    from scat_amd._lib import lib

    h = tmp_path / "scat_missing.h"
    h.write_text("/* a header ahead of its library */\nint scat_version(void);\n"
                 "int scat_mano_fit_nothing(const float* x, int n, void* stream);\n")
    L = lib()
    with pytest.raises(AttributeError, match="scat_mano_fit_nothing"):
        L.bind(str(h))
    assert str(h) not in L.bound


GOOD = dict(B=4, V=778, parents=PARENTS)
FIT_TAIL = dict(iters=20, init=1, lambda0=1e-3, w_pose=1e-6, w_beta=1e-6, free=(1 << 62) - 1)
NPTR = {"scat_mano_verts_jac": 10, "scat_mano_fit_verts": 10}


def _call(ns, entry, **kw):
    a = dict(GOOD, **FIT_TAIL)
    a["ptrs"] = [8 * (i + 1) for i in range(NPTR[entry])]
    a.update(kw)
    tail = () if entry == "scat_mano_verts_jac" else (a["iters"], a["init"], a["lambda0"], a["w_pose"], a["w_beta"], a["free"])
    return getattr(ns, entry)(*a["ptrs"], a["B"], a["V"], a["parents"], *tail, 0)


def _with_parent(i, p):
    return (PARENTS & ~(15 << (4 * i))) | (p << (4 * i))


@pytest.mark.parametrize("entry", ENTRIES)
def test_errors_surface_without_a_gpu(built, entry):
    """argument validation happens before any HIP call: made-up pointers are never followed, each refusal carries its
    SCAT_E_* code and names the entry point, and the kernel label does not move"""
    from scat_amd import mano
    from scat_amd._lib import ScatError, lib
    from scat_amd.fit import FIT_VERTS_HEADER

    L = lib()
    ns = L.bind(FIT_VERTS_HEADER)
    label = L.scat_last_kernel()
    nptr = NPTR[entry]

    def refused(code, pattern, **kw):
        with pytest.raises(ScatError, match=rf"{entry} failed \({code}\): {entry}: .*{pattern}"):
            _call(ns, entry, **kw)
        assert L.scat_last_kernel() == label

    base = [8 * (i + 1) for i in range(nptr)]
    for i in range(nptr):
        if entry == "scat_mano_fit_verts" and i == 6:      # weights: null means all ones
            continue
        refused(-2, "null pointer", ptrs=base[:i] + [0] + base[i + 1:])
    for i in range(nptr):
        refused(-2, "4-byte aligned", ptrs=base[:i] + [base[i] + 2] + base[i + 1:])
    refused(-1, "batch 0 must be positive", B=0)
    refused(-1, "batch -3 must be positive", B=-3)
    refused(-1, "0 vertices outside", V=0)
    refused(-1, rf"{mano.MAX_V + 1} vertices outside 1\.\.{mano.MAX_V}", V=mano.MAX_V + 1)
    for i, p in ((1, 1), (3, 7), (15, 15)):
        refused(-2, rf"parent\[{i}\] = {p}", parents=_with_parent(i, p))
    refused(-2, r"parent\[0\] = 5", parents=_with_parent(0, 5))
    if entry == "scat_mano_fit_verts":
        refused(-2, r"0 iterations outside 1\.\.64", iters=0)
        refused(-2, r"65 iterations outside 1\.\.64", iters=65)
        refused(-2, "init 2 must be 0", init=2)
        refused(-2, "init -1 must be 0 .*Procrustes over the vertices", init=-1)
        refused(-2, "lambda0 0 outside", lambda0=0.0)
        refused(-2, "lambda0 nan outside", lambda0=float("nan"))
        refused(-2, "w_pose -1 must be finite and not negative", w_pose=-1.0)
        refused(-2, "w_beta -0.5 must be finite and not negative", w_beta=-0.5)
        refused(-2, "w_beta inf must be finite", w_beta=float("inf"))
        refused(-2, "free_mask has bits above 61 set", free=1 << 62)
        refused(-2, "free_mask has bits above 61 set", free=1 << 63)


def test_fit_vertices_has_no_cpu_fallback():
    from scat_amd._lib import ScatError
    from scat_amd.fit import ManoFitter, mano_verts_jac

    m = host_model(37)
    f = ManoFitter(m)
    with pytest.raises(ScatError):
        f.fit_vertices(torch.zeros(2, 37, 3))
    with pytest.raises(ScatError):
        f.fit_mesh_outputs(torch.zeros(2, 58, 3))
    with pytest.raises(ScatError):
        mano_verts_jac(m, torch.zeros(2, 3), torch.zeros(2, 45), torch.zeros(2, 10))


def test_oracle_verts_in_either_dtype_are_the_layers():
    """verts_any, which the fp32 runs behind the gates use, is _mano_oracle.forward's mesh when it is run in fp64"""
    m = host_model(37)
    P = T_(params(7400, 3)).double()
    want = MO.forward(m, P[:, :3], P[:, 3:48], P[:, 48:58])[:, 21:]
    got = VO.verts_any(m, P[:, :3], P[:, 3:48], P[:, 48:58])
    # fp64 against fp64: rodrigues_any runs _mano_oracle.rodrigues there, the rest differs in the order of a subtraction
    assert VO.rel(got.numpy(), want.numpy()) < 1e-14


@pytest.mark.parametrize("V", [1, 37])
def test_oracle_jacobian_agrees_with_central_differences(V):
    """h = 1e-5 in fp64: truncation h^2 |f'''| / 6 ~ 1e-11 and rounding eps |f| / h ~ 1e-11 against entries of order 0.1"""
    m = host_model(V)
    P = T_(params(7401, 2)).double()
    x, jac = VO.verts_jac(m, P)
    assert x.shape == (2, V, 3) and jac.shape == (2, 3 * V, 58)
    h = 1e-5
    for q in range(58):
        e = torch.zeros(58, dtype=torch.float64)
        e[q] = h
        with torch.no_grad():
            fd = (VO.verts(m, P + e) - VO.verts(m, P - e)).reshape(2, 3 * V) / (2 * h)
        assert float((fd - jac[:, :, q]).abs().max()) < 1e-8 * max(1.0, float(jac.abs().max())), q


@pytest.mark.parametrize("V", FIT_V)
def test_oracle_converges_on_the_seeded_hands(V):
    """the cost never rises, every hand ends far below its start and below 0.1 mm, and the same hands fitted to their 21
    joints keep a vertex error that the vertex fit does not: what test_gpu_fit_verts.py's recovery gates rest on"""
    m = host_model(V)
    P, Tv, P0, Pf, final, hist = recovery_case(V)
    assert hist.shape == (20, NB) and np.isfinite(hist).all()
    assert (hist[1:] <= hist[:-1]).all() and (hist[-1] < hist[0]).all()
    start = VO.rms(m, P0, Tv).numpy()
    print(f"V {V}: start {1e3 * start} mm, after 20 {1e3 * final} mm")
    assert (final < 1e-4).all() and (final < 1e-2 * start).all()
    _, _, left = joints_case(V)
    print(f"V {V}: the joints fit leaves {1e3 * left} mm on the vertices")
    assert (left > 2 * final + 1e-5).all()


def test_oracle_converges_on_the_layers_hands():
    """layer_case, which the end-to-end GPU test gates on: the same hands without translation and scale"""
    V = 778
    P, Tv, P0, Pf, final, hist = layer_case(V)
    assert hist.shape == (20, NB) and (hist[1:] <= hist[:-1]).all() and (hist[-1] < hist[0]).all()
    start = VO.rms(host_model(V), P0, Tv).numpy()
    print(f"layer case: start {1e3 * start} mm, after 20 {1e3 * final} mm")
    assert (final < 1e-4).all() and (final < 1e-2 * start).all()


@pytest.mark.parametrize("V", FIT_V)
def test_oracle_step_is_accepted_and_lowers_the_cost(V):
    """step_case, which the one-step GPU test gates on: from 0.05 off the truth one step with lambda = 1e-2 is accepted for
    every hand, moves every hand and lowers its cost and its vertex RMS"""
    m = host_model(V)
    Tv, P1, Ps, c = step_case(V)
    with torch.no_grad():
        c0 = VO.cost(m, P1, Tv.double(), torch.ones(NB, V, dtype=torch.float64), 1e-6, 1e-6)
    assert np.isfinite(Ps.numpy()).all() and bool((c < c0).all())
    assert bool(((Ps - P1).abs().amax(1) > 1e-3).all())
    assert (VO.rms(m, Ps, Tv).numpy() < VO.rms(m, P1, Tv).numpy()).all()
