"""The MANO fit to a surface point cloud (point-to-plane ICP), the parts that need no GPU: the public header and _Lib.bind,
argument errors of the entry points and of the Python surface, and the fp64 oracle of tests/_fit_plane_oracle.py: its
normals against a loop over python floats, the three routes to a zero normal, the per-vertex metric system against the
per-point system it replaces, the Euclidean limit tau = 1 against _fit_verts_oracle, sqrt(M)^2 = M, the descent of a round,
and the quality assertion on the smooth model that the GPU test gates (tests/test_gpu_fit_plane.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_plane_oracle as LO  # noqa: E402
import _fit_points_oracle as PO  # noqa: E402
import _fit_verts_oracle as VO  # noqa: E402
from _fit_plane_cases import (ITERS, QB, ROUNDS, TAU, TAUS, T_, ZERO_37, assign_case, host_model, metric_case, quality_case,  # noqa: E402
                              quality_inputs, smooth_model, topology)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE_H = os.path.join(ROOT, "include", "scat_mano_fit_plane.h")
PARENTS = sum(p << (4 * i) for i, p in enumerate((0, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)))
LAUNCHING = ("scat_mesh_normals", "scat_mano_fit_verts_metric", "scat_mano_cloud_assign_plane", "scat_mano_fit_points_plane")
ENTRIES = LAUNCHING + ("scat_mano_fit_points_plane_ws",)
NULLABLE = {"scat_mesh_normals": (), "scat_mano_fit_verts_metric": ("weights",),
            "scat_mano_cloud_assign_plane": ("weights", "model_pts"), "scat_mano_fit_points_plane": ("weights", "idx", "dist")}
ALL = (1 << 62) - 1


@pytest.fixture(scope="module")
def built():
    from scat_amd import build

    return build.build(verbose=False)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


# ------------------------------------------------------------------------------------------------ the oracle
def test_oracle_normals_are_the_loop_over_python_floats():
    for V, B in ((1, 2), (37, 3), (778, 1)):
        x = np.random.default_rng(V).normal(size=(B, V, 3)).astype(np.float32)
        n, b = LO.normals(x, *topology(V)), LO.brute_normals(x, *topology(V))
        assert np.array_equal(n, b), V      # the same fp64 operations in the same order
        length = np.linalg.norm(n, axis=2)
        assert (np.abs(length[length > 0] - 1.0) < 1e-15).all()
    r = LO.normals(x, *topology(778), round32=True)
    assert np.array_equal(r, n.astype(np.float32).astype(np.float64)) and np.abs(r - n).max() <= 2.0 ** -24
    # corrupt indices skip the face and are never followed
    f, off, idx = (a.copy() for a in topology(37))
    f[3, 1], idx[10], idx[11] = 37, -1, 70
    x = np.random.default_rng(2).normal(size=(1, 37, 3))
    assert np.array_equal(LO.normals(x, f, off, idx), LO.brute_normals(x, f, off, idx))


def test_zero_normals_by_three_routes():
    """a vertex in no face, one whose only face is degenerate, two whose only faces are coincident with opposite winding:
    exactly zero; every other vertex of topology(37) has a unit normal on generic coordinates.  A mesh that is not finite
    gives zeros where it is summed"""
    x = np.random.default_rng(7).normal(size=(2, 37, 3)).astype(np.float32)
    n = LO.normals(x, *topology(37))
    zero = sorted(v for vs in ZERO_37.values() for v in vs)
    assert (n[:, zero] == 0).all()
    rest = [v for v in range(37) if v not in zero]
    assert (np.abs(np.linalg.norm(n[:, rest], axis=2) - 1.0) < 1e-15).all()
    assert (LO.normals(x[:, :1], *topology(1)) == 0).all()
    x[0, 5, 1] = np.inf
    n = LO.normals(x, *topology(37))
    touched = sorted({int(v) for f in topology(37)[0] if 5 in f for v in f} - {35})
    assert (n[0, touched] == 0).all() and np.isfinite(n).all() and (n[1, rest] != 0).any(1).all()


def test_sqrt_metric_squares_to_the_metric():
    n = T_(LO.normals(np.random.default_rng(3).normal(size=(2, 37, 3)), *topology(37)))
    for tau in (0.0, 0.01, 0.1, 0.5, 1.0):
        S, M = LO.sqrt_metric(n, tau), LO.metric(n, tau)
        assert float((S @ S - M).abs().max()) < 1e-15, tau
        r = torch.from_numpy(np.random.default_rng(4).normal(size=(2, 37, 3)))
        assert float(((r.unsqueeze(-2) @ M @ r.unsqueeze(-1)).reshape(2, 37) - LO.rho(r, n, tau)).abs().max()) < 1e-14
    zero = LO.flat(n)
    assert bool(zero.any()) and bool((LO.metric(n, 0.0)[zero] == torch.eye(3, dtype=torch.float64)).all())
    assert bool((LO.sqrt_metric(n, 0.0)[zero] == torch.eye(3, dtype=torch.float64)).all())


def _assigned(weighted=True):
    """assign_case(3, 257, 37) assigned by the points oracle at the oracle's model points, with their normals"""
    P, points, weights = assign_case(3, 257, 37, weighted)
    m, Pd = host_model(37), T_(P).double()
    with torch.no_grad():
        x = VO.model_verts(m, Pd).numpy()
    a = PO.assign(x, points, weights, 0.01)
    assert 0 < a["matched"].sum() < (a["idx"] >= 0).sum()
    return m, Pd, x, points, np.ones(points.shape[:2], np.float32) if weights is None else weights, a, LO.normals(x, *topology(37))


@pytest.mark.parametrize("tau", TAUS + (0.1,))
def test_per_vertex_metric_system_is_the_per_point_system(tau):
    """A and g of the per-vertex form (W_v, qbar_v, sqrt(M_v) on the rows) against one row triple per matched point with
    M between them, to 1e-12; the costs differ by the constant of the identity, which does not depend on P"""
    m, P, x, points, weights, a, n = _assigned()
    vt, vw, nt = torch.from_numpy(a["vtarget"]), torch.from_numpy(a["vw"]), torch.from_numpy(n)
    A, g, c = LO.normal_equations(m, P, vt, vw, nt, tau, 1e-6, 1e-6, ALL)
    Ap, gp, cp = LO.point_normal_equations(m, P, points, weights, a["idx"], a["matched"], nt, tau, 1e-6, 1e-6)
    assert rel(A, Ap) <= 1e-12 and rel(g, gp) <= 1e-12, (rel(A, Ap), rel(g, gp))
    P2 = P.clone()
    P2[:, :58] += 0.01
    c2 = LO.normal_equations(m, P2, vt, vw, nt, tau, 1e-6, 1e-6, ALL)[2]
    cp2 = LO.point_normal_equations(m, P2, points, weights, a["idx"], a["matched"], nt, tau, 1e-6, 1e-6)[2]
    const = cp - c
    assert bool((const >= 0).all()) and rel(cp2 - c2, const) <= 1e-9
    # the header's expression of the data cost is the per-point cost without the priors
    dc = LO.assign_cost(x, points, weights, a["idx"], a["matched"], n, tau)
    assert rel(dc, (cp - LO.priors(P, 1e-6, 1e-6)).numpy()) <= 1e-12


def test_tau_one_is_the_euclidean_fit():
    m, P, x, points, weights, a, n = _assigned()
    vt, vw, nt = torch.from_numpy(a["vtarget"]), torch.from_numpy(a["vw"]), torch.from_numpy(n)
    free = ALL & ~(7 << 48)
    A, g, c = LO.normal_equations(m, P, vt, vw, nt, 1.0, 1e-6, 2e-6, free)
    Ae, ge, ce = VO.normal_equations(m, P, vt, vw, 1e-6, 2e-6, free)
    assert rel(A, Ae) <= 1e-12 and rel(g, ge) <= 1e-12 and rel(c, ce) <= 1e-12
    assert rel(LO.assign_cost(x, points, weights, a["idx"], a["matched"], n, 1.0), a["stats"][:, 3]) <= 1e-12
    Tv, w, nn, P1 = metric_case(37)
    got, want = LO.lm(m, Tv.double(), w.double(), nn.double(), 1.0, P1, 3), VO.lm(m, Tv.double(), w.double(), P1, 3)
    assert rel(got[0], want[0]) <= 1e-12 and torch.equal(got[2], want[2])


@pytest.mark.parametrize("tau", (0.0, TAU))
def test_a_round_never_raises_the_metric_cost(tau):
    """without a trim, with the correspondences and normals of a round's start held fixed, the per-point metric cost
    after the round's Levenberg-Marquardt is not above the cost before it, in every round and on every hand: a step is
    accepted only if the per-vertex cost drops, and the two differ by a constant.  (The next assignment picks new
    vertices by Euclidean distance and new normals, which the metric cost is not bound by.)"""
    m, topo = smooth_model(), topology(778)
    _, mesh, pts, P0 = quality_inputs()
    Ps = LO.icp(m, pts, None, P0, topo, 4, ITERS, tau, history=True)[4]
    for r in range(4):
        with torch.no_grad():
            x0, x1 = VO.model_verts(m, Ps[r]).numpy(), VO.model_verts(m, Ps[r + 1]).numpy()
        a = PO.assign(x0, pts, None)
        n = LO.normals(x0, *topo)
        before = LO.assign_cost(x0, pts, None, a["idx"], a["matched"], n, tau) + LO.priors(Ps[r], 1e-6, 1e-6).numpy()
        after = LO.assign_cost(x1, pts, None, a["idx"], a["matched"], n, tau) + LO.priors(Ps[r + 1], 1e-6, 1e-6).numpy()
        assert (after <= before).all(), (r, before, after)
        assert r > 0 or (after < before).all()


def test_point_to_plane_beats_nearest_vertex_on_a_surface_cloud():
    """the quality assertion of _fit_plane_cases.quality_case, on the oracle alone: after ROUNDS x ITERS from the same
    start every hand's vertex RMS is below nearest-vertex ICP's, at the default tau and at 0"""
    for tau in (TAU, 0.0):
        r0, rn, rp, _ = quality_case(tau)
        print(f"tau {tau}: vertex RMS in mm, start {(1e3 * r0).round(3)}, nearest vertex {(1e3 * rn).round(3)}, point-to-plane "
              f"{(1e3 * rp).round(3)} after {ROUNDS} x {ITERS}")
        assert rp.shape == (QB,) and (rp < rn).all() and (rn < r0).all()


# ------------------------------------------------------------------------------------------------ header and bind
def test_header_declares_the_five_entry_points():
    from scat_amd import build, fit
    from scat_amd._lib import EXTENSION_HEADERS, HEADERS, parse_header

    assert os.path.samefile(fit.FIT_PLANE_HEADER, PLANE_H) and "scat_mano_fit_plane.h" in build.PUBLIC_HEADERS
    assert not any(os.path.samefile(h, PLANE_H) for h in (*HEADERS, *EXTENSION_HEADERS))
    protos = parse_header(PLANE_H)
    assert set(protos) == set(ENTRIES)
    for name in LAUNCHING:
        rt, args = protos[name]
        by = dict((an, ty) for ty, an in args)
        assert rt is ctypes.c_int and args[-1][1] == "stream", name
        assert by["B"] is ctypes.c_int and by["V"] is ctypes.c_int
        if name != "scat_mano_fit_verts_metric":
            assert by["F"] is ctypes.c_int and all(by[k] is ctypes.c_void_p for k in ("faces", "vf_off", "vf_idx"))
        if name != "scat_mesh_normals":
            assert by["w_tangent"] is ctypes.c_float and by["parents"] is ctypes.c_uint64 and "init" not in by
    assert protos["scat_mano_fit_points_plane_ws"][0] is ctypes.c_int64
    assert [ty for ty, _ in protos["scat_mano_fit_points_plane_ws"][1]] == [ctypes.c_int] * 4
    by = dict((an, ty) for ty, an in protos["scat_mano_fit_verts_metric"][1])
    assert by["normals"] is ctypes.c_void_p and "F" not in by
    for h in (*HEADERS, *EXTENSION_HEADERS, fit.FIT_VERTS_HEADER, fit.FIT_POINTS_HEADER):
        assert not set(protos) & set(parse_header(h)), h
    src = " ".join(open(PLANE_H).read().split()).replace(" * ", " ")
    for said in ("UNITS", "THE NORMALS", "THE METRIC", "NOT RENORMALISED", "rounded to fp32 once", "is skipped, never followed",
                 "a I + (1 - a) n_v n_v^T", "before any HIP call", "2 rounds + 1 launches", "bits of scat_mano_cloud_assign"):
        assert said in src, said
    assert build._public_headers_mtime() >= os.path.getmtime(PLANE_H)      # the header is a rebuild trigger


def test_bind_binds_the_header_and_leaves_the_tables(built):
    from scat_amd import _lib
    from scat_amd._lib import EXTENSION_HEADERS, HEADERS, ScatError, lib, parse_header
    from scat_amd.fit import FIT_PLANE_HEADER

    L = lib()
    before = (tuple(HEADERS), tuple(EXTENSION_HEADERS), dict(L.by_header), dict(L.by_extension), dict(L.protos))
    ns = L.bind(FIT_PLANE_HEADER)
    assert sorted(vars(ns)) == sorted(ENTRIES) and L.bind(FIT_PLANE_HEADER) is ns
    assert (tuple(_lib.HEADERS), tuple(_lib.EXTENSION_HEADERS), L.by_header, L.by_extension, L.protos) == before
    for name in ENTRIES:
        assert hasattr(L.cdll, name) and not hasattr(L, name)
        assert len(getattr(L.cdll, name).argtypes) == len(parse_header(FIT_PLANE_HEADER)[name][1])
    with pytest.raises(ScatError, match=r"scat_mesh_normals failed \(-2\): scat_mesh_normals: null pointer"):
        ns.scat_mesh_normals(0, 0, 0, 0, 0, 1, 1, 1, 0)


def test_workspace_query(built):
    from scat_amd._lib import lib
    from scat_amd.fit import FIT_PLANE_HEADER, FIT_POINTS_HEADER
    from scat_amd.mano import MAX_V

    q = lib().bind(FIT_PLANE_HEADER).scat_mano_fit_points_plane_ws
    base = lib().bind(FIT_POINTS_HEADER).scat_mano_fit_points_ws
    r16 = lambda n: (n + 15) // 16 * 16
    for B, N, V, F in ((1, 1, 1, 1), (3, 37, 37, 70), (3, 257, 37, 70), (65, 300, 778, 1538), (65, 8192, 1536, 4096)):
        assert int(q(B, N, V, F)) == int(base(B, N, V)) + r16(12 * B * V)      # the points loop's parts, then the normals
    for bad in ((0, 37, 37, 70), (3, 0, 37, 70), (3, 8193, 37, 70), (3, 37, 0, 70), (3, 37, MAX_V + 1, 70), (3, 37, 37, 0),
                (3, 37, 37, 4097)):
        assert int(q(*bad)) == 0, bad


GOOD = dict(B=3, N=37, V=37, F=70, parents=PARENTS, max_dist=0.03, w_tangent=0.01, rounds=5, iters=4, lambda0=1e-3, w_pose=1e-6,
            w_beta=1e-6, free_mask=ALL, ws=4096, stream=0)


def _call(ns, entry, **kw):
    """the entry point on made-up pointers 8, 16, 24, ... in the order of its pointer arguments (kw: by argument name)"""
    from scat_amd._lib import parse_header

    a = dict(GOOD)
    args = parse_header(PLANE_H)[entry][1]
    ptrs = [an for ty, an in args if ty is ctypes.c_void_p and an not in ("stream", "ws")]
    a.update({an: 8 * (i + 1) for i, an in enumerate(ptrs)})
    a.update(kw)
    a.setdefault("ws_bytes", max(int(ns.scat_mano_fit_points_plane_ws(a["B"], a["N"], a["V"], a["F"])), 16))
    return getattr(ns, entry)(*(a[an] for _, an in args)), ptrs


@pytest.mark.parametrize("entry", LAUNCHING)
def test_errors_surface_without_a_gpu(built, entry):
    """argument validation happens before any HIP call: made-up pointers are never followed, each refusal carries its
    SCAT_E_* code and names the entry point, and the kernel label does not move"""
    from scat_amd import mano
    from scat_amd._lib import ScatError, lib, parse_header
    from scat_amd.fit import FIT_PLANE_HEADER

    L = lib()
    ns = L.bind(FIT_PLANE_HEADER)
    label = L.scat_last_kernel()

    def refused(code, pattern, **kw):
        with pytest.raises(ScatError, match=rf"{entry} failed \({code}\): {entry}: .*{pattern}"):
            _call(ns, entry, **kw)
        assert L.scat_last_kernel() == label

    ptrs = [an for ty, an in parse_header(PLANE_H)[entry][1] if ty is ctypes.c_void_p and an not in ("stream", "ws")]
    assert set(NULLABLE[entry]) <= set(ptrs)
    for i, an in enumerate(ptrs):
        if an not in NULLABLE[entry]:
            refused(-2, "null pointer", **{an: 0})
        refused(-2, "4-byte aligned", **{an: 8 * (i + 1) + 2})
    refused(-1, "batch 0 must be positive", B=0)
    refused(-1, "0 vertices outside", V=0)
    refused(-1, rf"{mano.MAX_V + 1} vertices outside 1\.\.{mano.MAX_V}", V=mano.MAX_V + 1)
    if entry != "scat_mano_fit_verts_metric":
        refused(-1, r"0 faces outside 1\.\.4096", F=0)
        refused(-1, r"4097 faces outside 1\.\.4096", F=4097)
    if entry != "scat_mesh_normals":
        refused(-2, r"w_tangent -0\.01 outside 0\.\.1", w_tangent=-0.01)
        refused(-2, r"w_tangent 1\.5 outside 0\.\.1", w_tangent=1.5)
        refused(-2, r"w_tangent nan outside 0\.\.1", w_tangent=float("nan"))
        refused(-2, r"parent\[3\] = 7", parents=(PARENTS & ~(15 << 12)) | (7 << 12))
    if entry in ("scat_mano_cloud_assign_plane", "scat_mano_fit_points_plane"):
        refused(-1, r"8193 points outside 1\.\.8192", N=8193)
        refused(-2, "max_dist 0 must be positive", max_dist=0.0)
    if "stats" in ptrs:
        refused(-2, "stats must be 8-byte aligned", stats=8 * (ptrs.index("stats") + 1) + 4)
    if entry in ("scat_mano_fit_verts_metric", "scat_mano_fit_points_plane"):
        refused(-2, r"65 iterations outside 1\.\.64", iters=65)
        refused(-2, "lambda0 0 outside", lambda0=0.0)
        refused(-2, "free_mask has bits above 61 set", free_mask=1 << 62)
    if entry == "scat_mano_fit_points_plane":
        refused(-2, r"65 rounds outside 1\.\.64", rounds=65)
        refused(-2, "64 rounds of 5 iterations are more than 256 steps", rounds=64, iters=5)
        need = int(ns.scat_mano_fit_points_plane_ws(GOOD["B"], GOOD["N"], GOOD["V"], GOOD["F"]))
        refused(-3, "workspace must be a 16-byte-aligned pointer", ws=0)
        refused(-3, "workspace must be a 16-byte-aligned pointer", ws=4096 + 8)
        refused(-3, f"workspace of {need - 1} bytes, {need} needed", ws_bytes=need - 1)


# ------------------------------------------------------------------------------------------------ the Python surface
def test_python_surface_refuses_before_any_launch(built):
    """what the methods check on the host comes before the look at the tensors, so it shows without a GPU: a missing start,
    w_tangent outside [0, 1], faces that are no [F,3] integers, that name a vertex >= V or that are too many, a renderer
    of another V; then CPU tensors, as everywhere on the product path"""
    from scat_amd._lib import ScatError
    from scat_amd.fit import MAX_F, ManoFitter
    from scat_amd.render import MeshRenderer

    f = ManoFitter(host_model(37))
    faces = topology(37)[0]
    pts, p0 = torch.zeros(2, 5, 3), torch.zeros(2, 62)
    with pytest.raises(ScatError, match="needs a start"):
        f.fit_points_plane(pts, None, faces)
    for tau in (-0.1, 1.01, float("nan")):
        with pytest.raises(ScatError, match=r"w_tangent .* outside 0\.\.1"):
            f.fit_points_plane(pts, p0, faces, w_tangent=tau)
    bad = faces.copy()
    bad[4, 2] = 37
    for method in (lambda fc: f.fit_points_plane(pts, p0, fc), lambda fc: f.vertex_normals(torch.zeros(2, 37, 3), fc)):
        with pytest.raises(ScatError, match=r"face indices 0\.\.37 outside 0\.\.36"):
            method(bad)
        with pytest.raises(ScatError, match=r"face indices -1\.\.\d+ outside 0\.\.36"):
            method(torch.from_numpy(np.where(bad == 37, -1, bad)))
        with pytest.raises(ScatError, match="integer indices needed"):
            method(faces.astype(np.float32))
        with pytest.raises(ScatError, match="shape"):
            method(faces[:, :2])
        with pytest.raises(ScatError, match=rf"{MAX_F + 1} faces outside 1\.\.{MAX_F}"):
            method(np.zeros((MAX_F + 1, 3), np.int32))
        with pytest.raises(ScatError, match="the renderer has 778 vertices, the model 37"):
            method(MeshRenderer(topology(778)[0], 778))
        with pytest.raises(ScatError, match="needs GPU tensors"):
            method(faces)
    assert len(f._topologies) == 1 and f._topologies[id(faces)][0] is faces      # checked once, kept by the object
    with pytest.raises(ScatError, match="needs a fit result"):
        f.vertex_normals(torch.zeros(2, 62), faces)
