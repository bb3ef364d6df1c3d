"""The MANO fit to a point cloud, the parts that need no GPU: the public header and _Lib.bind, argument errors of the three
launching entry points and the workspace query, the refusal of CPU tensors, and the fp64 oracle of
tests/_fit_points_oracle.py: the per-vertex reduction against the per-point normal equations, its assignment against a
double loop, and the ICP's behaviour on the fixed cases that the GPU tests gate (tests/test_gpu_fit_points.py), which
shows those inputs fit for the gates."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_points_oracle as PO  # noqa: E402
import _fit_verts_oracle as VO  # noqa: E402
from _fit_points_cases import (ITERS, NB, ROUNDS, TRIM, assign_case, cloud, deliberate_case, host_model, icp_case,  # noqa: E402
                               start)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS_H = os.path.join(ROOT, "include", "scat_mano_fit_points.h")
PARENTS = sum(p << (4 * i) for i, p in enumerate((0, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)))
LAUNCHING = ("scat_cloud_assign", "scat_mano_cloud_assign", "scat_mano_fit_points")
ENTRIES = LAUNCHING + ("scat_mano_fit_points_ws",)
NULLABLE = {"scat_cloud_assign": ("weights",), "scat_mano_cloud_assign": ("weights", "model_pts"),
            "scat_mano_fit_points": ("weights", "idx", "dist")}


@pytest.fixture(scope="module")
def built():
    from scat_amd import build

    return build.build(verbose=False)


def test_header_declares_the_four_entry_points():
    from scat_amd import build, fit
    from scat_amd._lib import EXTENSION_HEADERS, HEADERS, parse_header

    assert os.path.samefile(fit.FIT_POINTS_HEADER, POINTS_H)
    assert "scat_mano_fit_points.h" in build.PUBLIC_HEADERS
    assert not any(os.path.samefile(h, POINTS_H) for h in (*HEADERS, *EXTENSION_HEADERS))
    protos = parse_header(POINTS_H)
    assert set(protos) == set(ENTRIES)
    for name in LAUNCHING:
        rt, args = protos[name]
        by = dict((an, ty) for ty, an in args)
        assert rt is ctypes.c_int and args[-1][1] == "stream", name
        assert by["max_dist"] is ctypes.c_float and all(by[k] is ctypes.c_int for k in ("B", "N", "V"))
        assert all(by[k] is ctypes.c_void_p for k in ("points", "weights")) and not any(n.startswith("tip") for n in by)
    assert protos["scat_mano_fit_points_ws"][0] is ctypes.c_int64
    assert [ty for ty, _ in protos["scat_mano_fit_points_ws"][1]] == [ctypes.c_int] * 3
    by = dict((an, ty) for ty, an in protos["scat_mano_fit_points"][1])
    assert by["ws"] is ctypes.c_void_p and by["ws_bytes"] is ctypes.c_int64 and by["free_mask"] is ctypes.c_uint64
    assert by["rounds"] is ctypes.c_int and by["iters"] is ctypes.c_int and by["parents"] is ctypes.c_uint64
    assert all(by[k] is ctypes.c_float for k in ("lambda0", "w_pose", "w_beta")) and "init" not in by
    assert "parents" not in dict((an, ty) for ty, an in protos["scat_cloud_assign"][1])
    for h in (*HEADERS, *EXTENSION_HEADERS, fit.FIT_VERTS_HEADER):
        assert not set(protos) & set(parse_header(h)), h
    src = " ".join(open(POINTS_H).read().split())
    for said in ("UNITS", "MATCHED iff", "lowest index wins", "NaN vw row", "n ascending", "same call gives the same bits",
                 "carries NO priors", "no floating-point atomic", "before any HIP call"):
        assert said in src.replace(" * ", " "), said
    assert build._public_headers_mtime() >= os.path.getmtime(POINTS_H)      # the header is a rebuild trigger


def test_bind_binds_the_header_and_leaves_the_tables(built):
    from scat_amd import _lib
    from scat_amd._lib import EXTENSION_HEADERS, FIT_SEQ_HEADER, HEADERS, ScatError, lib, parse_header
    from scat_amd.fit import FIT_POINTS_HEADER

    L = lib()
    before = (tuple(HEADERS), tuple(EXTENSION_HEADERS), dict(L.by_header), dict(L.by_extension), dict(L.protos))
    ns = L.bind(FIT_POINTS_HEADER)
    assert sorted(vars(ns)) == sorted(ENTRIES)
    assert L.bind(FIT_POINTS_HEADER) is ns and L.bound[FIT_POINTS_HEADER] is ns
    assert (tuple(_lib.HEADERS), tuple(_lib.EXTENSION_HEADERS), L.by_header, L.by_extension, L.protos) == before
    assert len(HEADERS) == 7 and EXTENSION_HEADERS == (FIT_SEQ_HEADER,) and list(L.by_header) == list(HEADERS)
    for name in ENTRIES:
        fn = getattr(ns, name)
        assert hasattr(L.cdll, name) and not hasattr(L, name)
        assert len(getattr(L.cdll, name).argtypes) == len(parse_header(FIT_POINTS_HEADER)[name][1])
        assert name == "scat_mano_fit_points_ws" or fn.__name__ == name      # the checked wrapper on the int returns
    with pytest.raises(ScatError, match=r"scat_cloud_assign failed \(-2\): scat_cloud_assign: null pointer"):
        ns.scat_cloud_assign(0, 0, 0, 1.0, 0, 0, 0, 0, 0, 1, 1, 1, 0)


def test_workspace_query(built):
    from scat_amd._lib import lib
    from scat_amd.fit import FIT_POINTS_HEADER
    from scat_amd.mano import MAX_V

    q = lib().bind(FIT_POINTS_HEADER).scat_mano_fit_points_ws
    sizes = [(1, 1, 1), (1, 37, 37), (3, 37, 37), (3, 257, 37), (3, 257, 778), (65, 300, 778), (65, 8192, 1536)]
    got = [int(q(*s)) for s in sizes]
    assert all(g > 0 and g % 16 == 0 for g in got) and got == sorted(got) and len(set(got)) == len(got)
    # stats, vtarget, vw, cost, accepted, idx, dist, each rounded up to 16 bytes
    r16 = lambda n: (n + 15) // 16 * 16
    for (B, N, V), g in zip(sizes, got):
        assert g == r16(32 * B) + r16(12 * B * V) + r16(4 * B * V) + 2 * r16(4 * B) + 2 * r16(4 * B * N)
    for bad in ((0, 37, 37), (3, 0, 37), (3, 8193, 37), (3, 37, 0), (3, 37, MAX_V + 1), (-1, 37, 37)):
        assert int(q(*bad)) == 0, bad


GOOD = dict(B=3, N=37, V=37, parents=PARENTS, max_dist=0.03, rounds=5, iters=4, lambda0=1e-3, w_pose=1e-6, w_beta=1e-6,
            free_mask=(1 << 62) - 1, ws=4096, stream=0)


def _call(ns, entry, **kw):
    """the entry point on made-up pointers 8, 16, 24, ... in the order of its pointer arguments (kw: by argument name)"""
    from scat_amd._lib import parse_header

    a = dict(GOOD)
    args = parse_header(POINTS_H)[entry][1]
    ptrs = [an for ty, an in args if ty is ctypes.c_void_p and an not in ("stream", "ws")]
    a.update({an: 8 * (i + 1) for i, an in enumerate(ptrs)})
    a.update(kw)
    a.setdefault("ws_bytes", max(int(ns.scat_mano_fit_points_ws(a["B"], a["N"], a["V"])), 16))
    return getattr(ns, entry)(*(a[an] for _, an in args)), ptrs


def _with_parent(i, p):
    return (PARENTS & ~(15 << (4 * i))) | (p << (4 * i))


@pytest.mark.parametrize("entry", LAUNCHING)
def test_errors_surface_without_a_gpu(built, entry):
    """argument validation happens before any HIP call: made-up pointers are never followed, each refusal carries its
    SCAT_E_* code and names the entry point, and the kernel label does not move"""
    from scat_amd import mano
    from scat_amd._lib import ScatError, lib, parse_header
    from scat_amd.fit import FIT_POINTS_HEADER

    L = lib()
    ns = L.bind(FIT_POINTS_HEADER)
    label = L.scat_last_kernel()

    def refused(code, pattern, **kw):
        with pytest.raises(ScatError, match=rf"{entry} failed \({code}\): {entry}: .*{pattern}"):
            _call(ns, entry, **kw)
        assert L.scat_last_kernel() == label

    ptrs = [an for ty, an in parse_header(POINTS_H)[entry][1] if ty is ctypes.c_void_p and an not in ("stream", "ws")]
    assert set(NULLABLE[entry]) < set(ptrs)
    for i, an in enumerate(ptrs):
        if an not in NULLABLE[entry]:
            refused(-2, "null pointer", **{an: 0})
        refused(-2, "4-byte aligned", **{an: 8 * (i + 1) + 2})
    if "stats" in ptrs:
        refused(-2, "stats must be 8-byte aligned", stats=8 * (ptrs.index("stats") + 1) + 4)
    refused(-1, "batch 0 must be positive", B=0)
    refused(-1, "batch -3 must be positive", B=-3)
    refused(-1, r"0 points outside 1\.\.8192", N=0)
    refused(-1, r"8193 points outside 1\.\.8192", N=8193)
    refused(-1, "0 vertices outside", V=0)
    refused(-1, rf"{mano.MAX_V + 1} vertices outside 1\.\.{mano.MAX_V}", V=mano.MAX_V + 1)
    refused(-2, "max_dist 0 must be positive", max_dist=0.0)
    refused(-2, "max_dist -0.5 must be positive", max_dist=-0.5)
    refused(-2, "max_dist nan must be positive", max_dist=float("nan"))
    if entry != "scat_cloud_assign":
        for i, p in ((1, 1), (3, 7), (15, 15)):
            refused(-2, rf"parent\[{i}\] = {p}", parents=_with_parent(i, p))
        refused(-2, r"parent\[0\] = 5", parents=_with_parent(0, 5))
    if entry == "scat_mano_fit_points":
        refused(-2, r"0 rounds outside 1\.\.64", rounds=0)
        refused(-2, r"65 rounds outside 1\.\.64", rounds=65)
        refused(-2, r"0 iterations outside 1\.\.64", iters=0)
        refused(-2, r"65 iterations outside 1\.\.64", iters=65)
        refused(-2, "64 rounds of 5 iterations are more than 256 steps", rounds=64, iters=5)
        refused(-2, "5 rounds of 52 iterations are more than 256 steps", iters=52)
        refused(-2, "lambda0 0 outside", lambda0=0.0)
        refused(-2, "lambda0 nan outside", lambda0=float("nan"))
        refused(-2, "w_pose -1 must be finite and not negative", w_pose=-1.0)
        refused(-2, "w_beta inf must be finite", w_beta=float("inf"))
        refused(-2, "free_mask has bits above 61 set", free_mask=1 << 62)
        need = int(ns.scat_mano_fit_points_ws(GOOD["B"], GOOD["N"], GOOD["V"]))
        refused(-3, "workspace must be a 16-byte-aligned pointer", ws=0)
        refused(-3, "workspace must be a 16-byte-aligned pointer", ws=4096 + 8)
        refused(-3, f"workspace of {need - 1} bytes, {need} needed", ws_bytes=need - 1)


def test_the_exact_workspace_and_the_largest_sizes_pass_validation(built):
    """the other side of the refusals: what is legal gets as far as the launch, which a box without a device refuses"""
    from scat_amd._lib import ScatError, lib
    from scat_amd.fit import FIT_POINTS_HEADER

    if torch.cuda.is_available():
        pytest.skip("a device is visible: a call that passes validation would launch on the made-up pointers")
    ns = lib().bind(FIT_POINTS_HEADER)
    for entry, kw in (("scat_mano_fit_points", {}), ("scat_mano_fit_points", dict(rounds=64, iters=4, N=8192, V=1536)),
                      ("scat_mano_fit_points", dict(weights=0, idx=0, dist=0, max_dist=float("inf"))),
                      ("scat_mano_cloud_assign", dict(weights=0, model_pts=0)), ("scat_cloud_assign", dict(weights=0, N=8192))):
        with pytest.raises(ScatError, match=rf"{entry} failed \(-4\): {entry}: launch failed"):
            _call(ns, entry, **kw)


def test_fit_points_has_no_cpu_fallback():
    from scat_amd._lib import ScatError
    from scat_amd.fit import ManoFitter

    f = ManoFitter(host_model(37))
    with pytest.raises(ScatError):
        f.fit_points(torch.zeros(2, 5, 3), init=torch.zeros(2, 62))
    with pytest.raises(ScatError):
        f.nearest_vertices(torch.zeros(2, 37, 3), torch.zeros(2, 5, 3))
    with pytest.raises(ScatError, match="needs a start"):
        f.fit_points(torch.zeros(2, 5, 3), init=None)


def test_oracle_assign_agrees_with_a_double_loop():
    """(N, V) = (37, 37), weights with zeros, and planted on dyadic coordinates: two identical vertices, a point at
    exactly max_dist = 2^-7 from its vertex and one at the next fp32 above.  Both sides are IEEE fp64 in the same
    order, so everything but the data cost (another order of one sum: 1e-12) is equal exactly"""
    verts, points, weights, _, _ = assign_case(3, 37, 37, True)
    verts, points, weights = verts.copy(), points.copy(), weights.copy()
    md = 2.0 ** -7
    verts[0, 5] = verts[0, 4]
    points[0, 1], weights[0, 1] = verts[0, 4] + np.float32(1e-3), 1.0
    verts[1, 0] = 1.0
    points[1, 1], points[1, 2] = (1 + md, 1, 1), (np.nextafter(np.float32(1 + md), np.float32(2)), 1, 1)
    weights[1, 1:3] = 1.0
    got = PO.assign(verts, points, weights, md)
    idx, dist, vw, vt, stats = PO.brute_assign(verts, points, weights, md)
    assert got["idx"][0, 1] == 4 and got["idx"][1, 1] == 0 and got["idx"][1, 2] == 0
    assert got["matched"][1, 1] and not got["matched"][1, 2] and got["dist"][1, 1] == md
    assert (got["idx"] == idx).all() and (got["dist"] == dist).all()
    assert np.array_equal(got["vw"], vw) and np.array_equal(got["vtarget"], vt)
    assert (got["stats"][:, :3] == stats[:, :3]).all() and VO.rel(got["stats"][:, 3], stats[:, 3]) < 1e-12
    assert 0 < got["matched"].sum() < (got["idx"] >= 0).sum() < 3 * 37


def test_oracle_deliberate_batch():
    verts, points, md, want = deliberate_case()      # asserts its ties and its trim boundary itself
    idx, dist, vw, vt, stats = PO.brute_assign(verts, points, None, md)
    assert (want["idx"] == idx).all() and (want["dist"] == dist).all() and np.array_equal(want["vw"], vw, equal_nan=True)


def test_oracle_unusable_hands():
    verts, points, weights, md, _ = assign_case(3, 37, 37, True)
    for what in ("nan point", "inf point", "negative weight", "nan weight", "nan vertex"):
        v, q, w = verts.copy(), points.copy(), weights.copy()
        if what == "nan point":
            q[1, 3, 1] = np.nan
        elif what == "inf point":
            q[1, 36, 2] = np.inf
        elif what == "negative weight":
            w[1, 0] = -1.0
        elif what == "nan weight":
            w[1, 5] = np.nan
        else:
            v[1, 7, 0] = np.nan
        a, ref = PO.assign(v, q, w, md), PO.assign(verts[[0, 2]], points[[0, 2]], weights[[0, 2]], md)
        assert a["stats"][1].tolist() == [2.0, 0.0, 0.0, np.inf] and (a["idx"][1] == -1).all() and (a["dist"][1] == 0).all(), what
        assert np.isnan(a["vw"][1]).all() and (a["vtarget"][1] == 0).all(), what
        for k in ("idx", "dist", "vw", "vtarget", "stats"):
            assert np.array_equal(a[k][[0, 2]], ref[k], equal_nan=True), (what, k)


def test_per_vertex_system_is_the_per_point_system():
    """rows J_c(n) with residual model_c(n) - q_n, one triple per matched point, against
    _fit_verts_oracle.normal_equations on (vtarget, vw): A and g to 1e-12 relative, and the costs apart by exactly the
    within-cluster scatter sum_n w_n |q_n - qbar_c(n)|^2"""
    V, wp, wb = 37, 1e-6, 1e-6
    m, P = host_model(V), start(V).double()
    q = np.concatenate([cloud(V, "shuffled"), cloud(V, "shuffled")[:, ::-1] + np.float32(2e-3)], axis=1)      # two points a vertex
    rng = np.random.default_rng(5)
    w = rng.uniform(0.5, 1.5, size=q.shape[:2]).astype(np.float32)
    w[:, ::9] = 0.0
    with torch.no_grad():
        a = PO.assign(VO.model_verts(m, P).numpy(), q, w, 0.05)
    assert 0 < a["matched"].sum() < (w > 0).sum() and (np.bincount(a["idx"][0][a["matched"][0]]) > 1).any()
    A, g, c = PO.point_normal_equations(m, P, q, w, a["idx"], a["matched"], wp, wb)
    Av, gv, cv = VO.normal_equations(m, P, torch.from_numpy(a["vtarget"]), torch.from_numpy(a["vw"]), wp, wb, (1 << 62) - 1)
    eA, eg = VO.rel(Av.numpy(), A.numpy()), VO.rel(gv.numpy(), g.numpy())
    scatter = np.array([(w[b].astype(np.float64) * ((q[b].astype(np.float64) - a["vtarget"][b][a["idx"][b]]) ** 2).sum(1))
                        [a["matched"][b]].sum() for b in range(NB)])
    ec = VO.rel(c.numpy() - cv.numpy(), scatter)
    print(f"A {eA:.3e}, g {eg:.3e}, cost difference against the scatter {ec:.3e} (scatter {scatter})")
    assert eA < 1e-12 and eg < 1e-12 and (scatter > 0).all()
    # the difference of two costs of 1e-3 carries their rounding: 1e-16 x 1e-3 against a scatter of 1e-4
    assert ec < 1e-10


@pytest.mark.parametrize("V", (37, 778))
def test_oracle_icp_descends(V):
    """max_dist = inf.  What the two half-steps guarantee is that data cost + priors never rises: the assignment lowers the
    data cost at fixed p, an accepted step lowers data cost + priors at fixed correspondences.  The data cost alone may rise
    by what the priors gain and no more; on these hands that is 1e-8 relative, at convergence, where the data cost
    (1e-8) is far below the priors (1e-5).  Lower at the end than at the start, for every hand."""
    _, _, _, costs, _, Ps = icp_case(V, "shuffled", None)
    prior = (1e-6 * (Ps[:, :, 3:58] ** 2).sum(2)).numpy()
    total = costs + prior
    rise = ((costs[1:] - costs[:-1]) / costs[:-1]).max()
    print(f"V {V}: data cost {costs[0]} -> {costs[-1]}; largest relative rise of the data cost alone {rise:.3e}")
    assert (total[1:] <= total[:-1]).all()
    assert (costs[-1] < costs[0]).all() and rise < 1e-6


def test_oracle_recovers_what_the_gpu_gates_assume():
    """recoverable: the oracle's final vertex RMS < 1e-4 m after 12 x 4 from the joints-fit start.  Asserted here so that
    a changed fixture cannot hide a failure behind an empty gate."""
    for V, kind, md, least in ((37, "shuffled", None, 6), (37, "shuffled", TRIM, 6), (778, "shuffled", None, 5),
                               (778, "shuffled", TRIM, 5), (778, "half", None, 5)):
        Pf, r0, rf, costs, rec, _ = icp_case(V, kind, md)
        print(f"V {V} {kind} max_dist {md}: start {(1e3 * r0).round(2)} mm, after {ROUNDS} x {ITERS} {(1e3 * rf).round(4)} mm, "
              f"recoverable {int(rec.sum())} of {NB}")
        assert rec.sum() >= least and np.isfinite(Pf.numpy()).all()
        assert (rf[rec] < 1e-2 * r0[rec]).all()
