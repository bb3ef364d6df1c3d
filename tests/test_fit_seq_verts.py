"""The MANO fit to a track of meshes and of point clouds, the parts that need no GPU: the public header and its binding by
_Lib.bind, the workspace queries, every refusal of the two entry points, the refusals of ManoFitter.fit_vertices_sequence and
fit_points_sequence, the fp64 oracle of tests/_fit_seq_verts_oracle.py against the oracles it composes and against the
header's recurrences, and the orderings on the quality case that the GPU test (tests/test_gpu_fit_seq_verts.py) reproduces."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_plane_oracle as LO  # noqa: E402
import _fit_seq_verts_cases as G  # noqa: E402
import _fit_seq_verts_oracle as QO  # noqa: E402
import _fit_verts_oracle as VO  # noqa: E402
from _fit_cases import JOINT_MAP, host_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ_VERTS_H = os.path.join(ROOT, "include", "scat_mano_fit_seq_verts.h")
PARENTS = sum(p << (4 * i) for i, p in enumerate((0, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)))
ENTRIES = {"scat_mano_fit_seq_verts_ws", "scat_mano_fit_seq_verts", "scat_mano_fit_points_seq_ws", "scat_mano_fit_points_seq"}
S_NAMES = ("s_rots", "s_poses", "s_betas", "s_trans", "s_scale")
WALK, AG = 4 * (63 * 62 + 62 * 62 + 2 * 62), 4 * 2 * 63 * 62      # bytes per frame: the walk's 31,496 and the two A_t, g_t


@pytest.fixture(scope="module")
def built():
    from scat_amd import build

    return build.build(verbose=False)


def test_header_declares_the_four_and_collides_with_no_other():
    from scat_amd import build, fit
    from scat_amd._lib import EXTENSION_HEADERS, HEADERS, parse_header

    assert os.path.samefile(fit.FIT_SEQ_VERTS_HEADER, SEQ_VERTS_H) and "scat_mano_fit_seq_verts.h" in build.PUBLIC_HEADERS
    assert not any(os.path.samefile(h, SEQ_VERTS_H) for h in (*HEADERS, *EXTENSION_HEADERS))
    protos = parse_header(SEQ_VERTS_H)
    assert set(protos) == ENTRIES
    for q, n in (("scat_mano_fit_seq_verts_ws", 3), ("scat_mano_fit_points_seq_ws", 5)):
        assert protos[q][0] is ctypes.c_int64 and [ty for ty, _ in protos[q][1]] == [ctypes.c_int] * n
    for name in ("scat_mano_fit_seq_verts", "scat_mano_fit_points_seq"):
        rt, args = protos[name]
        by = dict((an, ty) for ty, an in args)
        assert rt is ctypes.c_int and args[-1][1] == "stream"
        assert by["ws"] is ctypes.c_void_p and by["ws_bytes"] is ctypes.c_int64 and by["free_mask"] is ctypes.c_uint64
        assert all(by[k] is ctypes.c_int for k in ("S", "T", "V", "iters")) and by["parents"] is ctypes.c_uint64
        assert tuple(an for _, an in args if an.startswith("s_")) == S_NAMES
        assert all(by[k] is ctypes.c_float for k in S_NAMES + ("lambda0", "w_pose", "w_beta", "w_tangent"))
    # scat_mano_fit_points_plane's arguments, in its order, with T and the smoothness let in
    plane = [an for _, an in parse_header(fit.FIT_PLANE_HEADER)["scat_mano_fit_points_plane"][1]]
    mine = [an for _, an in protos["scat_mano_fit_points_seq"][1] if an not in ("T",) + S_NAMES]
    assert mine == ["S" if an == "B" else an for an in plane]
    others = (*HEADERS, *EXTENSION_HEADERS, fit.FIT_VERTS_HEADER, fit.FIT_POINTS_HEADER, fit.FIT_SEQ_KP_HEADER, fit.FIT_PLANE_HEADER)
    assert len(set(os.path.realpath(h) for h in others)) == len(os.listdir(os.path.join(ROOT, "include"))) - 1      # every other header
    for h in others:
        assert not set(protos) & set(parse_header(h)), h
    src = " ".join(open(SEQ_VERTS_H).read().replace(" * ", " ").split())
    for said in ("UNITS", "axis-angle", "LAUNCHES", "2 iters + 2 launches", "WORKSPACE", "62,752 bytes", "WHAT REFUSES A SEQUENCE",
                 "WHAT IS BRIDGED", "NOTHING MATCHED", "every check before any HIP call", "no atomic", "no data-dependent exit",
                 "depend neither on S nor on its index", "weights are all zero", "p is written only after an accepted step",
                 "with the same bits"):
        assert said in src, said
    for fn in (fit.ManoFitter.fit_vertices_sequence, fit.ManoFitter.fit_points_sequence):
        doc = " ".join(fn.__doc__.split())
        assert "bridged" in doc.lower() and "not fitted" in doc, fn
    assert build._public_headers_mtime() >= os.path.getmtime(SEQ_VERTS_H)      # the header is a rebuild trigger


def test_bind_binds_the_header_and_leaves_the_tables(built):
    from scat_amd import _lib
    from scat_amd._lib import EXTENSION_HEADERS, FIT_SEQ_HEADER, HEADERS, lib, parse_header
    from scat_amd.fit import FIT_SEQ_VERTS_HEADER

    L = lib()
    before = (tuple(HEADERS), tuple(EXTENSION_HEADERS), dict(L.by_header), dict(L.by_extension), dict(L.protos))
    ns = L.bind(FIT_SEQ_VERTS_HEADER)
    assert sorted(vars(ns)) == sorted(parse_header(SEQ_VERTS_H)) == sorted(ENTRIES)
    assert L.bind(FIT_SEQ_VERTS_HEADER) is ns and L.bound[FIT_SEQ_VERTS_HEADER] is ns
    assert (tuple(_lib.HEADERS), tuple(_lib.EXTENSION_HEADERS), L.by_header, L.by_extension, L.protos) == before
    assert len(HEADERS) == 7 and EXTENSION_HEADERS == (FIT_SEQ_HEADER,) and list(L.by_header) == list(HEADERS)
    for name in vars(ns):
        assert hasattr(L.cdll, name) and not hasattr(L, name)
    assert ns.scat_mano_fit_seq_verts.__name__ == "scat_mano_fit_seq_verts"      # the checked wrapper


def test_workspace_queries(built):
    from scat_amd._lib import lib
    from scat_amd.fit import FIT_PLANE_HEADER, FIT_POINTS_HEADER, FIT_SEQ_VERTS_HEADER

    L = lib()
    ns = L.bind(FIT_SEQ_VERTS_HEADER)
    q, qp = ns.scat_mano_fit_seq_verts_ws, ns.scat_mano_fit_points_seq_ws
    up16 = lambda n: (n + 15) & ~15
    sizes = [(1, 1), (1, 2), (2, 2), (2, 5), (3, 5), (3, 256), (1024, 16)]
    got = [int(q(S, T, 37)) for S, T in sizes]
    assert got == sorted(got) and len(set(got)) == len(got)
    for (S, T), g in zip(sizes, got):      # the five parts, each rounded up to 16 bytes
        assert g == up16(S * T * WALK) + up16(S * T * AG) + 2 * up16(4 * S * T) + 32 * S, (S, T)
    assert int(q(1, 1, 37)) // 1 >= 62752 and int(q(1024, 16, 778)) == 1024 * (16 * 62752 + 32)      # the header's figures
    assert [int(q(2, 5, V)) for V in (1, 37, 778, 1536)] == [int(q(2, 5, 37))] * 4      # monotone in V: it does not depend on V
    assert int(q((1 << 23) - 1, 256, 37)) == ((1 << 23) - 1) * (256 * 62752 + 32)      # S T = 2^31 - 256: the last S at T = 256
    for S, T, V in ((0, 5, 37), (-1, 5, 37), (2, 0, 37), (2, -1, 37), (2, 257, 37), (2, 5, 0), (2, 5, 1537), (1 << 23, 256, 37)):
        assert int(q(S, T, V)) == 0, (S, T, V)
    # the cloud track: the ICP loops' parts for B = S T hands, then the track's
    pts, pln = L.bind(FIT_POINTS_HEADER).scat_mano_fit_points_ws, L.bind(FIT_PLANE_HEADER).scat_mano_fit_points_plane_ws
    for S, T, N, V, F in ((1, 1, 1, 1, 0), (2, 3, 257, 37, 0), (2, 3, 257, 37, 70), (3, 5, 2048, 778, 1538)):
        want = int(pln(S * T, N, V, F) if F else pts(S * T, N, V)) + int(q(S, T, V))
        assert int(qp(S, T, N, V, F)) == want, (S, T, N, V, F)
    mono = [int(qp(*a)) for a in ((1, 2, 100, 37, 70), (2, 2, 100, 37, 70), (2, 3, 100, 37, 70), (2, 3, 101, 37, 70), (2, 3, 101, 38, 70))]
    assert mono == sorted(mono) and len(set(mono)) == len(mono)
    for a in ((0, 3, 257, 37, 0), (2, 0, 257, 37, 0), (2, 257, 257, 37, 0), (2, 3, 0, 37, 0), (2, 3, 8193, 37, 0), (2, 3, 257, 0, 0),
              (2, 3, 257, 1537, 0), (2, 3, 257, 37, -1), (2, 3, 257, 37, 4097), (1 << 23, 256, 257, 37, 0)):
        assert int(qp(*a)) == 0, a


GOOD = dict(S=2, T=5, V=778, parents=PARENTS, iters=4, init=0, tau=0.01, lambda0=1e-3, w_pose=1e-6, w_beta=1e-6,
            s=[1e-3, 1e-4, 1e-2, 1e-1, 1e-1], free=(1 << 62) - 1, ws=4096, ws_bytes=None)
# blend, joint_t, joint_s, weights_t, hands_mean, targets, weights, normals, p, cost, accepted
V_NPTR, V_OPTIONAL = 11, (6, 7)
# blend, joint_t, joint_s, weights_t, hands_mean, points, weights, faces, vf_off, vf_idx, p, data_cost, accepted, idx, dist
P_NPTR, P_OPTIONAL, P_TOPO = 15, (6, 13, 14), (7, 8, 9)
P_GOOD = dict(GOOD, N=257, F=70, rounds=3, max_dist=0.05)


def _call_verts(ns, **kw):
    a = dict(GOOD, ptrs=[8 * (i + 1) for i in range(V_NPTR)])
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(int(ns.scat_mano_fit_seq_verts_ws(a["S"], a["T"], a["V"])), 16)
    return ns.scat_mano_fit_seq_verts(*a["ptrs"], a["ws"], a["ws_bytes"], a["S"], a["T"], a["V"], a["parents"], a["iters"], a["init"],
                                      a["tau"], a["lambda0"], a["w_pose"], a["w_beta"], *a["s"], a["free"], 0)


def _call_points(ns, **kw):
    a = dict(P_GOOD, ptrs=[8 * (i + 1) for i in range(P_NPTR)])
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = max(int(ns.scat_mano_fit_points_seq_ws(a["S"], a["T"], a["N"], a["V"], a["F"])), 16)
    return ns.scat_mano_fit_points_seq(*a["ptrs"], a["ws"], a["ws_bytes"], a["S"], a["T"], a["N"], a["V"], a["F"], a["parents"],
                                       a["rounds"], a["iters"], a["max_dist"], a["tau"], a["lambda0"], a["w_pose"], a["w_beta"],
                                       *a["s"], a["free"], 0)


def _refuser(L, entry, call, ns):
    label = L.scat_last_kernel()

    def refused(code, pattern, **kw):
        from scat_amd._lib import ScatError

        with pytest.raises(ScatError, match=rf"{entry} failed \({code}\): {entry}: .*{pattern}"):
            call(ns, **kw)
        assert L.scat_last_kernel() == label

    return refused


def _shared_refusals(refused, good):
    from scat_amd import mano

    refused(-1, "batch 0 must be positive", S=0)
    refused(-1, r"0 frames outside 1\.\.256", T=0)
    refused(-1, r"257 frames outside 1\.\.256", T=257)
    refused(-1, r"8388608 sequences of 256 frames are more than 2147483647 frames in all", S=1 << 23, T=256)
    refused(-1, "0 vertices outside", V=0)
    refused(-1, rf"{mano.MAX_V + 1} vertices outside", V=mano.MAX_V + 1)
    refused(-2, r"0 iterations outside 1\.\.64", iters=0)
    refused(-2, r"65 iterations outside 1\.\.64", iters=65)
    refused(-2, "lambda0 0 outside", lambda0=0.0)
    refused(-2, "w_pose -1 must be finite and not negative", w_pose=-1.0)
    refused(-2, "w_beta inf must be finite", w_beta=float("inf"))
    refused(-2, r"w_tangent 1\.5 outside 0\.\.1", tau=1.5)
    refused(-2, r"w_tangent -0\.1 outside 0\.\.1", tau=-0.1)
    for i, name in enumerate(S_NAMES):
        for bad, text in ((-1.0, "-1"), (float("inf"), "inf"), (float("nan"), "nan")):
            s = list(good["s"])
            s[i] = bad
            refused(-2, f"{name} {text} must be finite and not negative", s=s)
    refused(-2, "free_mask has bits above 61 set", free=1 << 62)
    refused(-2, "free_mask has bits above 61 set", free=1 << 63)
    refused(-3, "workspace must be a 16-byte-aligned pointer", ws=0)
    refused(-3, "workspace must be a 16-byte-aligned pointer", ws=4096 + 4)


def test_mesh_track_errors_surface_without_a_gpu(built):
    """argument validation happens before any HIP call: made-up pointers are never followed, each refusal carries its
    SCAT_E_* code and names the entry point, and the kernel label does not move"""
    from scat_amd._lib import lib
    from scat_amd.fit import FIT_SEQ_VERTS_HEADER

    L = lib()
    ns = L.bind(FIT_SEQ_VERTS_HEADER)
    refused = _refuser(L, "scat_mano_fit_seq_verts", _call_verts, ns)
    base = [8 * (i + 1) for i in range(V_NPTR)]
    for i in range(V_NPTR):
        if i not in V_OPTIONAL:
            refused(-2, "null pointer", ptrs=[0 if j == i else v for j, v in enumerate(base)])
        refused(-2, "4-byte aligned", ptrs=base[:i] + [base[i] + 2] + base[i + 1:])
    _shared_refusals(refused, GOOD)
    refused(-2, "init 2 must be 0", init=2)
    refused(-2, "init 1 is the Euclidean fit's", init=1)
    _call_args = dict(ptrs=[0 if j == 7 else v for j, v in enumerate(base)])      # without normals tau is not looked at
    refused(-3, "workspace must be", tau=1.5, ws=0, **_call_args)
    need = int(ns.scat_mano_fit_seq_verts_ws(GOOD["S"], GOOD["T"], GOOD["V"]))
    refused(-3, f"workspace of {need - 1} bytes, {need} needed", ws_bytes=need - 1)


def test_cloud_track_errors_surface_without_a_gpu(built):
    from scat_amd._lib import lib
    from scat_amd.fit import FIT_SEQ_VERTS_HEADER

    L = lib()
    ns = L.bind(FIT_SEQ_VERTS_HEADER)
    refused = _refuser(L, "scat_mano_fit_points_seq", _call_points, ns)
    base = [8 * (i + 1) for i in range(P_NPTR)]
    without = lambda *idx: [0 if j in idx else v for j, v in enumerate(base)]
    for i in range(P_NPTR):
        if i not in P_OPTIONAL:
            refused(-2, "null pointer", ptrs=without(i))      # one of the topology's three without the others too
        refused(-2, "4-byte aligned", ptrs=base[:i] + [base[i] + 2] + base[i + 1:])
    refused(-2, "null pointer", ptrs=without(*P_TOPO))      # F = 70 without a topology
    refused(-1, r"0 faces outside 1\.\.4096", F=0)             # a topology without faces
    refused(-1, r"4097 faces outside 1\.\.4096", F=4097)
    refused(-1, r"0 points outside 1\.\.8192", N=0)
    refused(-1, r"8193 points outside 1\.\.8192", N=8193)
    refused(-2, "max_dist 0 must be positive", max_dist=0.0)
    refused(-2, "max_dist nan must be positive", max_dist=float("nan"))
    refused(-2, r"0 rounds outside 1\.\.64", rounds=0)
    refused(-2, r"65 rounds outside 1\.\.64", rounds=65)
    refused(-2, "64 rounds of 5 iterations are more than 256 steps", rounds=64, iters=5)
    _shared_refusals(refused, P_GOOD)
    for F in (70, 0):
        kw = dict(F=F) if F else dict(F=0, ptrs=without(*P_TOPO))
        need = int(ns.scat_mano_fit_points_seq_ws(2, 5, 257, 778, F))
        assert need > 0
        refused(-3, f"workspace of {need - 1} bytes, {need} needed", ws_bytes=need - 1, **kw)


def test_the_python_surface_refuses_before_the_library():
    from scat_amd._lib import ScatError
    from scat_amd.fit import ManoFitter, PointSequenceFitResult, SequenceFitResult
    from scat_amd.mano import ManoModel

    f = ManoFitter(ManoModel.synthetic(1, V=37), joint_map=JOINT_MAP)
    v, pts, p0 = torch.zeros(2, 3, 37, 3), torch.zeros(2, 3, 50, 3), torch.zeros(2, 3, 62)
    assert PointSequenceFitResult._fields == ("rots", "poses", "betas", "trans", "scale", "data_cost", "accepted", "p", "matched",
                                              "rms", "idx", "dist") and SequenceFitResult._fields[-1] == "p"

    def refused(pattern, fn, *a, **kw):
        with pytest.raises(ScatError, match=pattern):
            fn(*a, **kw)

    fv, fp = f.fit_vertices_sequence, f.fit_points_sequence
    refused("unknown smooth keys", fv, v, smooth=dict(cam=1.0))
    refused(r"smooth\['rots'\] = -1.0 must be finite", fv, v, smooth=dict(rots=-1.0))
    refused("CPU|cpu|GPU|device", fv, v)
    refused("unknown smooth keys", fp, pts, p0, smooth=dict(cam=1.0))
    refused("needs a start", fp, pts, None)
    refused(r"w_tangent 2 outside 0\.\.1", fp, pts, p0, w_tangent=2)
    refused("face indices", fp, pts, p0, faces=np.array([[0, 1, 37]]))
    refused("CPU|cpu|GPU|device", fp, pts, p0)


@pytest.mark.gpu
def test_the_python_surface_refuses_shapes_and_ranges():
    """the refusals that look at tensors on the device, reached before any launch"""
    from scat_amd._lib import ScatError
    from scat_amd.fit import ManoFitter
    from scat_amd.mano import ManoModel

    D = "cuda"
    f = ManoFitter(ManoModel.synthetic(1, V=37).to(D), joint_map=JOINT_MAP)
    v, pts, p0 = torch.zeros(2, 3, 37, 3, device=D), torch.zeros(2, 3, 50, 3, device=D), torch.zeros(2, 3, 62, device=D)

    def refused(pattern, fn, *a, **kw):
        with pytest.raises(ScatError, match=pattern):
            fn(*a, **kw)

    fv, fp = f.fit_vertices_sequence, f.fit_points_sequence
    refused(r"needs fp32 verts \[S,T,37,3\]", fv, v[:, :, :36])
    refused(r"needs fp32 verts \[S,T,37,3\]", fv, v.double())
    refused(r"needs fp32 verts \[S,T,37,3\]", fv, v[0])
    refused(r"needs fp32 weights \[2,3,37\]", fv, v, weights=torch.ones(2, 3, 36, device=D))
    refused(r"needs an fp32 start \[2,3,62\]", fv, v, init=p0[:, :2])
    refused(r"65 iterations outside", fv, v, iters=65)
    refused("free has bits above 61 set", fv, v, free=1 << 62)
    refused(r"needs fp32 points \[S,T,N,3\]", fp, pts[0], p0)
    refused(r"needs fp32 points \[S,T,N,3\]", fp, pts.double(), p0)
    refused(r"needs fp32 weights \[2,3,50\]", fp, pts, p0, weights=torch.ones(2, 3, 49, device=D))
    refused(r"needs an fp32 start \[2,3,62\]", fp, pts, p0[:1])
    refused("rounds outside", fp, pts, p0, rounds=65)
    refused("rounds outside", fp, pts, p0, rounds=64, iters=5)
    refused("max_dist 0 must be positive", fp, pts, p0, max_dist=0)


def test_one_frame_without_smoothness_is_the_frame_oracle():
    """T = 1 and zero smoothness: the track oracle is _fit_verts_oracle.lm, and with normals _fit_plane_oracle.lm; tau = 1
    is the Euclidean one"""
    m, zero = host_model(37), (0.0,) * 5
    X, _, _, P1, _, _ = G.step_case(37, 2, 1, False)
    w = G.ones(2, 1, 37)
    P, c, acc = QO.lm(m, X.double(), w, P1, 4, zero)
    Pv, cv, av = VO.lm(m, X.double()[:, 0], w[:, 0], P1[:, 0], 4)
    assert float((P[:, 0] - Pv).abs().max()) <= 1e-12 and float((c - cv).abs().max()) <= 1e-12 * float(cv.max())
    assert acc.tolist() == av.tolist()
    X, wm, n, P1, _, _ = G.step_case(37, 2, 1, True)
    P, c, acc = QO.lm(m, X.double(), wm.double(), P1, 4, zero, n.double(), G.TAU)
    Pl, cl, al = LO.lm(m, X.double()[:, 0], wm.double()[:, 0], n.double()[:, 0], G.TAU, P1[:, 0], 4)
    assert float((P[:, 0] - Pl).abs().max()) <= 1e-12 and acc.tolist() == al.tolist()
    X3, w3, n3, P3, _, _ = G.step_case(37, 2, 3, True)
    Pa = QO.lm(m, X3.double(), w3.double(), P3, 3, G.sm(G.SMOOTH), n3.double(), 1.0)[0]
    Pb = QO.lm(m, X3.double(), w3.double(), P3, 3, G.sm(G.SMOOTH))[0]
    assert float((Pa - Pb).abs().max()) <= 1e-12
    B = 6
    Y = torch.from_numpy(np.random.default_rng(3).normal(size=(B, 37, 3)))
    ww = torch.from_numpy(np.random.default_rng(4).random((B, 37)))
    assert float((QO.procrustes(m, Y, ww) - VO.procrustes_start(m, Y, ww)).abs().max()) <= 1e-12


def test_the_dense_factor_has_the_headers_blocks():
    """the dense Cholesky factor of the damped block-tridiagonal matrix: L_t on the diagonal, M_t = -D L_t-1^-T below it,
    zeros elsewhere, L_t L_t^T = H_t - M_t M_t^T"""
    m, T, U = host_model(37), 3, 62
    X, w, n, P1, _, _ = G.step_case(37, 2, T, True)
    H, g, _ = QO.normal_equations(m, P1, X.double(), w.double(), n.double(), G.TAU, 1e-6, 1e-6, G.sm(G.SMOOTH))
    Hd = H + 1e-2 * torch.diag_embed(torch.diagonal(H, dim1=1, dim2=2))
    L = torch.linalg.cholesky(Hd)
    D = torch.diag(QO.SO.dvec(G.sm(G.SMOOTH), torch.float64))
    blk = lambda A, i, j: A[:, i * U:(i + 1) * U, j * U:(j + 1) * U]
    for t in range(T):
        for j in range(T):
            if j > t or j < t - 1:
                assert float(blk(L, t, j).abs().max()) == 0.0 if j > t else float(blk(L, t, j).abs().max()) <= 1e-18
        if t > 0:
            M = -D @ torch.linalg.inv(blk(L, t - 1, t - 1)).transpose(1, 2)
            assert float((blk(L, t, t - 1) - M).abs().max()) <= 1e-9 * float(M.abs().max())
            R = blk(Hd, t, t) - M @ M.transpose(1, 2)
            Lt = blk(L, t, t)
            assert float((Lt @ Lt.transpose(1, 2) - R).abs().max()) <= 1e-9 * float(R.abs().max())


def test_the_track_beats_per_frame_icp_on_the_oracle():
    """the quality case on the oracle alone (tools/fit_seq_verts_gates.py prints the table, DESIGN 20 records it): the
    track's acceleration error is below per-frame point-to-plane ICP's, its vertex RMS over the visible frames is no worse,
    and the occluded interior frame ends nearer the truth than the start that per-frame ICP leaves it at"""
    q = G.quality_case()
    vis = [t for t in range(G.QT) if t != G.Q_GAP]
    assert (q["accel", "track"] < 0.5 * q["accel", "frame"]).all(), (q["accel", "track"], q["accel", "frame"])
    assert (q["rms", "track"][:, vis].mean(1) <= q["rms", "frame"][:, vis].mean(1)).all()
    assert np.array_equal(q["rms", "frame"][:, G.Q_GAP], q["rms", "start"][:, G.Q_GAP])      # per-frame ICP leaves it alone
    assert (q["rms", "track"][:, G.Q_GAP] < 0.5 * q["rms", "start"][:, G.Q_GAP]).all()
