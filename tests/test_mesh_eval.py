"""On-device mesh scoring, the parts that need no GPU: the public header and its binding, argument errors, the fp64 oracle
of tests/_mesh_eval_oracle.py pinned by hand-made clouds, mesh_evaluator.finalize_mesh on hand-made tables, and the
conditions that the inputs of tests/test_gpu_mesh_eval.py have to meet, asserted here on the oracle alone so that no
failure on the GPU can be blamed on the data."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_eval_cases as C  # noqa: E402
import _mesh_eval_oracle as MO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH_H = os.path.join(ROOT, "include", "scat_mesh_eval.h")
ENTRY = "scat_mesh_eval_accumulate"


@pytest.fixture(scope="module")
def built():
    from scat_amd import build

    return build.build(verbose=False)


def test_mesh_eval_header_is_bound(built):
    from scat_amd import build
    from scat_amd._lib import EVAL_HEADER, HEADER, HEADERS, MESH_EVAL_HEADER, lib, parse_header

    assert os.path.samefile(MESH_EVAL_HEADER, MESH_H)
    assert HEADERS[0] == HEADER and HEADERS[1] == MESH_EVAL_HEADER and HEADERS[2] == EVAL_HEADER
    protos = parse_header(MESH_H)
    assert set(protos) == {ENTRY}
    L = lib()
    rt, args = protos[ENTRY]
    assert hasattr(L.cdll, ENTRY) and callable(getattr(L, ENTRY)) and rt is ctypes.c_int
    names = [an for _, an in args]
    assert names == ["pred", "gt", "V", "keep", "thresholds_mm", "T", "f_thresholds_mm", "F", "record", "per_sample", "aligned",
                     "B", "stream"]
    assert names[-1] == "stream" and "ws" not in names and "ws_bytes" not in names
    assert L.by_header[MESH_EVAL_HEADER] == protos and list(L.by_header) == list(HEADERS) and not set(protos) & set(L.protos)
    for h in HEADERS:
        if not os.path.samefile(h, MESH_H):
            assert not set(protos) & set(parse_header(h)), h
    assert not any(n.endswith("_ws") for n in protos)
    assert build._public_headers_mtime() >= os.path.getmtime(MESH_H)      # the header is a rebuild trigger
    assert "scat_mesh_eval.h" in open(build.__file__).read()
    src = open(MESH_H).read()
    assert "2 n_pred n_gt / (V (n_pred + n_gt))" in src and "strict <" in src      # the header states the F-score rule


def test_mesh_eval_errors_surface_without_a_gpu(built):
    """argument validation happens before any HIP call: made-up pointers are never followed"""
    from scat_amd._lib import ScatError, lib

    L = lib()
    label = L.scat_last_kernel()
    good = dict(pred=8, gt=8, V=778, keep=0, th=8, T=100, fth=8, F=2, record=16, per=16, al=0, B=4)

    def refused(code, pattern, **kw):
        a = dict(good, **kw)
        with pytest.raises(ScatError, match=rf"{ENTRY} failed \({code}\): {ENTRY}: .*{pattern}"):
            L.scat_mesh_eval_accumulate(a["pred"], a["gt"], a["V"], a["keep"], a["th"], a["T"], a["fth"], a["F"], a["record"],
                                        a["per"], a["al"], a["B"], 0)
        assert L.scat_last_kernel() == label

    for k in ("pred", "gt", "th", "fth", "record", "per"):
        refused(-2, "null pointer", **{k: 0})
    for v in (0, 1025):
        refused(-1, rf"{v} vertices outside 1\.\.1024", V=v)
    for t in (0, 129):
        refused(-1, rf"{t} thresholds outside 1\.\.128", T=t)
    for f in (0, 9):
        refused(-1, rf"{f} F-score thresholds outside 1\.\.8", F=f)
    refused(-1, "batch 0 must be positive", B=0)
    refused(-1, "batch -3 must be positive", B=-3)
    refused(-2, "8-byte aligned", record=12)
    refused(-2, "8-byte aligned", per=20)
    for k in ("pred", "gt", "th", "fth", "al"):
        refused(-2, "4-byte aligned", **{k: 10})


def test_mesh_eval_has_no_cpu_fallback():
    import torch

    from scat_amd import ops
    from scat_amd._lib import ScatError
    from scat_amd.mesh_evaluator import MeshEvaluator

    assert ops.MESH_EVAL_RECORD_HEAD == MO.HEAD == 8 and ops.MESH_EVAL_SAMPLE_HEAD == MO.ROW_HEAD == 4
    with pytest.raises(ScatError, match="no CPU fallback"):
        ops.mesh_eval_accumulate(torch.zeros(2, 5, 3), torch.zeros(2, 5, 3), [20.0, 30.0])
    ev = MeshEvaluator()
    assert ev.thresholds.shape == (100,) and ev.thresholds[0] == 0 and ev.thresholds[-1] == 50
    assert ev.f_thresholds.tolist() == [5.0, 15.0] and ev.max_batches == 4096
    with pytest.raises(ScatError, match="no CPU fallback"):
        ev.update(torch.zeros(2, 5, 3), torch.zeros(2, 5, 3))
    with pytest.raises(ScatError, match="no CPU fallback"):
        ev.update_params(None, torch.zeros(2, 61), torch.zeros(2, 61))
    with pytest.raises(ValueError):
        MeshEvaluator(thresholds_mm=np.arange(129))
    with pytest.raises(ValueError):
        MeshEvaluator(f_thresholds_mm=np.arange(9))
    r = ev.result()      # nothing scored yet: counts of zero, NaN scores, no device touched
    assert r["batches"] == 0 and r["frames_kept"] == 0 and np.isnan(r["mpvpe_mm"]) and np.isnan(r["f_score"]).all()


# ---------------------------------------------------------------- the oracle, pinned by clouds scored by hand

SQUARE = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], dtype=np.float32)      # metres


def test_oracle_on_a_shifted_unit_square():
    """pred = the unit square moved by 3 mm in x, 4 mm in y: every vertex is 5 mm from its own and a metre from the rest"""
    g = SQUARE
    p = (SQUARE.astype(np.float64) + np.array([0.003, 0.004, 0.0])).astype(np.float32)
    s = MO.sample(p, g)
    assert not s["degenerate"] and not s["tie"]
    # (fp32 inputs near 1 m carry 6e-8 m = 6e-5 mm of rounding each)
    assert np.allclose(s["d_raw"], 5.0, atol=1e-3) and abs(s["mpvpe"] - 5.0) < 1e-3
    assert s["pa"] < 1e-3 and np.abs(s["aligned"] - g).max() < 1e-6      # a translation is aligned away
    assert all(np.array_equal(a, np.arange(4)) for a in s["arg_raw"])
    row = MO.scores(s, [4.0, 6.0], [4.0, 6.0])
    # flag, mpvpe, pa, 0 | cnt_raw | cnt_pa | raw (n_pred, n_gt, F) x 2 | aligned (n_pred, n_gt, F) x 2
    assert row[0] == 0 and row[3] == 0
    assert row[4:8].tolist() == [0, 4, 4, 4]
    assert row[8:].tolist() == [0, 0, 0, 4, 4, 1, 4, 4, 1, 4, 4, 1]
    # the counts of the two directions part when two pred points share one gt neighbour and a gt point is left alone
    p2 = SQUARE.astype(np.float64).copy()
    p2[1] = [0.002, 0.0, 0.0]        # corner 1 now sits 2 mm from gt corner 0
    s2 = MO.sample(p2.astype(np.float32), g)
    dq, dg = s2["nn_raw"]
    assert np.allclose(dq, [0, 2, 0, 0], atol=1e-3) and np.allclose(dg, [0, 998, 0, 0], atol=1e-3)
    assert s2["arg_raw"][0].tolist() == [0, 0, 2, 3] and s2["arg_raw"][1].tolist() == [0, 1, 2, 3]
    r2 = MO.scores(s2, [1.0], [5.0])
    assert r2[6:9].tolist() == [4, 3, 2.0 * 4 * 3 / (4 * 7)]      # n_pred 4, n_gt 3: precision 1, recall 3/4
    # the comparison is strict: a distance equal to the threshold does not count, for PCK it does
    p3 = SQUARE.astype(np.float64).copy()
    p3[:, 2] = 0.25                   # exactly representable: every distance is exactly 250 mm
    r3 = MO.scores(MO.sample(p3.astype(np.float32), g), [250.0], [250.0, 250.5])
    assert r3[4] == 4 and r3[6:12].tolist() == [0, 0, 0, 4, 4, 1]


def test_oracle_on_equal_far_and_mirrored_clouds():
    g = C.inputs(37, 6)[1][0]
    th, fth = [5.0, 20.0], [5.0, 15.0]
    s = MO.sample(g, g)
    row = MO.scores(s, th, fth)
    assert row[1] == 0 and row[2] < 1e-9 and row[4:8].tolist() == [37] * 4
    assert row[8:].reshape(4, 3).tolist() == [[37, 37, 1]] * 4
    # 10 m away: nothing within reach raw, everything after the alignment (fp32 near 10 m: 5e-4 mm of rounding each)
    far = (g.astype(np.float64) + 10.0).astype(np.float32)
    s = MO.sample(far, g)
    row = MO.scores(s, th, fth)
    assert abs(row[1] - 1000.0 * np.sqrt(300.0)) < 1e-2 and row[4:6].tolist() == [0, 0]
    assert row[8:14].tolist() == [0, 0, 0, 0, 0, 0]
    assert row[2] < 2e-3 and row[6:8].tolist() == [37, 37] and row[14:].reshape(2, 3).tolist() == [[37, 37, 1]] * 2
    # a mirrored cloud is aligned by a proper rotation only: the error stays, the reflection would have removed it
    mir = (g * np.array([-1.0, 1.0, 1.0], dtype=np.float32))
    s = MO.sample(mir, g)
    assert s["pa"] > 1.0 and s["ratio"] > C.MIN_RATIO
    X1, X2 = mir.astype(np.float64) - mir.mean(0), g.astype(np.float64) - g.mean(0)
    A = s["aligned"] - s["aligned"].mean(0)
    M = np.linalg.lstsq(X1, A, rcond=None)[0].T      # aligned = M pred + t: M = scale R
    assert np.linalg.det(M) > 0
    assert np.allclose(M @ M.T, np.eye(3) * (np.linalg.det(M) ** (2 / 3)), atol=1e-9)
    # and it is the best proper similarity: a small turn away from it does worse
    e0 = np.linalg.norm(A - X2)
    for ax in range(3):
        ang = [0.0, 0.0, 0.0]
        ang[ax] = 1e-3
        assert np.linalg.norm(A @ C.rot(*ang).T - X2) > e0
    # degenerate: a non-finite input, a cloud of one point
    bad = g.copy()
    bad[5, 1] = np.nan
    assert MO.sample(bad, g)["degenerate"] and MO.sample(g, bad)["degenerate"]
    assert MO.sample(np.tile(g[:1], (37, 1)), g)["degenerate"]


# ---------------------------------------------------------------- finalize_mesh

def _row(n_in, kept, skipped, degenerate, sums, V, cnt_raw, cnt_pa, f_raw, f_pa):
    return np.array([n_in, kept, skipped, degenerate, *sums, V, 0.0, *cnt_raw, *cnt_pa, *f_raw, *f_pa], dtype=np.float64)


def test_finalize_mesh_on_hand_made_tables():
    from scat_amd.evaluator import area_under_curve
    from scat_amd.mesh_evaluator import finalize_mesh

    th, fth = np.array([10.0, 30.0, 50.0]), np.array([5.0, 15.0])
    # V = 10; batch 0 keeps 4 frames (40 vertices), batch 1 keeps 1 (10 vertices), batch 2 keeps none
    t = np.stack([_row(4, 4, 0, 0, (40.0, 8.0), 10, (10, 20, 40), (20, 40, 40), (2.0, 3.0), (3.0, 4.0)),
                  _row(4, 1, 2, 1, (30.0, 6.0), 10, (10, 10, 10), (10, 10, 10), (0.5, 1.0), (1.0, 1.0)),
                  _row(4, 0, 4, 0, (0.0, 0.0), 10, (0, 0, 0), (0, 0, 0), (0.0, 0.0), (0.0, 0.0))])
    r = finalize_mesh(t, th, fth)
    assert (r["batches"], r["frames"], r["frames_kept"], r["frames_skipped"], r["frames_degenerate"]) == (3, 12, 5, 6, 1)
    assert r["vertices"] == 10
    assert r["mpvpe_mm"] == 70.0 / 5 and r["pa_mpvpe_mm"] == 14.0 / 5
    # pooled: 20, 30 and 50 of 50 vertices
    assert np.allclose(r["pck_v"], [40.0, 60.0, 100.0], rtol=0, atol=1e-12)
    assert np.allclose(r["pck_v_pa"], [60.0, 100.0, 100.0], rtol=0, atol=1e-12)
    assert np.allclose(r["f_score"], [0.5, 0.8], rtol=0, atol=1e-15) and np.allclose(r["f_score_pa"], [0.8, 1.0], rtol=0, atol=1e-15)
    # AUC by hand: trapezoids over x = (0.2, 0.6, 1.0), divided by the width 0.8
    want = (0.4 * (40.0 + 60.0) / 2 + 0.4 * (60.0 + 100.0) / 2) / 0.8
    assert abs(r["auc_v"] - want) < 1e-12 and abs(area_under_curve(th, r["pck_v"]) - want) < 1e-12
    assert abs(r["auc_v_pa"] - (0.4 * 80.0 + 0.4 * 100.0) / 0.8) < 1e-12
    assert np.array_equal(r["thresholds_mm"], th) and np.array_equal(r["f_thresholds_mm"], fth)
    # the independent oracle agrees on every field
    o = MO.finalize(t, th, fth)
    for k, v in o.items():
        assert np.allclose(r[k], v, rtol=1e-14, atol=0), k
    # nothing kept at all, and no row at all: counts, and NaN rather than a division error
    for tab, nb in ((t[2:], 1), (np.zeros((0, t.shape[1])), 0)):
        e = finalize_mesh(tab, th, fth)
        assert e["batches"] == nb and e["frames_kept"] == 0 and np.isnan(e["mpvpe_mm"]) and np.isnan(e["pa_mpvpe_mm"])
        assert np.isnan(e["pck_v"]).all() and np.isnan(e["f_score_pa"]).all() and e["pck_v"].shape == (3,)
    # rows of another vertex count do not pool; rows of another width are not this table
    t2 = t.copy()
    t2[1, 6] = 12
    with pytest.raises(ValueError, match="vertex counts"):
        finalize_mesh(t2, th, fth)
    with pytest.raises(ValueError, match="do not match"):
        finalize_mesh(t, th[:2], fth)
    with pytest.raises(ValueError, match="do not match"):
        finalize_mesh(t, th, fth[:1])


# ---------------------------------------------------------------- conditions on the inputs of the GPU tests

@pytest.mark.parametrize("V,B,tset", C.CASES)
def test_gpu_inputs_meet_their_conditions(V, B, tset):
    """From the oracle alone.  Measured with SEED = 7300: smallest margin 1.6e-5 mm (V = 65, B = 65), smallest ratio 0.027;
    at V = 778 the nearest neighbour is another vertex than the own one for 63-100 % of the vertices; no ties."""
    th, fth = C.THRESHOLDS[tset]
    S = C.samples(V, B)
    if V == 1:
        assert all(s["degenerate"] for s in S)      # a single point has no spread: every sample is degenerate
        return
    assert not any(s["degenerate"] for s in S)
    margin, ratio = MO.margins(S, th, fth)
    assert margin >= C.MIN_MARGIN_MM, f"a distance lies {margin:.3e} mm from a threshold"
    assert ratio >= C.MIN_RATIO, f"rotation nearly not unique: ratio {ratio:.3e}"
    assert not any(s["tie"] for s in S), "two candidates at equal minimal distance"
    per = C.oracle(V, B, tset)[1]
    f = per[:, MO.ROW_HEAD + 2 * th.size:].reshape(B, 2, fth.size, 3)
    assert (f[..., 0] != f[..., 1]).any(), "n_pred == n_gt everywhere: a swapped direction would pass"
    if V == 778:
        own = np.arange(V)
        for b, s in enumerate(S):
            if B >= 6 and b == 3:      # pred == gt: every vertex is its own neighbour
                assert all((a == own).all() for a in s["arg_raw"])
                continue
            for side in ("arg_raw", "arg_pa"):
                for a in s[side]:
                    assert (a != own).mean() >= 0.25, (b, side)      # scoring correspondences instead would fail
    if B >= 6:      # what the special samples are there for
        assert per[3, 1] == 0.0 and (f[3, :, :, 2] == 1.0).all()                      # pred == gt
        assert (f[4, 0, fth <= 30.0, :] == 0).all() and per[4, 1] > 1.7e4             # 10 m away: nothing raw ...
        assert (f[4, 1, fth >= 15.0, 2] > 0.5).all()                                  # ... and a mesh again once aligned
        assert per[2, 2] > 5.0                                                        # mirrored: stays wrong
