"""On-device evaluation, the parts that need no GPU: the second public header and its binding, argument errors of both
entry points, the fp64 oracle of tests/_eval_oracle.py pinned to the reference's own outputs (tests/golden/metrics.npz),
and evaluator.finalize on hand-made tables."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_oracle as EO  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL_H = os.path.join(ROOT, "include", "scat_eval.h")


@pytest.fixture(scope="module")
def built():
    from scat_amd import build

    return build.build(verbose=False)


def test_eval_header_is_bound_beside_the_main_one(built):
    from scat_amd._lib import lib, parse_header

    protos = parse_header(EVAL_H)
    assert set(protos) == {"scat_eval_frame_mask", "scat_eval_frame_mask_ws", "scat_eval_accumulate",
                           "scat_eval_accumulate_ws"}
    L = lib()
    for name, (rt, args) in protos.items():
        assert hasattr(L.cdll, name), name
        assert callable(getattr(L, name)), name
        if rt is ctypes.c_int:
            assert args[-1][1] == "stream", name
    # the default parse is still the main header alone: none of the evaluation names, nothing lost
    main = parse_header()
    assert not set(main) & set(protos)
    assert len(main) == 91 and {"scat_loss_fwd_bwd", "scat_augment_plan", "scat_version"} <= set(main)
    assert set(L.protos) == set(main) | set(protos)
    src = open(EVAL_H).read()
    assert src.count("eval.py:") >= 8      # every entry point cites the reference lines it stands in for


def test_eval_errors_surface_without_a_gpu(built):
    """argument validation of both entry points happens before any HIP call"""
    from scat_amd._lib import ScatError, lib

    L = lib()
    T, B = 7, 4
    ws = L.scat_eval_accumulate_ws(B, T)
    assert ws >= B * (32 + 2 * T) and L.scat_eval_accumulate_ws(B, 0) == 0
    good = dict(out=8, gt3d=8, gt2d=8, ld=105, keep=0, th=8, T=T, record=16, per=0, al=0, B=B, ws=16, ws_bytes=ws)

    def acc(**kw):
        a = dict(good, **kw)
        return L.scat_eval_accumulate(a["out"], a["gt3d"], a["gt2d"], a["ld"], a["keep"], a["th"], a["T"], a["record"],
                                      a["per"], a["al"], a["B"], a["ws"], a["ws_bytes"], 0)

    for k in ("out", "gt3d", "gt2d", "th", "record", "ws"):
        with pytest.raises(ScatError, match=r"\(-2\).*null pointer"):
            acc(**{k: 0})
    for t in (0, 65):
        with pytest.raises(ScatError, match=r"\(-1\).*outside 1\.\.64"):
            acc(T=t)
    with pytest.raises(ScatError, match=r"\(-1\).*must be positive"):
        acc(B=0)
    with pytest.raises(ScatError, match=r"\(-1\).*ld_gt"):
        acc(ld=62)
    with pytest.raises(ScatError, match=r"\(-2\).*8-byte aligned"):
        acc(record=12)
    with pytest.raises(ScatError, match=r"\(-2\).*8-byte aligned"):
        acc(per=20)
    with pytest.raises(ScatError, match=r"\(-2\).*4-byte aligned"):
        acc(out=10)
    with pytest.raises(ScatError, match=r"\(-3\).*workspace"):
        acc(ws_bytes=ws - 1)

    n = 150528
    fws = L.scat_eval_frame_mask_ws(B, n)
    assert fws >= 8 * B
    with pytest.raises(ScatError, match=r"\(-2\).*null pointer"):
        L.scat_eval_frame_mask(0, 8, B, n, 150528.0, 2000.0, 16, fws, 0)
    with pytest.raises(ScatError, match=r"\(-2\).*null pointer"):
        L.scat_eval_frame_mask(8, 0, B, n, 150528.0, 2000.0, 16, fws, 0)
    with pytest.raises(ScatError, match=r"\(-1\).*must be positive"):
        L.scat_eval_frame_mask(8, 8, 0, n, 150528.0, 2000.0, 16, fws, 0)
    with pytest.raises(ScatError, match=r"\(-1\).*row length"):
        L.scat_eval_frame_mask(8, 8, B, 0, 150528.0, 2000.0, 16, fws, 0)
    with pytest.raises(ScatError, match=r"\(-2\).*4-byte aligned"):
        L.scat_eval_frame_mask(10, 8, B, n, 150528.0, 2000.0, 16, fws, 0)
    with pytest.raises(ScatError, match=r"\(-3\).*workspace"):
        L.scat_eval_frame_mask(8, 8, B, n, 150528.0, 2000.0, 16, fws - 1, 0)


def test_eval_ops_have_no_cpu_fallback():
    import torch

    from scat_amd import ops
    from scat_amd._lib import ScatError
    from scat_amd.evaluator import Evaluator

    with pytest.raises(ScatError, match="no CPU fallback"):
        ops.eval_frame_mask(torch.zeros(2, 3, 8, 8))
    with pytest.raises(ScatError, match="no CPU fallback"):
        ops.eval_accumulate(torch.zeros(2, 66), torch.zeros(2, 105), [20.0, 30.0])
    with pytest.raises(ScatError, match="no CPU fallback"):
        Evaluator(torch.nn.Identity()).update(torch.zeros(2, 3, 224, 224), torch.zeros(2, 105))


def test_oracle_reproduces_the_reference(golden):
    """the oracle on the seeded joints of tests/golden/metrics.npz against the reference's own functions, with the gates
    tests/test_metrics.py holds scat_amd.metrics to"""
    from tests.test_metrics import metric_inputs

    g = golden("metrics")
    pred, gt = metric_inputs()
    B = pred.shape[0]
    out = np.concatenate([np.zeros((B, 3), np.float32), pred.reshape(B, 63)], axis=1)
    rec, per, al, samples = EO.batch(out, gt, np.zeros((B, 42), np.float32), g["rnge"])
    rel = lambda a, b: float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / np.abs(b).max())
    assert rec[0] == B and rec[1] == B and rec[2] == 0 and rec[3] == 0
    assert rel(al, g["pa_aligned"]) < 2e-5
    assert rel(rec[4] / B, g["mpjpe_mm"]) < 2e-6
    assert rel(rec[5] / B, g["pa_mpjpe_mm"]) < 1e-4
    f = EO.finalize(rec[None, :], g["rnge"])
    assert np.abs(f["pck"] - g["pck"]).max() < 1e-4
    assert np.abs(f["pck_pa"] - g["pck_pa"]).max() < 1e-4
    assert abs(f["auc"] - float(g["auc"])) < 1e-4
    assert rel(per[:, 0], 1000.0 * g["mpjpe_per_sample"].astype(np.float64)) < 2e-6


def _row(n_in, kept, skipped, degenerate, sums, cnt_raw, cnt_pa):
    return np.array([n_in, kept, skipped, degenerate, *sums, 0.0, *cnt_raw, *cnt_pa], dtype=np.float64)


def test_finalize_on_hand_made_tables():
    from scat_amd.evaluator import area_under_curve, finalize

    th = np.array([20.0, 30.0, 50.0])
    # batch 0 keeps 4 frames (84 joints), batch 1 keeps 1 (21 joints), batch 2 keeps none
    t = np.stack([_row(4, 4, 0, 0, (40.0, 8.0, 12.0), (21, 42, 84), (42, 84, 84)),
                  _row(4, 1, 2, 1, (30.0, 6.0, 5.0), (21, 21, 21), (21, 21, 21)),
                  _row(4, 0, 4, 0, (0.0, 0.0, 0.0), (0, 0, 0), (0, 0, 0))])
    r = finalize(t, th)
    assert (r["batches"], r["frames"], r["frames_kept"], r["frames_skipped"], r["frames_degenerate"]) == (3, 12, 5, 6, 1)
    assert r["batches_empty"] == 1
    assert r["mpjpe_mm"] == 70.0 / 5 and r["pa_mpjpe_mm"] == 14.0 / 5 and r["err2d_px"] == 17.0 / 5
    # the reference's PCK: mean of the per-batch percentages (25, 50, 100) and (100, 100, 100), the empty batch left out
    assert np.allclose(r["pck"], [62.5, 75.0, 100.0], rtol=0, atol=1e-12)
    # pooled: 42, 63 and 105 of 105 joints
    assert np.allclose(r["pck_pooled"], [40.0, 60.0, 100.0], rtol=0, atol=1e-12)
    assert np.abs(r["pck"] - r["pck_pooled"]).max() > 2.0
    assert np.allclose(r["pck_pa"], [75.0, 100.0, 100.0], atol=1e-12)
    assert np.allclose(r["pck_pa_pooled"], [100.0 * 63 / 105, 100.0, 100.0], atol=1e-12)
    # AUC by hand: trapezoids over x = (0.4, 0.6, 1.0), divided by the width 0.6
    want = (0.2 * (62.5 + 75.0) / 2 + 0.4 * (75.0 + 100.0) / 2) / 0.6
    assert abs(r["auc"] - want) < 1e-12
    # ... and invariant to the normalisation of the abscissa (eval.py:1029 divides by rnge.max())
    assert abs(area_under_curve(th, r["pck"]) - r["auc"]) < 1e-12
    assert abs(area_under_curve(th / 7.0, r["pck"]) - r["auc"]) < 1e-12
    # the independent oracle agrees on every field
    o = EO.finalize(t, th)
    for k, v in o.items():
        assert np.allclose(r[k], v, rtol=1e-14, atol=0), k
    # equal batches: both averages coincide
    t2 = np.stack([t[0], t[0]])
    r2 = finalize(t2, th)
    assert np.array_equal(r2["pck"], r2["pck_pooled"]) and r2["batches_empty"] == 0
    # nothing kept at all: counts, and NaN rather than a division error
    r3 = finalize(t[2:], th)
    assert r3["frames_kept"] == 0 and r3["batches_empty"] == 1 and np.isnan(r3["mpjpe_mm"]) and np.isnan(r3["pck"]).all()
    with pytest.raises(ValueError):
        finalize(t, th[:2])


def test_oracle_frame_mask_keeps_sample_zero():
    x = np.ones((3, 8), dtype=np.float32)
    x[2, 0] = -20.0
    assert EO.frame_mask(x, 8.0, 2.0).tolist() == [1, 0, 1]
