"""On-device evaluation on a real MI355X (include/scat_eval.h, scat_amd/evaluator.py) against the fp64 numpy oracle of
tests/_eval_oracle.py, against the reference's own outputs in tests/golden/metrics.npz, and inside guard bands."""
import functools
import os
import random
import sys

import numpy as np
import pytest
import torch

from scat_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_oracle as EO  # noqa: E402
from _guard import Arena  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
HEAD = EO.HEAD
BATCHES = (1, 2, 63, 64, 65, 96, 257)     # wavefront (64) and workgroup (4 samples) edges, more than one workgroup
THRESHOLDS = {"reference": np.arange(20, 51, 5.0), "golden": np.arange(20, 51, 1.0), "max": np.linspace(1, 64, 64)}
MIN_MARGIN_MM = 1e-6      # every distance at least this far from every threshold: a count can not hinge on rounding
MIN_RATIO = 1e-3          # (sigma2 + sign(det K) sigma3) / sigma1: the optimal proper rotation is unique

T_ = lambda a: torch.from_numpy(np.array(a))      # a copy: the shared inputs are read-only


@pytest.fixture(scope="module")
def ops():
    from scat_amd import ops as o
    from scat_amd._lib import lib

    lib().scat_check_device()
    return o


def _rot(a, b, c):
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return rz @ ry @ rx


@functools.lru_cache(maxsize=None)
def inputs(B):
    """out [B,66], labels [B,105] fp32: gt ~ N(0, 0.05 m); pred = rotation (three angles) x scale in [0.7, 1.4] x gt +
    shift + N(0, 6 mm); from B = 5 on sample 1 is planar, 2 mirrored in x, 3 equal to gt, 4 shifted by 10 m"""
    seed = 4100 + B
    gt = synth.normal_like(seed, "gt", (B, 21, 3), 0.05).astype(np.float64)
    ang = synth.uniform(seed, "angles", (B, 3), -np.pi, np.pi)
    scale = synth.uniform(seed, "scale", (B,), 0.7, 1.4)
    shift = synth.uniform(seed, "shift", (B, 1, 3), -0.03, 0.03)
    noise = synth.normal_like(seed, "noise", (B, 21, 3), 0.006)
    pred = np.stack([scale[b] * gt[b] @ _rot(*ang[b]).T for b in range(B)]) + shift + noise
    if B >= 5:
        gt[1, :, 2] = 0.0
        pred[1, :, 2] = 0.0
        pred[2] = gt[2] * np.array([-1.0, 1.0, 1.0]) + noise[2]
        pred[3] = gt[3]
        pred[4] += 10.0
    cam = np.concatenate([synth.uniform(seed, "cam_s", (B, 1), 3.0, 7.0), synth.uniform(seed, "cam_t", (B, 2), -0.1, 0.1)], 1)
    out = np.concatenate([cam, pred.reshape(B, 63)], axis=1).astype(np.float32)
    gt2d = synth.uniform(seed, "gt2d", (B, 42), 0.0, 224.0)
    labels = np.concatenate([gt.reshape(B, 63), gt2d], axis=1).astype(np.float32)
    if B >= 5:
        assert np.array_equal(out[3, 3:], labels[3, :63])
    out.setflags(write=False)
    labels.setflags(write=False)
    return out, labels


@functools.lru_cache(maxsize=None)
def oracle(B, tset):
    out, labels = inputs(B)
    return EO.batch(out, labels[:, :63], labels[:, 63:], THRESHOLDS[tset])


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def run(ops, out, labels, th, keep=None):
    rec, per, al = ops.eval_accumulate(T_(out).to(DEV), T_(labels).to(DEV), T_(np.asarray(th, dtype=np.float32)).to(DEV),
                                       keep=None if keep is None else T_(keep).to(DEV), want_per_sample=True,
                                       want_aligned=True)
    return rec.cpu().numpy(), per.cpu().numpy(), al.cpu().numpy()


@pytest.mark.parametrize("tset", list(THRESHOLDS))
@pytest.mark.parametrize("B", BATCHES)
def test_accumulate_matches_the_oracle(ops, B, tset):
    """Counts and frame counts are equal; sums, per-sample scores and aligned joints within 1e-6 norm-wise relative (both
    sides are fp64 on identical fp32 inputs, so the true distance is rounding: 1e-6 is the tightest non-exact gate the
    project uses).  Measured worst over the 21 cases on an MI355X: sums 6.8e-16, per-sample scores 5.4e-15, aligned joints
    4.6e-8 (they are returned as fp32: that is their rounding); smallest margin 1.4e-4 mm, smallest ratio 0.169."""
    th = THRESHOLDS[tset]
    T = th.size
    out, labels = inputs(B)
    rec_o, per_o, al_o, samples = oracle(B, tset)
    # conditions on the inputs, from the oracle alone
    margin, ratio = EO.margins(samples, th)
    assert margin >= MIN_MARGIN_MM, f"a distance lies {margin:.3e} mm from a threshold"
    assert ratio >= MIN_RATIO, f"rotation nearly not unique: ratio {ratio:.3e}"
    assert rec_o[1] == B and rec_o[3] == 0
    rec, per, al = run(ops, out, labels, th)
    assert rec.shape == (HEAD + 2 * T,)
    assert np.array_equal(rec[:4], rec_o[:4]) and rec[7] == 0.0
    assert np.array_equal(rec[HEAD:], rec_o[HEAD:])
    e_sum = max(abs(rec[c] - rec_o[c]) / abs(rec_o[c]) for c in (4, 5, 6))
    e_per = max(rel(per[:, c], per_o[:, c]) for c in range(3))
    e_al = rel(al, al_o)
    print(f"B {B} {tset}: margin {margin:.3e} mm ratio {ratio:.3f} sums {e_sum:.3e} per_sample {e_per:.3e} aligned {e_al:.3e}")
    assert np.array_equal(per[:, 3], per_o[:, 3])
    assert e_sum < 1e-6 and e_per < 1e-6
    assert e_al < 1e-6      # aligned is returned as fp32: 6e-8 of rounding


def test_accumulate_matches_the_reference_golden(ops, golden):
    """B = 12 on the seeded joints of tests/golden/metrics.npz, with the gates tests/test_metrics.py uses"""
    from tests.test_metrics import metric_inputs

    g = golden("metrics")
    pred, gt = metric_inputs()
    B = pred.shape[0]
    out = np.concatenate([np.zeros((B, 3), np.float32), pred.reshape(B, 63)], axis=1)
    labels = np.concatenate([gt.reshape(B, 63), np.zeros((B, 42), np.float32)], axis=1)
    rec, per, al = run(ops, out, labels, g["rnge"])
    assert rec[0] == B and rec[1] == B and rec[2] == 0 and rec[3] == 0
    assert rel(al, g["pa_aligned"]) < 2e-5
    assert rel(rec[4] / B, g["mpjpe_mm"]) < 2e-6
    assert rel(rec[5] / B, g["pa_mpjpe_mm"]) < 1e-4
    from scat_amd.evaluator import finalize

    f = finalize(rec[None, :], g["rnge"])
    assert np.abs(f["pck"] - g["pck"]).max() < 1e-4
    assert np.abs(f["pck_pa"] - g["pck_pa"]).max() < 1e-4
    assert abs(f["auc"] - float(g["auc"])) < 1e-4


def _ordered_sum(col):
    s = 0.0
    for v in col.tolist():
        s += v
    return s


def test_record_sums_are_ordered_and_repeatable(ops):
    B, th = 257, THRESHOLDS["reference"]
    out, labels = inputs(B)
    rec, per, al = run(ops, out, labels, th)
    for c in range(3):
        assert rec[4 + c] == _ordered_sum(per[:, c]), c      # bit for bit: ascending sample order
    rec2, per2, al2 = run(ops, out, labels, th)
    assert rec.tobytes() == rec2.tobytes() and per.tobytes() == per2.tobytes() and al.tobytes() == al2.tobytes()


def test_keep_and_degenerate_samples(ops):
    B, th = 65, THRESHOLDS["reference"]
    out, labels = inputs(B)
    keep = np.ones(B, dtype=np.uint8)
    keep[[0, 5, 6, 63, 64]] = 0
    rec_k, per_k, al_k = run(ops, out, labels, th, keep)
    sel = keep.astype(bool)
    rec_c, per_c, al_c = run(ops, out[sel], labels[sel], th)
    assert rec_k[0] == B and rec_k[2] == 5 and rec_c[0] == B - 5 and rec_c[2] == 0
    same = [1, 3, 4, 5, 6, 7] + list(range(HEAD, HEAD + 2 * th.size))
    assert rec_k[same].tobytes() == rec_c[same].tobytes()
    assert np.array_equal(per_k[~sel], np.tile([0.0, 0.0, 0.0, 1.0], (5, 1))) and not al_k[~sel].any()
    assert per_k[sel].tobytes() == per_c.tobytes()
    rec_o = EO.batch(out, labels[:, :63], labels[:, 63:], th, keep)[0]
    assert np.array_equal(rec_k[:4], rec_o[:4]) and np.array_equal(rec_k[HEAD:], rec_o[HEAD:])

    # degenerate samples: a NaN joint, an infinite 2-D label, a NaN camera, an all-joints-equal prediction
    out_d, lab_d = out.copy(), labels.copy()
    out_d[7, 30] = np.nan
    lab_d[8, 70] = np.inf
    out_d[9, 1] = np.nan
    out_d[10, 3:] = np.tile(out[10, 3:6], 21)
    bad = [7, 8, 9, 10]
    rec_d, per_d, al_d = run(ops, out_d, lab_d, th)
    ok = np.ones(B, dtype=bool)
    ok[bad] = False
    rec_g, per_g, al_g = run(ops, out[ok], labels[ok], th)
    assert np.isfinite(rec_d).all() and np.isfinite(per_d).all() and np.isfinite(al_d).all()
    assert rec_d[0] == B and rec_d[1] == B - 4 and rec_d[2] == 0 and rec_d[3] == 4
    same = [1, 2, 4, 5, 6, 7] + list(range(HEAD, HEAD + 2 * th.size))
    assert rec_d[same].tobytes() == rec_g[same].tobytes()
    assert np.array_equal(per_d[bad], np.tile([0.0, 0.0, 0.0, 2.0], (4, 1))) and not al_d[bad].any()
    rec_o = EO.batch(out_d, lab_d[:, :63], lab_d[:, 63:], th)[0]
    assert np.array_equal(rec_d[:4], rec_o[:4]) and np.array_equal(rec_d[HEAD:], rec_o[HEAD:])


N_IMG = 3 * 224 * 224


def test_frame_mask_thresholds_abs_and_sample_zero(ops):
    """exactly representable sums at n = 150 528: | |sum| - 150528 | of 0, 1999, 2000, 2001, the abs, and the quirk"""
    ones = np.ones(N_IMG, dtype=np.float32)
    busy = synth.images(77, 1).reshape(-1)
    assert abs(abs(float(busy.astype(np.float64).sum())) - N_IMG) > 3000

    def holes(k, sign=1.0):
        f = sign * ones
        f[np.arange(k) * 73 + 5] = 0.0      # k pixels zeroed: the sum falls short of 150 528 by exactly k
        return f

    a = np.stack([ones, busy, -ones, ones, ones])
    assert a.shape == (5, N_IMG)
    keep = ops.eval_frame_mask(T_(a).to(DEV).reshape(5, 3, 224, 224)).cpu().numpy()
    assert keep.dtype == np.uint8 and keep.tolist() == [1, 1, 0, 0, 0] == EO.frame_mask(a, N_IMG, 2000.0).tolist()
    b = np.stack([busy, holes(1999), holes(2000), holes(2001), holes(2001, -1.0), holes(2000, -1.0)])
    keep = ops.eval_frame_mask(T_(b).to(DEV)).cpu().numpy()
    assert keep.tolist() == [1, 0, 0, 1, 1, 0] == EO.frame_mask(b, N_IMG, 2000.0).tolist()
    # other constants are honoured
    keep = ops.eval_frame_mask(T_(b).to(DEV), blank_sum=N_IMG - 2000.0, tol=0.5).cpu().numpy()
    assert keep.tolist() == [1, 1, 0, 1, 1, 0]


@pytest.mark.parametrize("n", [1, 255, 1027])
def test_frame_mask_head_and_tail(ops, n):
    """odd row lengths: rows start at every residue of 16 bytes, so the scalar head and tail of a row are both in play; a
    missed or doubled element moves the sum by 1 against a tolerance of 0.5"""
    B = 9
    x = np.ones((B, n), dtype=np.float32)
    x[2, 0] = 3.0
    x[3, n - 1] = 3.0
    x[6, 0] = 3.0
    x[7, n - 1] = 3.0
    want = [1, 0, 1, 1, 0, 0, 1, 1, 0]
    assert EO.frame_mask(x, float(n), 0.5).tolist() == want
    keep = ops.eval_frame_mask(T_(x).to(DEV), blank_sum=float(n), tol=0.5).cpu().numpy()
    assert keep.tolist() == want


def test_both_kernels_inside_guard_bands():
    """every operand between poisoned bands, aligned and skewed by one float; a record at an address = 4 mod 8 is refused"""
    from scat_amd._lib import ScatError, lib

    L = lib()
    L.scat_check_device()
    B, th = 65, THRESHOLDS["max"].astype(np.float32)
    T = th.size
    out, labels = inputs(B)
    keep_in = np.ones(B, dtype=np.uint8)
    keep_in[[3, 64]] = 0
    frames = np.ones((3, N_IMG), dtype=np.float32)
    frames[1] = synth.images(78, 1).reshape(-1)
    stream = torch.cuda.current_stream().cuda_stream
    arena = Arena(DEV, "nan", nbytes=32 << 20)
    got = {}
    for skew in (0, 1):
        arena.reset()
        dskew = 2 * skew      # doubles stay 8-byte aligned: moved by two floats
        o = arena.place(T_(out), skew, name="out")
        lab = arena.place(T_(labels), skew, name="labels")
        kp = arena.place(T_(keep_in), skew, name="keep")
        t = arena.place(T_(th), skew, name="thresholds")
        rec = arena.place((HEAD + 2 * T,), dskew, torch.float64, name="record", out=True)
        per = arena.place((B, 4), dskew, torch.float64, name="per_sample", out=True)
        al = arena.place((B, 63), skew, name="aligned", out=True)
        nws = L.scat_eval_accumulate_ws(B, T)
        ws = arena.place((nws,), dskew, torch.uint8, name="ws", out=True)
        assert o.data_ptr() % 16 == 4 * skew and rec.data_ptr() % 16 == 8 * skew
        L.scat_eval_accumulate(o.data_ptr(), lab.data_ptr(), lab.data_ptr() + 4 * 63, 105, kp.data_ptr(), t.data_ptr(), T,
                               rec.data_ptr(), per.data_ptr(), al.data_ptr(), B, ws.data_ptr(), nws, stream)
        x = arena.place(T_(frames), skew, name="frames")
        fk = arena.place((3,), skew, torch.uint8, name="frame_keep", out=True)
        nfw = L.scat_eval_frame_mask_ws(3, N_IMG)
        fws = arena.place((nfw,), dskew, torch.uint8, name="frame_ws", out=True)
        L.scat_eval_frame_mask(x.data_ptr(), fk.data_ptr(), 3, N_IMG, float(N_IMG), 2000.0, fws.data_ptr(), nfw, stream)
        torch.cuda.synchronize()
        arena.check()
        got[skew] = (rec.cpu().numpy().copy(), per.cpu().numpy().copy(), al.cpu().numpy().copy(), fk.cpu().numpy().copy())
    for a, b in zip(got[0], got[1]):
        assert a.tobytes() == b.tobytes()
    assert got[0][3].tolist() == [1, 1, 0]
    rec_o = EO.batch(out, labels[:, :63], labels[:, 63:], th, keep_in)[0]
    assert np.array_equal(got[0][0][:4], rec_o[:4]) and np.array_equal(got[0][0][HEAD:], rec_o[HEAD:])
    # a record (or per_sample) at 4 mod 8 is refused before any launch: nothing in the arena moves
    arena.reset()
    o = arena.place(T_(out), 0, name="out")
    lab = arena.place(T_(labels), 0, name="labels")
    t = arena.place(T_(th), 0, name="thresholds")
    # (as floats: a tensor of doubles can not sit at such an address)
    rec = arena.place((2 * (HEAD + 2 * T),), 1, name="record", out=True, finite=False)
    per = arena.place((B, 8), 1, name="per_sample", out=True, finite=False)
    assert rec.data_ptr() % 8 == 4 and per.data_ptr() % 8 == 4
    ws = arena.place((nws,), 0, torch.uint8, name="ws", out=True)
    before = rec.view(torch.int32).clone()
    for r, p in ((rec.data_ptr(), 0), (rec.data_ptr() + 4, per.data_ptr())):
        with pytest.raises(ScatError, match=r"\(-2\).*8-byte aligned"):      # SCAT_E_ARG
            L.scat_eval_accumulate(o.data_ptr(), lab.data_ptr(), lab.data_ptr() + 4 * 63, 105, 0, t.data_ptr(), T, r, p, 0, B,
                                   ws.data_ptr(), nws, stream)
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(rec.view(torch.int32), before)


def test_evaluator_end_to_end(ops):
    """three batches of 4 through the synthetic EncoderTransformer, a blank frame at index 2 of the second batch"""
    from scat_amd.evaluator import Evaluator, finalize
    from tests.test_gpu_model import make_encoder

    net = make_encoder(31)
    th = np.arange(20, 51, 5.0)
    xs = [synth.images(500 + i, 4) for i in range(3)]
    xs[1][2] = 1.0
    labs = [synth.labels(600 + i, 4) for i in range(3)]

    def wide(lab):      # the 61 + 63 + 42 layout of eval.py:852-855
        w = synth.uniform(9, "pose", (lab.shape[0], 166), -1.0, 1.0)
        w[:, 61:124], w[:, 124:] = lab[:, :63], lab[:, 63:]
        return w

    results = []
    for layout in (lambda v: v, wide):
        ev = Evaluator(net)
        random.seed(23)
        outs = [ev.update(T_(x).to(DEV), T_(layout(lab)).to(DEV)).cpu().numpy() for x, lab in zip(xs, labs)]
        r = ev.result()
        rows, margin = [], np.inf
        for x, lab, out in zip(xs, labs, outs):
            keep = EO.frame_mask(x, float(N_IMG), 2000.0)
            rec, _, _, samples = EO.batch(out, lab[:, :63], lab[:, 63:], th, keep)
            margin = min(margin, EO.margins(samples, th)[0])
            rows.append(rec)
        assert margin >= MIN_MARGIN_MM
        want = EO.finalize(np.stack(rows), th)
        assert (r["frames"], r["frames_kept"], r["frames_skipped"], r["frames_degenerate"]) == (12, 11, 1, 0)
        assert r["batches"] == 3 and r["batches_empty"] == 0
        for k, v in want.items():
            if isinstance(v, int):
                assert r[k] == v, k
            else:
                assert rel(r[k], v) < 1e-6, (k, r[k], v)
        assert r["pck"].shape == (7,) and np.isfinite(r["mpjpe_mm"]) and r["mpjpe_mm"] > 0
        results.append((r, outs))
    # the same network outputs scored under both label layouts give the same row, bit for bit
    out = T_(results[0][1][0]).to(DEV)
    t = T_(th.astype(np.float32)).to(DEV)
    r105 = ops.eval_accumulate(out, T_(labs[0]).to(DEV), t)[0].cpu().numpy()
    r166 = ops.eval_accumulate(out, T_(wide(labs[0])).to(DEV), t)[0].cpu().numpy()
    pair = ops.eval_accumulate(out, (T_(labs[0][:, :63].copy()).to(DEV), T_(labs[0][:, 63:].copy()).to(DEV)), t)[0].cpu().numpy()
    assert r105.tobytes() == r166.tobytes() == pair.tobytes()
