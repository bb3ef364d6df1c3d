"""On-device mesh scoring on a real MI355X (include/scat_mesh_eval.h, scat_amd/mesh_evaluator.py) against the fp64 numpy
oracle of tests/_mesh_eval_oracle.py, and inside guard bands.  The inputs are those of tests/_mesh_eval_cases.py;
tests/test_mesh_eval.py asserts their conditions (margins, unique rotations, no ties, neighbours that differ from the
corresponding vertex) on the oracle alone."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_eval_cases as C  # noqa: E402
import _mesh_eval_oracle as MO  # noqa: E402
from _guard import Arena  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
HEAD, ROW = MO.HEAD, MO.ROW_HEAD

T_ = lambda a: torch.from_numpy(np.array(a))      # a copy: the shared inputs are read-only


@pytest.fixture(scope="module")
def ops():
    from scat_amd import ops as o
    from scat_amd._lib import lib

    lib().scat_check_device()
    return o


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def run(ops, pred, gt, tset, keep=None):
    th, fth = C.THRESHOLDS[tset]
    rec, per, al = ops.mesh_eval_accumulate(T_(pred).to(DEV), T_(gt).to(DEV), T_(th.astype(np.float32)).to(DEV),
                                            T_(fth.astype(np.float32)).to(DEV),
                                            keep=None if keep is None else T_(keep).to(DEV), want_aligned=True)
    return rec.cpu().numpy(), per.cpu().numpy(), al.cpu().numpy()


def int_columns(T, F):
    """the columns of a per_sample row that hold exact integers: flag, the PCK counts, every n_pred and n_gt"""
    cols = [0, 3] + list(range(ROW, ROW + 2 * T))
    cols += [ROW + 2 * T + 3 * i + j for i in range(2 * F) for j in (0, 1)]
    return cols


def f_columns(T, F):
    return [ROW + 2 * T + 3 * i + 2 for i in range(2 * F)]


@pytest.mark.parametrize("V,B,tset", C.CASES)
def test_accumulate_matches_the_oracle(ops, V, B, tset):
    """Frame counts, flags, every PCK count and every n_pred and n_gt are equal; sums, mpvpe, pa_mpvpe, F, the F sums and
    the fp32 aligned vertices within 1e-6 norm-wise relative (both sides are fp64 on identical fp32 inputs, so the true
    distance is rounding: tests/test_gpu_eval.py's gate and reasoning).  Measured worst over the cases on an MI355X: sums
    2.8e-15, mpvpe / pa_mpvpe 6.6e-15, F and its sums the same bits, aligned vertices 3.9e-8 (they are returned as fp32:
    that is their rounding)."""
    th, fth = C.THRESHOLDS[tset]
    T, F = th.size, fth.size
    pred, gt = C.inputs(V, B)
    rec_o, per_o, al_o = C.oracle(V, B, tset)
    rec, per, al = run(ops, pred, gt, tset)
    assert rec.shape == (HEAD + 2 * T + 2 * F,) and per.shape == (B, ROW + 2 * T + 6 * F) and al.shape == (B, V, 3)
    assert np.array_equal(rec[:4], rec_o[:4]) and rec[6] == V and rec[7] == 0.0
    ic = int_columns(T, F)
    assert np.array_equal(per[:, ic], per_o[:, ic])
    assert np.array_equal(rec[HEAD:HEAD + 2 * T], rec_o[HEAD:HEAD + 2 * T])
    if V == 1:      # every sample degenerate: a table of flags and zeros
        assert rec[3] == B and not rec[4:6].any() and not rec[HEAD:].any() and not al.any()
        assert np.array_equal(per, per_o)
        return
    assert rec_o[1] == B
    e_sum = max(abs(rec[c] - rec_o[c]) / abs(rec_o[c]) for c in (4, 5))
    e_fsum = rel(rec[HEAD + 2 * T:], rec_o[HEAD + 2 * T:])
    e_per = max(rel(per[:, c], per_o[:, c]) for c in (1, 2))
    e_f = rel(per[:, f_columns(T, F)], per_o[:, f_columns(T, F)])
    e_al = rel(al, al_o)
    print(f"V {V} B {B} {tset}: sums {e_sum:.3e} F sums {e_fsum:.3e} mpvpe/pa {e_per:.3e} F {e_f:.3e} aligned {e_al:.3e}")
    assert e_sum < 1e-6 and e_fsum < 1e-6 and e_per < 1e-6 and e_f < 1e-6
    assert e_al < 1e-6      # aligned is returned as fp32: 6e-8 of rounding


def _ordered_sum(col):
    s = 0.0
    for v in col.tolist():
        s += v
    return s


def test_record_is_ordered_repeatable_and_independent_of_the_batch(ops):
    """the sums are the per_sample columns added in ascending sample order, bit for bit; the same call twice gives the same
    bits; B = 65 split into calls of 64 and 1 gives the single call's per_sample rows"""
    V, B, tset = 65, 65, "workload"
    th, fth = C.THRESHOLDS[tset]
    T, F = th.size, fth.size
    pred, gt = C.inputs(V, B)
    rec, per, al = run(ops, pred, gt, tset)
    assert rec[4] == _ordered_sum(per[:, 1]) and rec[5] == _ordered_sum(per[:, 2])
    for i, c in enumerate(f_columns(T, F)):
        assert rec[HEAD + 2 * T + i] == _ordered_sum(per[:, c]), i
    assert np.array_equal(rec[HEAD:HEAD + 2 * T], per[:, ROW:ROW + 2 * T].sum(axis=0))
    rec2, per2, al2 = run(ops, pred, gt, tset)
    assert rec.tobytes() == rec2.tobytes() and per.tobytes() == per2.tobytes() and al.tobytes() == al2.tobytes()
    _, per_a, al_a = run(ops, pred[:64], gt[:64], tset)
    _, per_b, al_b = run(ops, pred[64:], gt[64:], tset)
    assert per.tobytes() == np.concatenate([per_a, per_b]).tobytes()
    assert al.tobytes() == np.concatenate([al_a, al_b]).tobytes()


def test_keep_and_degenerate_samples(ops):
    V, B, tset = 257, 6, "workload"
    th, fth = C.THRESHOLDS[tset]
    T, F = th.size, fth.size
    W = ROW + 2 * T + 6 * F
    pred, gt = C.inputs(V, B)
    zero_row = lambda flag: np.array([flag] + [0.0] * (W - 1))
    # skipped samples: counted, rows of zeros with flag 1, and none of their data read: they are poisoned with NaN
    keep = np.ones(B, dtype=np.uint8)
    keep[[0, 4]] = 0
    sel = keep.astype(bool)
    pred_k, gt_k = pred.copy(), gt.copy()
    pred_k[~sel], gt_k[~sel] = np.nan, np.nan
    rec_k, per_k, al_k = run(ops, pred_k, gt_k, tset, keep)
    rec_c, per_c, al_c = run(ops, pred[sel], gt[sel], tset)
    assert rec_k[0] == B and rec_k[1] == B - 2 and rec_k[2] == 2 and rec_k[3] == 0 and rec_c[0] == B - 2 and rec_c[2] == 0
    same = [1, 3, 4, 5, 6, 7] + list(range(HEAD, HEAD + 2 * T + 2 * F))
    assert rec_k[same].tobytes() == rec_c[same].tobytes()
    assert np.array_equal(per_k[~sel], np.stack([zero_row(1.0)] * 2)) and not al_k[~sel].any()
    assert per_k[sel].tobytes() == per_c.tobytes() and al_k[sel].tobytes() == al_c.tobytes()
    rec_o, per_o, _ = C.oracle(V, B, tset, keep)
    assert np.array_equal(rec_k[:4], rec_o[:4]) and np.array_equal(rec_k[HEAD:HEAD + 2 * T], rec_o[HEAD:HEAD + 2 * T])
    ic = int_columns(T, F)
    assert np.array_equal(per_k[:, ic], per_o[:, ic])

    # degenerate samples: a NaN in pred, an infinity in gt, an all-coincident pred
    pred_d, gt_d = pred.copy(), gt.copy()
    pred_d[0, 200, 1] = np.nan
    gt_d[2, 256, 2] = np.inf
    pred_d[5] = pred[5, 7]
    bad = [0, 2, 5]
    ok = np.ones(B, dtype=bool)
    ok[bad] = False
    rec_d, per_d, al_d = run(ops, pred_d, gt_d, tset)
    rec_g, per_g, al_g = run(ops, pred[ok], gt[ok], tset)
    assert np.isfinite(rec_d).all() and np.isfinite(per_d).all() and np.isfinite(al_d).all()
    assert rec_d[0] == B and rec_d[1] == B - 3 and rec_d[2] == 0 and rec_d[3] == 3
    same = [1, 2, 4, 5, 6, 7] + list(range(HEAD, HEAD + 2 * T + 2 * F))
    assert rec_d[same].tobytes() == rec_g[same].tobytes()      # the record moves by the documented counts only
    assert np.array_equal(per_d[bad], np.stack([zero_row(2.0)] * 3)) and not al_d[bad].any()
    assert per_d[ok].tobytes() == per_g.tobytes() and al_d[ok].tobytes() == al_g.tobytes()      # the neighbours' rows


def test_record_as_a_row_of_a_larger_table(ops):
    V, B, tset = 37, 6, "workload"
    th, fth = C.THRESHOLDS[tset]
    n = HEAD + 2 * th.size + 2 * fth.size
    pred, gt = C.inputs(V, B)
    table = torch.full((3, n), -7.0, dtype=torch.float64, device=DEV)
    p, g = T_(pred).to(DEV), T_(gt).to(DEV)
    rec, _, al = ops.mesh_eval_accumulate(p, g, th.tolist(), fth.tolist(), record=table[1])
    assert al is None and rec.data_ptr() == table[1].data_ptr()
    t = table.cpu().numpy()
    assert (t[0] == -7.0).all() and (t[2] == -7.0).all()
    assert t[1].tobytes() == run(ops, pred, gt, tset)[0].tobytes()
    from scat_amd._lib import ScatError

    with pytest.raises(ScatError, match="record as a contiguous fp64 GPU row"):
        ops.mesh_eval_accumulate(p, g, th.tolist(), fth.tolist(), record=table[:, 0])
    with pytest.raises(ScatError, match="gt of pred's shape"):
        ops.mesh_eval_accumulate(p, g[:, :36].contiguous(), th.tolist())
    with pytest.raises(ScatError, match="contiguous"):
        ops.mesh_eval_accumulate(p.transpose(0, 1), g.transpose(0, 1), th.tolist())
    with pytest.raises(ScatError, match="keep as a contiguous uint8"):
        ops.mesh_eval_accumulate(p, g, th.tolist(), keep=torch.ones(B, device=DEV))
    with pytest.raises(ScatError, match=r"1\.\.128"):
        ops.mesh_eval_accumulate(p, g, list(range(129)))
    with pytest.raises(ScatError, match=r"1\.\.8"):
        ops.mesh_eval_accumulate(p, g, th.tolist(), f_thresholds=list(range(1, 10)))


@pytest.mark.parametrize("V,tset", [(778, "workload"), (65, "caps")])
def test_kernels_inside_guard_bands(V, tset):
    """every operand between poisoned bands, at skews of 0, 1 and 3 floats, with and without the optional pointers; a
    record or per_sample at an address = 4 mod 8 is refused before any launch"""
    from scat_amd._lib import ScatError, lib

    L = lib()
    L.scat_check_device()
    B = 6
    th, fth = (a.astype(np.float32) for a in C.THRESHOLDS[tset])
    T, F = th.size, fth.size
    pred, gt = C.inputs(V, B)
    keep_in = np.ones(B, dtype=np.uint8)
    keep_in[[1, 5]] = 0
    stream = torch.cuda.current_stream().cuda_stream
    arena = Arena(DEV, "nan", nbytes=8 << 20)
    got = {}
    for skew in (0, 1, 3):
        for optional in (True, False):
            arena.reset()
            dskew = 2 * (skew % 2)      # doubles stay 8-byte aligned: moved by two floats or not at all
            p = arena.place(T_(pred), skew, name="pred")
            g = arena.place(T_(gt), skew, name="gt")
            t = arena.place(T_(th), skew, name="thresholds")
            ft = arena.place(T_(fth), skew, name="f_thresholds")
            rec = arena.place((HEAD + 2 * T + 2 * F,), dskew, torch.float64, name="record", out=True)
            per = arena.place((B, ROW + 2 * T + 6 * F), dskew, torch.float64, name="per_sample", out=True)
            kp = al = None
            if optional:
                kp = arena.place(T_(keep_in), skew, name="keep")
                al = arena.place((B, V, 3), skew, name="aligned", out=True)
            assert p.data_ptr() % 16 == 4 * skew and rec.data_ptr() % 16 == 4 * dskew
            L.scat_mesh_eval_accumulate(p.data_ptr(), g.data_ptr(), V, kp.data_ptr() if optional else 0, t.data_ptr(), T,
                                        ft.data_ptr(), F, rec.data_ptr(), per.data_ptr(), al.data_ptr() if optional else 0,
                                        B, stream)
            torch.cuda.synchronize()
            arena.check()
            got[skew, optional] = (rec.cpu().numpy().copy(), per.cpu().numpy().copy(),
                                   al.cpu().numpy().copy() if optional else None)
    for optional in (True, False):
        for skew in (1, 3):
            for a, b in zip(got[0, optional], got[skew, optional]):
                assert (a is None and b is None) or a.tobytes() == b.tobytes()
    for optional, keep in ((True, keep_in), (False, None)):
        rec_o, per_o, _ = C.oracle(V, B, tset, keep)
        ic = int_columns(T, F)
        assert np.array_equal(got[0, optional][0][:4], rec_o[:4]) and np.array_equal(got[0, optional][1][:, ic], per_o[:, ic])
    # a record (or per_sample) at 4 mod 8 is refused before any launch: nothing in the arena moves
    arena.reset()
    p = arena.place(T_(pred), 0, name="pred")
    g = arena.place(T_(gt), 0, name="gt")
    t = arena.place(T_(th), 0, name="thresholds")
    ft = arena.place(T_(fth), 0, name="f_thresholds")
    # (as floats: a tensor of doubles can not sit at such an address)
    rec = arena.place((2 * (HEAD + 2 * T + 2 * F) + 2,), 1, name="record", out=True, finite=False)
    per = arena.place((B, 2 * (ROW + 2 * T + 6 * F) + 2), 1, name="per_sample", out=True, finite=False)
    assert rec.data_ptr() % 8 == 4 and per.data_ptr() % 8 == 4
    before = (rec.view(torch.int32).clone(), per.view(torch.int32).clone())
    for r, q in ((rec.data_ptr(), per.data_ptr() + 4), (rec.data_ptr() + 4, per.data_ptr())):
        with pytest.raises(ScatError, match=r"\(-2\).*8-byte aligned"):      # SCAT_E_ARG
            L.scat_mesh_eval_accumulate(p.data_ptr(), g.data_ptr(), V, 0, t.data_ptr(), T, ft.data_ptr(), F, r, q, 0, B, stream)
    torch.cuda.synchronize()
    arena.check()
    assert torch.equal(rec.view(torch.int32), before[0]) and torch.equal(per.view(torch.int32), before[1])


class _Syncs:
    """counts what torch itself calls a synchronizing operation (torch.cuda.set_sync_debug_mode) inside a block"""

    def __enter__(self):
        self.mode = torch.cuda.get_sync_debug_mode()
        self.cm = warnings.catch_warnings(record=True)
        self.log = self.cm.__enter__()
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        return self

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.mode)
        self.n = sum("synchronizing" in str(w.message) for w in self.log)
        self.cm.__exit__(*exc)


def test_mesh_evaluator_end_to_end(ops, monkeypatch):
    """three batches of unequal size against finalize_mesh of the oracle's rows; update() does not synchronise (after the
    first, which allocates the table), result() makes exactly one device-to-host copy"""
    from scat_amd.mesh_evaluator import MeshEvaluator, finalize_mesh

    V, tset = 257, "workload"
    th, fth = C.THRESHOLDS[tset]
    sizes = (6, 1, 4)
    batches = [C.inputs(V, 6), C.inputs(V, 1), tuple(a[:4] for a in C.inputs(V, 65))]
    keeps = [None, None, np.array([1, 0, 1, 1], dtype=np.uint8)]
    bad = batches[0][0].copy()
    bad[5, 3, 0] = np.inf      # one degenerate frame
    batches[0] = (bad, batches[0][1])
    dev = [(T_(p).to(DEV), T_(g).to(DEV), None if k is None else T_(k).to(DEV)) for (p, g), k in zip(batches, keeps)]
    ev = MeshEvaluator(th, fth, max_batches=8)
    rows = []
    for i, (p, g, k) in enumerate(dev):
        with _Syncs() as s:
            per = ev.update(p, g, keep=k)
        assert per.shape == (sizes[i], ROW + 2 * th.size + 6 * fth.size)
        if i:
            assert s.n == 0, "update() synchronised"
        S = [MO.sample(a, b) for a, b in zip(*batches[i])]
        margin, ratio = MO.margins(S, th, fth, keeps[i])      # conditions on the inputs, from the oracle alone
        assert margin >= C.MIN_MARGIN_MM and ratio >= C.MIN_RATIO and not any(q.get("tie") for q in S)
        rows.append(MO.batch(S, th, fth, keeps[i])[0])
    assert ev.n == 3
    copies = []
    to_host = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **kw: (copies.append(tuple(self.shape)), to_host(self, *a, **kw))[1])
    with _Syncs() as s:
        r = ev.result()
    monkeypatch.undo()
    assert copies == [(3, HEAD + 2 * th.size + 2 * fth.size)] and s.n == 1, (copies, s.n)
    want = MO.finalize(np.stack(rows), th, fth)
    assert (r["batches"], r["frames"], r["frames_kept"], r["frames_skipped"], r["frames_degenerate"]) == (3, 11, 9, 1, 1)
    assert r["vertices"] == V
    for k, v in want.items():
        if isinstance(v, int):
            assert r[k] == v, k
        else:
            assert rel(r[k], v) < 1e-6, (k, r[k], v)
    assert r["pck_v"].shape == (100,) and r["f_score"].shape == (2,) and 0 < r["pa_mpvpe_mm"] < r["mpvpe_mm"]
    assert finalize_mesh(ev._table[:3].cpu().numpy(), th, fth)["mpvpe_mm"] == r["mpvpe_mm"]
    # a batch of another vertex count does not pool; reset() starts over
    p37, g37 = (T_(a).to(DEV) for a in C.inputs(37, 1))
    ev.update(p37, g37)
    with pytest.raises(ValueError, match="vertex counts"):
        ev.result()
    ev.reset()
    ev.update(p37, g37)
    r = ev.result()
    assert (r["batches"], r["frames"], r["vertices"]) == (1, 1, 37)


def test_update_params_scores_the_layers_own_meshes(ops):
    """MANO parameters in, ManoLayer on both sets, against the oracle fed with the layer's own output"""
    from scat_amd import synth
    from scat_amd.mano import ManoLayer, ManoModel
    from scat_amd.mesh_evaluator import MeshEvaluator

    B, V = 5, 37
    model = ManoModel.synthetic(3, V=V).to(torch.device(DEV, 0))
    layer = ManoLayer(model)
    gt_p = np.concatenate([synth.normal_like(41, n, (B, k), s) for n, k, s in
                           (("cam", 3, 1.0), ("rots", 3, 0.8), ("poses", 45, 0.4), ("betas", 10, 1.0))], axis=1).astype(np.float32)
    pred_p = (gt_p + synth.normal_like(42, "noise", (B, 61), 0.05)).astype(np.float32)
    gp, pp = T_(gt_p).to(DEV), T_(pred_p).to(DEV)
    th, fth = C.THRESHOLDS["workload"]
    ev = MeshEvaluator(th, fth, max_batches=2)
    per = ev.update_params(layer, pp, gp).cpu().numpy()
    ev.update_params(layer, pp[:, 3:].contiguous(), gp[:, 3:].contiguous())      # without the camera: the same meshes
    with torch.no_grad():
        vp = layer(pp[:, 3:6].contiguous(), pp[:, 6:51].contiguous(), pp[:, 51:61].contiguous())[:, 21:].cpu().numpy()
        vg = layer(gp[:, 3:6].contiguous(), gp[:, 6:51].contiguous(), gp[:, 51:61].contiguous())[:, 21:].cpu().numpy()
    assert vp.shape == (B, V, 3)
    S = [MO.sample(a, b) for a, b in zip(vp, vg)]
    margin, ratio = MO.margins(S, th, fth)
    assert margin >= C.MIN_MARGIN_MM and ratio >= C.MIN_RATIO and not any(s["degenerate"] or s["tie"] for s in S)
    rec_o, per_o, _ = MO.batch(S, th, fth)
    ic = int_columns(th.size, fth.size)
    assert np.array_equal(per[:, ic], per_o[:, ic])
    assert max(rel(per[:, c], per_o[:, c]) for c in (1, 2)) < 1e-6
    table = ev._table[:2].cpu().numpy()
    assert table[0].tobytes() == table[1].tobytes()
    r, want = ev.result(), MO.finalize(np.stack([rec_o, rec_o]), th, fth)
    assert r["frames"] == 2 * B and r["frames_kept"] == 2 * B
    for k, v in want.items():
        if not isinstance(v, int):
            assert rel(r[k], v) < 1e-6, (k, r[k], v)
    assert pp.grad is None and not per_o[:, 1].max() == 0.0
