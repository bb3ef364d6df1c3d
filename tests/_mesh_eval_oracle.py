"""fp64 numpy oracle of on-device mesh scoring (include/scat_mesh_eval.h, scat_amd/mesh_evaluator.py), written from the
rules the header states and not from the kernels: brute-force distance matrices, and the alignment of tests/_eval_oracle.py
(numpy.linalg.svd, where the library takes a quaternion eigenvector).  The F-score is the one of point-cloud
reconstruction, F = 2 n_pred n_gt / (V (n_pred + n_gt)) from nearest-neighbour distances strictly below a threshold; this
module is its authority.  Plain helper module."""
from __future__ import annotations

import numpy as np

from _eval_oracle import auc, procrustes

HEAD = 8
ROW_HEAD = 4


def nearest(q, c):
    """q [V,3], c [V,3] fp64 -> (d_qc [V], d_cq [V], arg_qc [V], arg_cq [V], tie): the distance from every q_i to its
    nearest c_j and from every c_j to its nearest q_i (one sqrt, after the minimum of the squared distances), who that
    neighbour is, and whether any minimum is attained twice"""
    d2 = ((q[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)
    out, tie = [], False
    for m in (d2, d2.T):
        arg = m.argmin(axis=1)
        lo = m[np.arange(m.shape[0]), arg]
        if m.shape[1] > 1:
            second = np.partition(m, 1, axis=1)[:, 1]
            tie = tie or bool((second == lo).any())
        out.append((np.sqrt(lo), arg))
    return out[0][0], out[1][0], out[0][1], out[1][1], tie


def sample(pred, gt):
    """one sample, [V,3] fp32 each -> dict(degenerate, mpvpe, pa, d_raw[V], d_pa[V], aligned[V,3], ratio, tie, and for
    side in raw / pa: nn_<side> = (pred -> gt [V], gt -> pred [V]) in mm, arg_<side> the neighbours)"""
    p, g = np.asarray(pred, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    V = p.shape[0]
    if not (np.isfinite(p).all() and np.isfinite(g).all()):
        return dict(degenerate=True, V=V)
    aligned, var1, ratio = procrustes(p, g)
    if var1 == 0.0:
        return dict(degenerate=True, V=V)
    d_raw = 1000.0 * np.linalg.norm(p - g, axis=1)
    d_pa = 1000.0 * np.linalg.norm(aligned - g, axis=1)
    s = dict(degenerate=False, V=V, mpvpe=d_raw.mean(), pa=d_pa.mean(), d_raw=d_raw, d_pa=d_pa, aligned=aligned, ratio=ratio)
    tie = False
    for side, q in (("raw", p), ("pa", aligned)):
        dq, dg, aq, ag, t = nearest(q, g)
        s["nn_" + side], s["arg_" + side] = (1000.0 * dq, 1000.0 * dg), (aq, ag)
        tie = tie or t
    s["tie"] = tie
    return s


def f_score(n_pred, n_gt, V):
    return 2.0 * n_pred * n_gt / (V * (n_pred + n_gt)) if n_pred + n_gt > 0 else 0.0


def scores(s, thresholds, f_thresholds):
    """the per_sample row of a scored sample: 4 + 2T + 6F doubles"""
    th = np.asarray(thresholds, dtype=np.float32).astype(np.float64)
    fth = np.asarray(f_thresholds, dtype=np.float32).astype(np.float64)
    row = [0.0, s["mpvpe"], s["pa"], 0.0]
    row += [float((s["d_raw"] <= t).sum()) for t in th] + [float((s["d_pa"] <= t).sum()) for t in th]
    for side in ("raw", "pa"):
        dq, dg = s["nn_" + side]
        for t in fth:
            n_pred, n_gt = float((dq < t).sum()), float((dg < t).sum())
            row += [n_pred, n_gt, f_score(n_pred, n_gt, s["V"])]
    return np.array(row)


def batch(samples, thresholds, f_thresholds, keep=None):
    """samples: [sample(pred[b], gt[b])] (None where keep[b] == 0 is fine) -> (record [8 + 2T + 2F],
    per_sample [B, 4 + 2T + 6F], aligned [B,V,3]): what scat_mesh_eval_accumulate writes; the sums run over the kept
    samples in ascending order"""
    B = len(samples)
    T, F = np.asarray(thresholds).size, np.asarray(f_thresholds).size
    V = next(s["V"] for s in samples if s is not None)
    rec = np.zeros(HEAD + 2 * T + 2 * F)
    per = np.zeros((B, ROW_HEAD + 2 * T + 6 * F))
    al = np.zeros((B, V, 3))
    rec[0], rec[6] = B, V
    for b, s in enumerate(samples):
        if keep is not None and not keep[b]:
            per[b, 0] = 1
            rec[2] += 1
            continue
        if s["degenerate"]:
            per[b, 0] = 2
            rec[3] += 1
            continue
        row = scores(s, thresholds, f_thresholds)
        per[b], al[b] = row, s["aligned"]
        rec[1] += 1
        rec[4] += row[1]
        rec[5] += row[2]
        rec[HEAD:HEAD + 2 * T] += row[ROW_HEAD:ROW_HEAD + 2 * T]
        fs = row[ROW_HEAD + 2 * T:].reshape(2, F, 3)[:, :, 2]
        rec[HEAD + 2 * T:] += fs.reshape(-1)
    return rec, per, al


def margins(samples, thresholds, f_thresholds, keep=None):
    """(smallest |distance - threshold| in mm, smallest rotation-uniqueness ratio) over the scored samples: corresponding
    distances against the PCK thresholds, nearest-neighbour distances against the F-score thresholds"""
    th = np.asarray(thresholds, dtype=np.float32).astype(np.float64)
    fth = np.asarray(f_thresholds, dtype=np.float32).astype(np.float64)
    m, r = np.inf, np.inf
    for b, s in enumerate(samples):
        if s is None or s["degenerate"] or (keep is not None and not keep[b]):
            continue
        d = np.concatenate([s["d_raw"], s["d_pa"]])
        n = np.concatenate([*s["nn_raw"], *s["nn_pa"]])
        m = min(m, np.abs(d[:, None] - th[None, :]).min(), np.abs(n[:, None] - fth[None, :]).min())
        r = min(r, s["ratio"])
    return m, r


def finalize(table, thresholds, f_thresholds):
    """the bookkeeping over record rows, row by row: every frame weighs alike"""
    th = np.asarray(thresholds, dtype=np.float64)
    T, F = th.size, np.asarray(f_thresholds).size
    tot = np.zeros(6)
    cnt, fsum, V = np.zeros(2 * T), np.zeros(2 * F), None
    for row in np.asarray(table, dtype=np.float64):
        tot += row[:6]
        cnt += row[HEAD:HEAD + 2 * T]
        fsum += row[HEAD + 2 * T:]
        assert V in (None, row[6])
        V = row[6]
    res = dict(frames=int(tot[0]), frames_kept=int(tot[1]), frames_skipped=int(tot[2]), frames_degenerate=int(tot[3]))
    if tot[1] == 0:
        return res
    res.update(vertices=int(V), mpvpe_mm=tot[4] / tot[1], pa_mpvpe_mm=tot[5] / tot[1],
               pck_v=100.0 * cnt[:T] / (V * tot[1]), pck_v_pa=100.0 * cnt[T:] / (V * tot[1]),
               f_score=fsum[:F] / tot[1], f_score_pa=fsum[F:] / tot[1])
    if T > 1:
        res.update(auc_v=auc(th / th.max(), res["pck_v"]), auc_v_pa=auc(th / th.max(), res["pck_v_pa"]))
    return res
