"""fp64 numpy oracle of on-device evaluation (include/scat_eval.h, scat_amd/evaluator.py), written from the reference's
formulas (eval.py:110-161, 300-340, 467-475, 817-823, 998, 1026-1029) and not from the kernels: the rotation comes from
numpy.linalg.svd as in the reference, the library's from a quaternion eigenvector.  Plain helper module."""
from __future__ import annotations

import numpy as np

HEAD = 8


def procrustes(S1, S2):
    """one sample, [21,3] fp64: S1 aligned onto S2 (eval.py:110-161), plus (sigma2 + sign(det K) sigma3) / sigma1"""
    mu1, mu2 = S1.mean(axis=0), S2.mean(axis=0)
    X1, X2 = (S1 - mu1).T, (S2 - mu2).T                     # [3,21] as the reference holds them
    var1 = (X1 ** 2).sum()
    K = X1 @ X2.T
    U, s, Vt = np.linalg.svd(K)
    Z = np.eye(3)
    Z[2, 2] = np.sign(np.linalg.det(U @ Vt))
    R = Vt.T @ Z @ U.T
    with np.errstate(all="ignore"):
        scale = np.trace(R @ K) / var1
        t = mu2 - scale * (R @ mu1)
        aligned = (scale * (R @ S1.T)).T + t
        ratio = (s[1] + np.sign(np.linalg.det(K)) * s[2]) / s[0] if s[0] > 0 else 0.0
    return aligned, var1, ratio


def sample(out66, gt3d, gt2d):
    """one sample -> dict(mpjpe, pa, e2d, d_raw[21], d_pa[21], aligned[21,3], degenerate, ratio); inputs fp32"""
    o = np.asarray(out66, dtype=np.float64).reshape(66)
    g = np.asarray(gt3d, dtype=np.float64).reshape(21, 3)
    g2 = np.asarray(gt2d, dtype=np.float64).reshape(21, 2)
    cam, p = o[:3], o[3:].reshape(21, 3)
    bad = not (np.isfinite(o).all() and np.isfinite(g).all() and np.isfinite(g2).all())
    zero = dict(mpjpe=0.0, pa=0.0, e2d=0.0, d_raw=np.zeros(21), d_pa=np.zeros(21), aligned=np.zeros((21, 3)),
                degenerate=True, ratio=0.0)
    if bad:
        return zero
    aligned, var1, ratio = procrustes(p, g)
    if var1 == 0.0:
        return zero
    d_raw = 1000.0 * np.linalg.norm(p - g, axis=1)
    d_pa = 1000.0 * np.linalg.norm(aligned - g, axis=1)
    proj = (cam[0] * (p[:, :2] + cam[1:3])) * 112.0 + 112.0      # eval.py:467-475
    e2d = np.linalg.norm(proj - g2, axis=1).mean()
    return dict(mpjpe=d_raw.mean(), pa=d_pa.mean(), e2d=e2d, d_raw=d_raw, d_pa=d_pa, aligned=aligned, degenerate=False,
                ratio=ratio)


def batch(out, gt3d, gt2d, thresholds, keep=None):
    """-> (record [8+2T], per_sample [B,4], aligned [B,21,3], samples): the row scat_eval_accumulate writes; the three
    sums run over the kept samples in ascending order"""
    B = out.shape[0]
    th = np.asarray(thresholds, dtype=np.float32).astype(np.float64)
    T = th.size
    rec = np.zeros(HEAD + 2 * T)
    per = np.zeros((B, 4))
    al = np.zeros((B, 21, 3))
    samples = []
    rec[0] = B
    for b in range(B):
        if keep is not None and not keep[b]:
            per[b, 3] = 1
            rec[2] += 1
            samples.append(None)
            continue
        s = sample(out[b], gt3d[b], gt2d[b])
        samples.append(s)
        if s["degenerate"]:
            per[b, 3] = 2
            rec[3] += 1
            continue
        rec[1] += 1
        per[b, :3] = s["mpjpe"], s["pa"], s["e2d"]
        al[b] = s["aligned"]
        rec[4] += s["mpjpe"]
        rec[5] += s["pa"]
        rec[6] += s["e2d"]
        rec[HEAD:HEAD + T] += (s["d_raw"][None, :] <= th[:, None]).sum(axis=1)
        rec[HEAD + T:] += (s["d_pa"][None, :] <= th[:, None]).sum(axis=1)
    return rec, per, al, samples


def margins(samples, thresholds):
    """(smallest |distance - threshold| in mm, smallest uniqueness ratio) over the scored samples of a batch"""
    th = np.asarray(thresholds, dtype=np.float32).astype(np.float64)
    m, r = np.inf, np.inf
    for s in samples:
        if s is None or s["degenerate"]:
            continue
        d = np.concatenate([s["d_raw"], s["d_pa"]])
        m = min(m, np.abs(d[:, None] - th[None, :]).min())
        r = min(r, s["ratio"])
    return m, r


def frame_mask(x, blank_sum, tol):
    """eval.py:817-823 with its quirk: sample 0 is never dropped"""
    s = np.abs(np.asarray(x, dtype=np.float64).reshape(x.shape[0], -1).sum(axis=1))
    keep = (np.abs(s - blank_sum) > tol).astype(np.uint8)
    keep[0] = 1
    return keep


def auc(x, y):
    """eval.py:328-340"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    _, i = np.unique(x, return_index=True)
    x, y = x[i], y[i]
    return np.trapezoid(y, x) / np.trapezoid(np.ones_like(x), x)


def finalize(table, thresholds):
    """the eval loop's bookkeeping over record rows, batch by batch as eval.py:998-1029 does it"""
    th = np.asarray(thresholds, dtype=np.float64)
    T = th.size
    tot = np.zeros(7)
    pck_all, pck_pa_all, n = np.zeros(T), np.zeros(T), 0
    cnt, cnt_pa = np.zeros(T), np.zeros(T)
    empty = 0
    for row in np.asarray(table, dtype=np.float64):
        tot += row[:7]
        cnt += row[HEAD:HEAD + T]
        cnt_pa += row[HEAD + T:]
        if row[1] == 0:
            empty += 1
            continue
        n += 1
        pck_all += 100.0 * row[HEAD:HEAD + T] / (21 * row[1])
        pck_pa_all += 100.0 * row[HEAD + T:] / (21 * row[1])
    res = dict(frames=int(tot[0]), frames_kept=int(tot[1]), frames_skipped=int(tot[2]), frames_degenerate=int(tot[3]),
               batches_empty=empty)
    if tot[1] == 0:
        return res
    res.update(mpjpe_mm=tot[4] / tot[1], pa_mpjpe_mm=tot[5] / tot[1], err2d_px=tot[6] / tot[1],
               pck=pck_all / n, pck_pa=pck_pa_all / n, pck_pooled=100.0 * cnt / (21 * tot[1]),
               pck_pa_pooled=100.0 * cnt_pa / (21 * tot[1]))
    for k in ("pck", "pck_pa", "pck_pooled", "pck_pa_pooled"):
        res[k.replace("pck", "auc")] = auc(th / th.max(), res[k])
    return res
