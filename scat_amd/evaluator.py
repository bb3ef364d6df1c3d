"""On-device evaluation: what the reference's eval loop (eval.py:788-1053) does per batch on the host — eval-mode forward,
blank padding frames dropped, Procrustes alignment, PCK, MPJPE — with the scores of batch i accumulated into row i of a
table that stays on the GPU until ``result()``.

    ev = Evaluator(net)                          # thresholds 20..50 mm, eval.py:806
    for inputs, labels in loader:                # GPU tensors: [B,3,224,224] fp32, [B,105] or [B,166] fp32
        ev.update(inputs, labels)                # forward + two small kernels, no host synchronisation
    r = ev.result()                              # ONE device-to-host copy

The reference keeps its token masking active in eval mode (hand_net.py:369-373 draws from python ``random`` on every
call); ``update`` does not touch that generator, the caller seeds it."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import ScatError

HEAD = ops.EVAL_RECORD_HEAD


def area_under_curve(xpts, ypts):
    """eval.py:328-340: trapezoid area over the distinct abscissae, divided by that of the constant 1."""
    xpts, ypts = np.asarray(xpts, dtype=np.float64), np.asarray(ypts, dtype=np.float64)
    _, idx = np.unique(xpts, return_index=True)
    x, y = xpts[idx], ypts[idx]
    trapz = lambda v: float(np.sum((v[1:] + v[:-1]) * np.diff(x)) / 2.0)
    return trapz(y) / trapz(np.ones_like(x))


def finalize(table, thresholds):
    """table [n_batches, 8 + 2T] (the record rows of scat_eval_accumulate, a CPU array), thresholds [T] in mm -> dict.

    pck / pck_pa / auc / auc_pa are the reference's: the per-batch percentage 100 cnt / (21 n_kept) averaged over the
    batches with equal weight (eval.py:998, :1028; a batch without a kept frame has no percentage, it is left out and
    counted in ``batches_empty``), AUC over thresholds / max (eval.py:1029).  The ``*_pooled`` values weigh every frame
    alike.  mpjpe_mm / pa_mpjpe_mm / err2d_px are means over all kept frames."""
    t = np.asarray(table, dtype=np.float64).reshape(-1, np.asarray(table).shape[-1])
    th = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    T = th.size
    if t.shape[1] != HEAD + 2 * T:
        raise ValueError(f"finalize: rows of {t.shape[1]} doubles do not match {T} thresholds ({HEAD + 2 * T})")
    n_in, n_kept, n_skip, n_deg = (int(round(v)) for v in t[:, :4].sum(axis=0)) if t.shape[0] else (0, 0, 0, 0)
    nan = float("nan")
    res = {"batches": int(t.shape[0]), "frames": n_in, "frames_kept": n_kept, "frames_skipped": n_skip,
           "frames_degenerate": n_deg, "thresholds_mm": th.copy()}
    for k, col in (("mpjpe_mm", 4), ("pa_mpjpe_mm", 5), ("err2d_px", 6)):
        res[k] = float(t[:, col].sum() / n_kept) if n_kept else nan
    live = t[:, 1] > 0
    res["batches_empty"] = int((~live).sum())
    xn = th / th.max()
    for name, lo in (("", HEAD), ("_pa", HEAD + T)):
        cnt = t[:, lo:lo + T]
        if live.any():
            per_batch = 100.0 * cnt[live] / (21.0 * t[live, 1:2])
            pck = per_batch.mean(axis=0)
            pooled = 100.0 * cnt.sum(axis=0) / (21.0 * n_kept)
        else:
            pck = pooled = np.full(T, nan)
        res["pck" + name], res["pck" + name + "_pooled"] = pck, pooled
        res["auc" + name] = area_under_curve(xn, pck) if T > 1 else nan
        res["auc" + name + "_pooled"] = area_under_curve(xn, pooled) if T > 1 else nan
    return res


class Evaluator:
    """Runs ``net`` over batches and keeps the scores on the device.  preprocess="u8": ``inputs`` are uint8 frames
    [B,3,H,W], resized and normalised by ops.preprocess_u8 first."""

    def __init__(self, net, thresholds_mm=range(20, 51, 5), skip_blank=True, max_batches=4096, preprocess=None):
        if preprocess not in (None, "u8"):
            raise ValueError(f"Evaluator: preprocess must be None or 'u8', got {preprocess!r}")
        self.net, self.skip_blank, self.max_batches, self.preprocess = net, bool(skip_blank), int(max_batches), preprocess
        self.thresholds = np.asarray([float(t) for t in thresholds_mm], dtype=np.float32)
        if not 1 <= self.thresholds.size <= 64:
            raise ValueError("Evaluator: 1..64 thresholds")
        self._table = self._th = None
        self.n = 0

    def reset(self):
        self.n = 0

    def update(self, inputs, labels):
        """One batch; returns the network's outputs [B,66].  No .item(), no host copy, no synchronisation."""
        if not (inputs.is_cuda and labels.is_cuda):
            raise ScatError("Evaluator.update needs GPU tensors (no CPU fallback on the product path)")
        if self.n >= self.max_batches:
            raise ScatError(f"Evaluator: more than max_batches = {self.max_batches} batches")
        if self._table is None:
            T = self.thresholds.size
            self._table = torch.zeros((self.max_batches, HEAD + 2 * T), dtype=torch.float64, device=inputs.device)
            self._th = torch.from_numpy(self.thresholds).to(inputs.device)
        if self.preprocess == "u8":
            inputs = ops.preprocess_u8(inputs)
        self.net.eval()
        with torch.no_grad():
            out = self.net(inputs)[0]
        keep = ops.eval_frame_mask(inputs) if self.skip_blank else None
        ops.eval_accumulate(out, labels, self._th, keep=keep, record=self._table[self.n])
        self.n += 1
        return out

    def result(self):
        if self._table is None or self.n == 0:
            return finalize(np.zeros((0, HEAD + 2 * self.thresholds.size)), self.thresholds)
        return finalize(self._table[:self.n].cpu().numpy(), self.thresholds)
