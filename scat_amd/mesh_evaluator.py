"""On-device mesh scoring: what a hand-mesh benchmark reports about predicted vertices — mean per-vertex error raw and
after a similarity alignment, the vertex PCK curve and its AUC, F-scores at 5 and 15 mm — with the scores of batch i
accumulated into row i of a table that stays on the GPU until ``result()`` (include/scat_mesh_eval.h).

    ev = MeshEvaluator()                         # PCK thresholds 0..50 mm in 100 steps, F-scores at 5 and 15 mm
    for pred_verts, gt_verts in batches:         # GPU tensors [B,V,3] fp32, metres, corresponding vertices
        ev.update(pred_verts, gt_verts)          # two kernels, no host synchronisation
    r = ev.result()                              # ONE device-to-host copy

``update_params`` takes MANO parameters instead and runs a ManoLayer on both sets first.  The joint scores of
scat_amd.evaluator are a separate table: Evaluator and finalize are not involved."""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from ._lib import ScatError
from .evaluator import area_under_curve

HEAD = ops.MESH_EVAL_RECORD_HEAD


def finalize_mesh(table, thresholds, f_thresholds):
    """table [n_batches, 8 + 2T + 2F] (the record rows of scat_mesh_eval_accumulate, a CPU array), thresholds [T] and
    f_thresholds [F] in mm -> dict.

    Every frame weighs alike: mpvpe_mm / pa_mpvpe_mm and f_score / f_score_pa [F] are means over all kept frames,
    pck_v / pck_v_pa [T] the pooled percentages 100 cnt / (V n_kept), auc_v / auc_v_pa the area under them over
    thresholds / max (evaluator.area_under_curve).  V is read from the rows that scored a batch; rows that disagree on it
    are an error.  Nothing kept: NaN rather than a division error."""
    t = np.asarray(table, dtype=np.float64).reshape(-1, np.asarray(table).shape[-1])
    th = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    fth = np.asarray(f_thresholds, dtype=np.float64).reshape(-1)
    T, F = th.size, fth.size
    if t.shape[1] != HEAD + 2 * T + 2 * F:
        raise ValueError(f"finalize_mesh: rows of {t.shape[1]} doubles do not match {T} thresholds and {F} F-score "
                         f"thresholds ({HEAD + 2 * T + 2 * F})")
    vs = sorted({int(round(v)) for v in t[:, 6]})
    if len(vs) > 1:
        raise ValueError(f"finalize_mesh: rows of different vertex counts {vs} do not pool")
    V = vs[0] if vs else 0
    n_in, n_kept, n_skip, n_deg = (int(round(v)) for v in t[:, :4].sum(axis=0)) if t.shape[0] else (0, 0, 0, 0)
    nan = float("nan")
    res = {"batches": int(t.shape[0]), "frames": n_in, "frames_kept": n_kept, "frames_skipped": n_skip,
           "frames_degenerate": n_deg, "vertices": V, "thresholds_mm": th.copy(), "f_thresholds_mm": fth.copy()}
    res["mpvpe_mm"] = float(t[:, 4].sum() / n_kept) if n_kept else nan
    res["pa_mpvpe_mm"] = float(t[:, 5].sum() / n_kept) if n_kept else nan
    xn = th / th.max() if T and th.max() > 0 else th
    for name, lo, flo in (("", HEAD, HEAD + 2 * T), ("_pa", HEAD + T, HEAD + 2 * T + F)):
        if n_kept:
            pck = 100.0 * t[:, lo:lo + T].sum(axis=0) / (float(V) * n_kept)
            fs = t[:, flo:flo + F].sum(axis=0) / n_kept
        else:
            pck, fs = np.full(T, nan), np.full(F, nan)
        res["pck_v" + name] = pck
        res["auc_v" + name] = area_under_curve(xn, pck) if T > 1 else nan
        res["f_score" + name] = fs
    return res


class MeshEvaluator:
    """Scores batches of predicted meshes against ground truth of the same topology and keeps the scores on the device."""

    def __init__(self, thresholds_mm=np.linspace(0, 50, 100), f_thresholds_mm=(5.0, 15.0), max_batches=4096):
        self.thresholds = np.asarray([float(t) for t in thresholds_mm], dtype=np.float32)
        self.f_thresholds = np.asarray([float(t) for t in f_thresholds_mm], dtype=np.float32)
        if not 1 <= self.thresholds.size <= 128:
            raise ValueError("MeshEvaluator: 1..128 thresholds")
        if not 1 <= self.f_thresholds.size <= 8:
            raise ValueError("MeshEvaluator: 1..8 F-score thresholds")
        self.max_batches = int(max_batches)
        self._table = self._th = self._fth = None
        self.n = 0

    @property
    def _width(self):
        return HEAD + 2 * self.thresholds.size + 2 * self.f_thresholds.size

    def reset(self):
        self.n = 0

    def update(self, pred_verts, gt_verts, keep=None):
        """One batch, [B,V,3] fp32 each; returns its per-sample rows (a device tensor, layout in
        include/scat_mesh_eval.h).  No .item(), no host copy, no synchronisation."""
        if not (isinstance(pred_verts, torch.Tensor) and isinstance(gt_verts, torch.Tensor) and pred_verts.is_cuda
                and gt_verts.is_cuda):
            raise ScatError("MeshEvaluator.update needs GPU tensors (no CPU fallback on the product path)")
        if self.n >= self.max_batches:
            raise ScatError(f"MeshEvaluator: more than max_batches = {self.max_batches} batches")
        if self._table is None or self._table.device != pred_verts.device:
            if self.n:
                raise ScatError(f"MeshEvaluator: the table is on {self._table.device}, this batch on {pred_verts.device}")
            self._table = torch.zeros((self.max_batches, self._width), dtype=torch.float64, device=pred_verts.device)
            self._th = torch.from_numpy(self.thresholds).to(pred_verts.device)
            self._fth = torch.from_numpy(self.f_thresholds).to(pred_verts.device)
        _, per_sample, _ = ops.mesh_eval_accumulate(pred_verts, gt_verts, self._th, self._fth, keep=keep,
                                                    record=self._table[self.n])
        self.n += 1
        return per_sample

    def update_params(self, layer, pred_params, gt_params, keep=None):
        """MANO parameters instead of vertices: [B,61] as ManoLayer.params_to_outputs takes them (3 camera, 3 global
        rotation, 45 finger pose, 10 shape; the camera is not used) or [B,58] without the camera.  ``layer`` (a
        ManoLayer) runs on both sets under no_grad and the meshes are scored."""
        verts = []
        with torch.no_grad():
            for name, p in (("pred_params", pred_params), ("gt_params", gt_params)):
                if not (isinstance(p, torch.Tensor) and p.is_cuda):
                    raise ScatError("MeshEvaluator.update_params needs GPU tensors (no CPU fallback on the product path)")
                if p.dim() != 2 or p.shape[1] not in (58, 61):
                    raise ScatError(f"MeshEvaluator.update_params needs {name} [B,61] or [B,58], got {tuple(p.shape)}")
                q = p[:, p.shape[1] - 58:]
                verts.append(layer(q[:, 0:3].contiguous(), q[:, 3:48].contiguous(), q[:, 48:58].contiguous())[:, 21:]
                             .contiguous())
        return self.update(verts[0], verts[1], keep=keep)

    def result(self):
        if self._table is None or self.n == 0:
            return finalize_mesh(np.zeros((0, self._width)), self.thresholds, self.f_thresholds)
        return finalize_mesh(self._table[:self.n].cpu().numpy(), self.thresholds, self.f_thresholds)
