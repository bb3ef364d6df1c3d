#!/usr/bin/env python
"""On-device mesh scoring against what a user has without it, V = 778, T = 100, F = 2, batch 1 / 96 / 1024: device events
after warm-up, medians over alternated repeats (the method of tools/fit_bench.py).

  kernel       ops.mesh_eval_accumulate: two launches (scat_mesh_eval_accumulate), its three output allocations included
  torch_fp64   the same scores written with torch on the device in fp64: torch.cdist (its default mode, which takes the
               matrix-product form at this size) and min for the nearest neighbours in both directions, raw and aligned;
               torch.linalg.svd and det for the alignment; comparisons and sums for the counts.  In chunks of 64 samples,
               so that the distance matrices of batch 1024 (4.9 GB each in fp64) fit.

Every case is a window of ``inner`` calls between two events (host launch time included); the cases alternate inside every
repeat so that drift hits both alike.  The kernel's scores are checked against the baseline's in the same run: counts
equal, mpvpe / pa_mpvpe / F within 1e-6.  Prints the median and the spread and the ratio; with --out also writes the table
to a file (profiles/mesh_eval_bench.txt is such a run).  Not measured here: the two launches apart, and the sample kernel
without the fold."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

CHUNK = 64


def torch_scores(pred, gt, th, fth):
    """pred, gt [B,V,3] fp32, th [T], fth [F] fp64 on the device -> dict of per-sample fp64 tensors, by the rules of
    include/scat_mesh_eval.h"""
    out = {k: [] for k in ("mpvpe", "pa", "cnt_raw", "cnt_pa", "n_raw", "n_pa", "f_raw", "f_pa")}
    for lo in range(0, pred.shape[0], CHUNK):
        p, g = pred[lo:lo + CHUNK].double(), gt[lo:lo + CHUNK].double()
        V = p.shape[1]
        mu1, mu2 = p.mean(1, keepdim=True), g.mean(1, keepdim=True)
        X1, X2 = p - mu1, g - mu2
        var1 = (X1 * X1).sum((1, 2))
        K = X1.transpose(1, 2) @ X2
        U, _, Vh = torch.linalg.svd(K)
        Z = torch.diag_embed(torch.stack([torch.ones_like(var1), torch.ones_like(var1), torch.sign(torch.linalg.det(U @ Vh))], 1))
        R = Vh.transpose(1, 2) @ Z @ U.transpose(1, 2)
        scale = torch.diagonal(R @ K, dim1=1, dim2=2).sum(1) / var1
        a = scale[:, None, None] * (X1 @ R.transpose(1, 2)) + mu2
        for name, q in (("raw", p), ("pa", a)):
            d = 1000.0 * (q - g).norm(dim=2)
            out["mpvpe" if name == "raw" else "pa"].append(d.mean(1))
            out["cnt_" + name].append((d[:, :, None] <= th).sum(1).double())
            D = 1000.0 * torch.cdist(q, g)
            n_pred = (D.min(2).values[:, :, None] < fth).sum(1).double()
            n_gt = (D.min(1).values[:, :, None] < fth).sum(1).double()
            out["n_" + name].append(torch.stack([n_pred, n_gt], 2))
            out["f_" + name].append(torch.where(n_pred + n_gt > 0, 2.0 * n_pred * n_gt / (V * (n_pred + n_gt).clamp_min(1.0)),
                                                torch.zeros_like(n_pred)))
    return {k: torch.cat(v) for k, v in out.items()}


def compare(per, ref, T, F):
    """the kernel's per_sample rows against torch_scores -> (count mismatches, worst relative error of the scores)"""
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    tri = per[:, 4 + 2 * T:].reshape(-1, 2, F, 3)
    bad = int((per[:, 4:4 + T] != ref["cnt_raw"]).sum() + (per[:, 4 + T:4 + 2 * T] != ref["cnt_pa"]).sum())
    bad += int((tri[:, 0, :, :2] != ref["n_raw"]).sum() + (tri[:, 1, :, :2] != ref["n_pa"]).sum())
    err = max(rel(per[:, 1], ref["mpvpe"]), rel(per[:, 2], ref["pa"]), rel(tri[:, 0, :, 2], ref["f_raw"]),
              rel(tri[:, 1, :, 2], ref["f_pa"]))
    return bad, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 96, 1024])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=2, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    from scat_amd import ops
    from scat_amd._lib import lib
    from scat_amd.mano import ManoLayer, ManoModel

    lib().scat_check_device()
    dev = torch.device("cuda", 0)
    model = ManoModel.synthetic(1).to(dev)
    layer = ManoLayer(model)
    th32 = torch.linspace(0.5, 50.0, 100, device=dev)
    fth32 = torch.tensor([5.0, 15.0], device=dev)
    th, fth = th32.double(), fth32.double()
    T, F = th.numel(), fth.numel()
    lines = [f"V = {model.V}, T = {T}, F = {F}, {a.repeats} repeats, windows of {a.inner} calls, cases alternated; ms per call, "
             f"device events around the window (host launch time included); {torch.cuda.get_device_name(0)}"]
    failed = False
    for B in a.batches:
        gen = torch.Generator(device=dev).manual_seed(700 + B)
        rnd = lambda *shape: torch.randn(*shape, device=dev, generator=gen)
        # gt: meshes of random hands; pred: the hands of perturbed parameters, moved, and 2 mm of noise per vertex
        par = torch.cat([0.8 * rnd(B, 3), 0.4 * rnd(B, 45), rnd(B, 10)], 1)
        par2 = par + 0.05 * rnd(B, 58)
        with torch.no_grad():
            gt = layer(par[:, :3].contiguous(), par[:, 3:48].contiguous(), par[:, 48:].contiguous())[:, 21:].contiguous()
            pred = layer(par2[:, :3].contiguous(), par2[:, 3:48].contiguous(), par2[:, 48:].contiguous())[:, 21:]
        pred = (pred + 0.01 * rnd(B, 1, 3) + 0.002 * rnd(B, model.V, 3)).contiguous()
        cases = [("kernel", lambda: ops.mesh_eval_accumulate(pred, gt, th32, fth32)[1]),
                 ("torch_fp64", lambda: torch_scores(pred, gt, th, fth))]
        for _ in range(a.warmup):
            for _, fn in cases:
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in cases}
        for _ in range(a.repeats):
            for name, fn in cases:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / a.inner)
        per, ref = cases[0][1](), cases[1][1]()
        bad, err = compare(per, ref, T, F)
        tri = per[:, 4 + 2 * T:].reshape(-1, 2, F, 3)
        ok = bool((per[:, 0] == 0).all()) and bad == 0 and err < 1e-6
        failed = failed or not ok
        lines.append(f"batch {B}: mpvpe {per[:, 1].mean():.3f} mm, pa_mpvpe {per[:, 2].mean():.3f} mm, F@5 raw "
                     f"{tri[:, 0, 0, 2].mean():.4f} aligned {tri[:, 1, 0, 2].mean():.4f}, F@15 raw {tri[:, 0, 1, 2].mean():.4f} "
                     f"aligned {tri[:, 1, 1, 2].mean():.4f}; kernel against torch_fp64: {bad} counts differ, scores within "
                     f"{err:.2e} ({'ok' if ok else 'FAILED'})")
        med = {}
        for name, _ in cases:
            t = sorted(times[name])
            med[name] = statistics.median(t)
            lines.append(f"  {name:12s} median {med[name]:9.4f} ms  min {t[0]:9.4f}  max {t[-1]:9.4f}")
        lines.append(f"  kernel / torch: {med['kernel'] / med['torch_fp64']:.4f}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if failed:
        raise SystemExit("mesh_eval_bench: the kernel's scores and the torch baseline's disagree")


if __name__ == "__main__":
    main()
