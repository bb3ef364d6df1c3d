#!/usr/bin/env python
"""The on-device MANO fit to a point cloud, V = 778, N = 2048 points, batch 1 / 96 / 1024, 5 rounds x 4 iterations from
a start 0.03 off the truth in every model unknown: device events after warm-up, medians over alternated repeats, all
columns in the same process.

  fit_points    ManoFitter.fit_points: 2 x rounds + 1 launches (scat_mano_cloud_assign, scat_mano_fit_verts, ...)
  assign        the assignment launch alone (scat_mano_cloud_assign at the start): pose V vertices, N x V fp64 distances,
                the per-vertex reduction
  fit_vertices  ManoFitter.fit_vertices at rounds x iters iterations on the ordered mesh of the same hands from the same
                start: what the fit costs when the correspondences are known
  torch_icp64   the same ICP loop in fp64 torch on the device: the assignment as a [b, N, V] distance table (argmin,
                scatter_add), tools/fit_verts_bench.py's Levenberg-Marquardt with per-vertex weights; no host
                synchronisation inside the loop, the batch in chunks of 64 hands for the table; timed in 3 of the repeats

The cloud: every point is a random vertex of the hand's true mesh plus 1 mm of noise.  Every case is a window of
``inner`` calls between two events (host launch time included); the cases alternate inside every repeat so that drift
hits all alike.  With --out also writes the table to a file (profiles/fit_points_bench.txt is such a run).

--sweep times the assignment alone on 96 hands of random vertices (scat_cloud_assign, no posing) at sizes chosen to take
its three phases apart: V = 512 against 513 adds one scan of the index array per thread and next to no walk; max_dist
tiny against inf removes the reduction's loads and sums (nothing is matched) and keeps walk and scans; N and V doubled
scale the walk by N V."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)

T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def torch_icp(plain, pts, P0, rounds, iters, chunk=64):
    """plain: fit_verts_bench.TorchLM64; pts [B,N,3] fp64, P0 [B,62] fp64 -> P"""
    out = []
    for b0 in range(0, P0.shape[0], chunk):
        P, q = P0[b0:b0 + chunk].clone(), pts[b0:b0 + chunk]
        B, N = q.shape[:2]
        for _ in range(rounds):
            with torch.no_grad():
                x = torch.exp(P[:, 61]).reshape(-1, 1, 1) * plain.verts(P) + P[:, None, 58:61]
                d = q.unsqueeze(2) - x.unsqueeze(1)
                idx = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).argmin(2)
                del d
                W = torch.zeros(B, x.shape[1], dtype=torch.float64, device=q.device).scatter_add_(1, idx, torch.ones_like(q[..., 0]))
                S = torch.zeros_like(x).scatter_add_(1, idx.unsqueeze(2).expand(B, N, 3), q)
                tgt = S / W.clamp_min(1.0).unsqueeze(2)
            P = fit_weighted(plain, tgt, W, P, iters)
        out.append(P)
    return torch.cat(out)


def fit_weighted(plain, T, w, P0, iters):
    """TorchLM64.fit with per-vertex weights"""
    P, B = P0.clone(), P0.shape[0]
    V, dev = T.shape[1], P0.device
    wr = w.repeat_interleave(3, dim=1)
    lam = torch.full((B,), plain.lambda0, dtype=torch.float64, device=dev)
    eye3 = torch.eye(3, dtype=torch.float64, device=dev).repeat(V, 1).unsqueeze(0)
    eye = torch.eye(62, dtype=torch.float64, device=dev).expand(B, 62, 62)
    zero = torch.zeros(58, dtype=torch.float64, device=dev)

    def cost(Q):
        with torch.no_grad():
            r = (torch.exp(Q[:, 61]).reshape(-1, 1, 1) * plain.verts(Q) + Q[:, None, 58:61] - T).reshape(B, 3 * V)
        return (wr * r * r).sum(1) + plain.w_pose * (Q[:, 3:48] ** 2).sum(1) + plain.w_beta * (Q[:, 48:58] ** 2).sum(1)

    for _ in range(iters):
        Pm, pad = P[:, :58].detach(), P[:, 58:].detach()
        jm = torch.autograd.functional.jacobian(lambda e: plain.verts(torch.cat([Pm + e, pad], dim=1)), zero,
                                                strategy="forward-mode", vectorize=True).reshape(B, 3 * V, 58)
        with torch.no_grad():
            x = plain.verts(P)
        s = torch.exp(P[:, 61]).reshape(B, 1, 1)
        J = torch.cat([s * jm, eye3.expand(B, 3 * V, 3), (s * x).reshape(B, 3 * V, 1)], dim=2)
        r = (s * x + P[:, None, 58:61] - T).reshape(B, 3 * V)
        A = J.transpose(1, 2) @ (wr.unsqueeze(2) * J) + torch.diag(plain.prior)
        g = (J.transpose(1, 2) @ (wr * r).unsqueeze(2)).squeeze(2) + plain.prior * P
        L, info = torch.linalg.cholesky_ex(A + lam.reshape(B, 1, 1) * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2)))
        ok = info == 0
        Pt = P - torch.cholesky_solve(g.unsqueeze(2), torch.where(ok.reshape(B, 1, 1), L, eye)).squeeze(2)
        take = ok & torch.isfinite(Pt).all(1) & (cost(Pt) < cost(P))
        P = torch.where(take.unsqueeze(1), Pt, P)
        lam = torch.where(take, (lam * 0.1).clamp_min(1e-12), (lam * 10).clamp_max(1e12))
    return P


def sweep(lines, repeats, inner):
    from scat_amd import synth
    from scat_amd.fit import cloud_assign

    B, dev = 96, torch.device("cuda", 0)
    rows = [(N, V, md) for N, V in ((2048, 256), (2048, 512), (2048, 513), (2048, 768), (2048, 778), (2048, 1536), (1024, 512),
                                    (4096, 512), (8192, 1536)) for md in (float("inf"), 1e-9)]
    data = {}
    for N, V, _ in rows:
        if (N, V) not in data:
            verts = T_(synth.normal_like(7, "sweep.verts", (B, V, 3), 0.1)).to(dev)
            pick = torch.from_numpy(np.random.default_rng(N + V).integers(0, V, size=(B, N))).to(dev)
            data[(N, V)] = (verts, (torch.gather(verts, 1, pick.unsqueeze(2).expand(B, N, 3)) +
                                    T_(synth.normal_like(8, "sweep.noise", (B, N, 3), 5e-3)).to(dev)).contiguous())
    run = lambda N, V, md: cloud_assign(*data[(N, V)], None, md).idx
    for r in rows:
        run(*r)
    torch.cuda.synchronize()
    times = {r: [] for r in rows}
    for _ in range(repeats):
        for r in rows:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                run(*r)
            e1.record()
            e1.synchronize()
            times[r].append(e0.elapsed_time(e1) / inner)
    lines.append(f"sweep: scat_cloud_assign alone, {B} hands of random vertices, ms per launch, median of {repeats} windows of {inner}")
    for N, V, md in rows:
        lines.append(f"  N {N:5d} V {V:5d} max_dist {md:g}: {statistics.median(times[(N, V, md)]):8.4f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true", help="also time the assignment alone over N, V and max_dist")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 96, 1024])
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=4, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-torch", action="store_true", help="leave the fp64 torch loop out")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    from fit_verts_bench import TorchLM64
    from scat_amd import synth
    from scat_amd._lib import lib
    from scat_amd.fit import ManoFitter, mano_cloud_assign
    from scat_amd.mano import ManoLayer, ManoModel

    lib().scat_check_device()
    dev = torch.device("cuda", 0)
    host = ManoModel.synthetic(1)
    model = ManoModel.synthetic(1).to(dev)
    fitter = ManoFitter(model)
    layer = ManoLayer(model)
    plain = TorchLM64(host, fitter.w_pose, fitter.w_beta, fitter.lambda0, dev)
    steps, N = a.rounds * a.iters, a.points
    lines = [f"V = {model.V}, N = {N} points, {a.rounds} rounds x {a.iters} LM iterations, {a.repeats} repeats, windows of {a.inner} "
             f"calls (torch_icp64: 1), cases alternated; ms per call, device events around the window (host launch time "
             f"included); {torch.cuda.get_device_name(0)}"]
    for B in a.batches:
        true = torch.cat([T_(synth.normal_like(90 + B, n, (B, k), s)) for n, k, s in
                          (("rots", 3, 0.8), ("poses", 45, 0.4), ("betas", 10, 1.0), ("trans", 3, 0.05), ("log_scale", 1, 0.2))],
                         dim=1).to(dev)
        with torch.no_grad():
            out = torch.exp(true[:, 61]).reshape(-1, 1, 1) * layer(true[:, 0:3].contiguous(), true[:, 3:48].contiguous(),
                                                                    true[:, 48:58].contiguous()) + true[:, None, 58:61]
        Tv = out[:, 21:].contiguous()
        pick = torch.from_numpy(np.random.default_rng(90 + B).integers(0, model.V, size=(B, N))).to(dev)
        pts = (torch.gather(Tv, 1, pick.unsqueeze(2).expand(B, N, 3)) +
               T_(synth.normal_like(91 + B, "cloud.noise", (B, N, 3), 1e-3)).to(dev)).contiguous()
        P0 = true.clone()
        P0[:, :58] += 0.03 * T_(synth.normal_like(92 + B, "fit.off", (B, 58), 1.0)).to(dev)
        cases = [("fit_points", lambda: fitter.fit_points(pts, P0, rounds=a.rounds, iters=a.iters).p),
                 ("assign", lambda: mano_cloud_assign(model, P0, pts, None, float("inf")).idx),
                 ("fit_vertices", lambda: fitter.fit_vertices(Tv, init=P0, iters=steps).p)]
        if not a.no_torch:
            pts64, P064 = pts.double(), P0.double()
            cases.append(("torch_icp64", lambda: torch_icp(plain, pts64, P064, a.rounds, a.iters)))
        inner = {name: 1 if name == "torch_icp64" else a.inner for name, _ in cases}
        for _ in range(a.warmup):
            for _, fn in cases:
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in cases}
        for rep in range(a.repeats):
            for name, fn in cases:
                if name == "torch_icp64" and rep >= 3:
                    continue
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner[name]):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / inner[name])

        def rms(P):
            with torch.no_grad():
                d = torch.exp(P[:, 61]).reshape(-1, 1, 1) * plain.verts(P.double()) + P[:, None, 58:61].double() - Tv.double()
            return (d * d).sum(2).mean(1).sqrt() * 1e3

        reached = [("start", rms(P0))] + [(name, rms(fn())) for name, fn in cases if name != "assign"]
        lines.append(f"batch {B}: vertex RMS against the true mesh in mm, median (max) over the batch: " +
                     "; ".join(f"{name} {r.median():.4f} ({r.max():.4f})" for name, r in reached))
        med = {}
        for name, _ in cases:
            t = sorted(times[name])
            med[name] = statistics.median(t)
            lines.append(f"  {name:14s} median {med[name]:10.4f} ms  min {t[0]:10.4f}  max {t[-1]:10.4f}")
        rnd = (med["fit_points"] - med["assign"]) / a.rounds
        lines.append(f"  a round (assign + {a.iters} iterations): {rnd:.4f} ms, the assign {med['assign'] / rnd:.3f} of it; fit_points / "
                     f"fit_vertices at {steps} iterations: {med['fit_points'] / med['fit_vertices']:.2f}" +
                     ("" if a.no_torch else f"; fit_points / torch_icp64: {med['fit_points'] / med['torch_icp64']:.5f}"))
    if a.sweep:
        sweep(lines, a.repeats, 8)
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
