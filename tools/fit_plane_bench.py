#!/usr/bin/env python
"""The on-device point-to-plane MANO fit against the nearest-vertex fit it stands beside, V = 778, N = 2048 points, batch
1 / 96 / 1024, rounds x iters from a start 0.03 off the truth in every model unknown and 3 mm off in trans: device events
after warm-up, medians over alternated repeats, all columns in the same process.

  (a) fit_points_plane   ManoFitter.fit_points_plane: 2 x rounds + 1 launches
  (b) fit_points         ManoFitter.fit_points at the same rounds x iters: the kernels as they were before this method
  (c) assign_plane       scat_mano_cloud_assign_plane alone at the start, against
      assign             scat_mano_cloud_assign alone: what forming the normals and the metric cost adds to a launch
  (d) fit_metric         scat_mano_fit_verts_metric at rounds x iters iterations on the ordered mesh with its normals, against
      fit_vertices       ManoFitter.fit_vertices at the same iterations: what sqrt(M) on the rows and rho in the cost add

The model is tests/_fit_plane_cases.smooth_model (the hand surface of tests/golden/hand_mesh.npz, so that a cloud drawn on
the faces of the posed mesh is what a depth camera gives); its skinning weights are dense, 16 per vertex against MANO's
4, and all columns run on this one model.  Every case is a window of ``inner`` calls between two events (host launch time included); the cases
alternate inside every repeat so that drift hits all alike.  The transform of the rows is applied by the work-item that wrote
them (no barrier added); a separate pass with one more barrier per tile was not built, so there is one number, not two.

--sweep adds, at batch 96, the vertex RMS against the true mesh (median over the batch) after k = 1 .. 20 rounds of both
methods, the first k from which a method stays within 10 % of its own RMS after 20 rounds, and the time of a call with
that many rounds: the figure that decides between them.  --out also writes the table to a file
(profiles/fit_plane_bench.txt is such a run)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))

T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def timed(cases, repeats, inner, warmup):
    """-> {name: sorted ms per call}: windows of `inner` calls between two events, the cases alternated in every repeat"""
    for _ in range(warmup):
        for _, fn in cases:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cases}
    for _ in range(repeats):
        for name, fn in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner)
    return {k: sorted(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true", help="also the rounds each method needs to reach its plateau, and their time")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 96, 1024])
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--tau", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=4, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import _fit_plane_cases as G
    import _fit_verts_oracle as VO
    from scat_amd import synth
    from scat_amd._lib import lib
    from scat_amd.fit import ManoFitter, mano_cloud_assign, mano_cloud_assign_plane, mano_fit_verts_metric, mesh_normals

    lib().scat_check_device()
    dev = torch.device("cuda", 0)
    host = G.smooth_model()
    model = host.to(dev)
    fitter = ManoFitter(model)
    faces = G.topology(778)[0]
    topo = fitter._topology("fit_plane_bench", faces, dev)
    steps, N = a.rounds * a.iters, a.points
    lines = [f"V = {model.V}, F = {len(faces)}, N = {N} points on the faces, {a.rounds} rounds x {a.iters} LM iterations, w_tangent {a.tau}, "
             f"{a.repeats} repeats, windows of {a.inner} calls, {a.warmup} warm-up calls of every case, cases alternated; ms per call, "
             f"device events around the window (host launch time included); {torch.cuda.get_device_name(0)}"]

    def rms(P, mesh):
        return VO.rms(host, P.cpu(), mesh) * 1e3

    for B in a.batches:
        true = np.concatenate([synth.normal_like(190 + B, n, (B, k), s) for n, k, s in
                               (("rots", 3, 0.8), ("poses", 45, 0.25), ("betas", 10, 1.0), ("trans", 3, 0.05), ("log_scale", 1, 0.1))],
                              axis=1).astype(np.float32)
        mesh64 = []
        with torch.no_grad():
            for b0 in range(0, B, 128):
                mesh64.append(VO.model_verts(host, T_(true[b0:b0 + 128]).double()))
        mesh64 = torch.cat(mesh64)
        pts = T_(G.surface_cloud(mesh64.numpy(), faces.astype(np.int64), N, 191 + B)).to(dev)
        P0 = true.copy()
        P0[:, :58] += 0.03 * synth.normal_like(192 + B, "fit.off", (B, 58), 1.0)
        P0[:, 58:61] += 0.003 * synth.normal_like(192 + B, "fit.trans", (B, 3), 1.0)
        P0 = T_(P0.astype(np.float32)).to(dev)
        Tv = mesh64.float().to(dev)
        Tn = mesh_normals(Tv, topo)
        inf = float("inf")
        plane = lambda k=a.rounds: fitter.fit_points_plane(pts, P0, faces, rounds=k, iters=a.iters, w_tangent=a.tau).p
        near = lambda k=a.rounds: fitter.fit_points(pts, P0, rounds=k, iters=a.iters).p

        def metric():
            p = P0.clone()
            mano_fit_verts_metric(model, Tv, None, Tn, p, steps, a.tau, fitter.lambda0, fitter.w_pose, fitter.w_beta)
            return p

        cases = [("fit_points_plane", plane), ("fit_points", near),
                 ("assign_plane", lambda: mano_cloud_assign_plane(model, P0, pts, None, topo, inf, a.tau)[0].idx),
                 ("assign", lambda: mano_cloud_assign(model, P0, pts, None, inf).idx),
                 ("fit_metric", metric), ("fit_vertices", lambda: fitter.fit_vertices(Tv, init=P0, iters=steps).p)]
        times = timed(cases, a.repeats, a.inner, a.warmup)
        reached = [("start", rms(P0, mesh64))] + [(name, rms(fn(), mesh64)) for name, fn in cases if not name.startswith("assign")]
        lines.append(f"batch {B}: vertex RMS against the true mesh in mm, median (max) over the batch: " +
                     "; ".join(f"{name} {r.median():.4f} ({r.max():.4f})" for name, r in reached))
        med = {}
        for name, _ in cases:
            t = times[name]
            med[name] = statistics.median(t)
            lines.append(f"  {name:17s} median {med[name]:10.4f} ms  min {t[0]:10.4f}  max {t[-1]:10.4f}")
        lines.append(f"  (a) / (b) fit_points_plane / fit_points: {med['fit_points_plane'] / med['fit_points']:.3f}; (c) assign_plane / assign: "
                     f"{med['assign_plane'] / med['assign']:.3f}; (d) fit_metric / fit_vertices: {med['fit_metric'] / med['fit_vertices']:.3f}")
        if a.sweep and B == 96:
            ks = list(range(1, 21))
            curve = {name: [float(rms(fn(k), mesh64).median()) for k in ks] for name, fn in (("fit_points_plane", plane), ("fit_points", near))}
            need = {}
            for name, r in curve.items():
                need[name] = next(k for i, k in enumerate(ks) if all(v <= 1.1 * r[-1] for v in r[i:]))
                lines.append(f"  sweep {name}: median vertex RMS in mm after k rounds x {a.iters}: " + " ".join(f"{v:.3f}" for v in r))
            sweep_cases = [(f"{name} x {need[name]}", (lambda fn=fn, k=need[name]: fn(k))) for name, fn in
                           (("fit_points_plane", plane), ("fit_points", near))]
            ts = timed(sweep_cases, a.repeats, a.inner, a.warmup)
            for (label, _), name in zip(sweep_cases, curve):
                lines.append(f"  sweep {name}: within 10 % of its own plateau ({curve[name][-1]:.3f} mm after 20 rounds) from {need[name]} "
                             f"rounds, which take {statistics.median(ts[label]):.4f} ms (min {ts[label][0]:.4f}, max {ts[label][-1]:.4f})")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
