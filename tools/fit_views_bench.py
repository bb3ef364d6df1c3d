#!/usr/bin/env python
"""The on-device MANO fit to keypoints in calibrated views (scat_mano_fit_views) with 2 and with 8 cameras, beside
fit_keypoints on the same hands seen by the first camera: V = 778, batch 1 / 96 / 1024, 20 iterations, tools/fit_bench.py's
method (device events after warm-up around windows of fits, host launch time included, the cases alternated inside every
repeat, median and min..max).

  views_c2      ManoFitter.fit_keypoints_views, 2 cameras a third of a turn apart, from the triangulated start
  views_c8      the same with 8 cameras an eighth of a turn apart
  views_c8_gm   the same with the Geman-McClure loss (sigma2 = 10 px)
  kp_2d         ManoFitter.fit_keypoints on the keypoints of camera 0 (its pixels as a 640 x 640 frame's), from its own
                closed-form start, trans and log_scale frozen: the weak-perspective fit that one view allows
  triangulate   ManoFitter.triangulate with 8 cameras, alone

The claim to check is that C = 8 costs little more than C = 2: the views are summed into a 3 x 3 matrix per joint by 21
threads before the 256 assemble the normal equations.  No time is promised; the numbers are what a run printed
(profiles/fit_views_bench.txt is such a run)."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

JMAP = (0, 13, 14, 15, 20, 1, 2, 3, 16, 4, 5, 6, 17, 10, 11, 12, 19, 7, 8, 9, 18)


def look_at(phi, radius=0.5):
    o = radius * np.array([math.cos(phi), 0.0, math.sin(phi)])
    z = -o / np.linalg.norm(o)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R, -R @ o


def rig(C, dev):
    from scat_amd.fit import Cameras

    Rt = [look_at(0.3 + c * 2 * math.pi / max(C, 3)) for c in range(C)]
    f = lambda a: torch.tensor(np.array(a), dtype=torch.float32, device=dev).unsqueeze(0)
    return Cameras(f([r for r, _ in Rt]), f([t for _, t in Rt]), f([[600.0, 600.0, 320.0, 240.0]] * C))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 96, 1024])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=2, help="fits per timed window")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    from scat_amd import synth
    from scat_amd._lib import lib
    from scat_amd.fit import FitResult, ManoFitter, _groups, free_mask, project_points
    from scat_amd.mano import ManoModel

    lib().scat_check_device()
    dev = torch.device("cuda", 0)
    model = ManoModel.synthetic(1).to(dev)
    fitter = ManoFitter(model, joint_map=JMAP, iters=a.iters, w_pose=1e-2, w_beta=1e-2)
    T_ = lambda x: torch.from_numpy(np.array(x))
    rigs = {C: rig(C, dev) for C in (2, 8)}
    lines = [f"V = {model.V}, {a.iters} LM iterations, {a.repeats} repeats, windows of {a.inner} fits, cases alternated; ms per "
             f"fit, device events around the window (host launch time included); {torch.cuda.get_device_name(0)}"]
    for B in a.batches:
        true = torch.cat([T_(synth.normal_like(190 + B, n, (B, k), s)) for n, k, s in
                          (("rots", 3, 0.8), ("poses", 45, 0.2), ("betas", 10, 1.0), ("trans", 3, 0.02), ("log_scale", 1, 0.1))],
                         dim=1).float().to(dev)
        truth = FitResult(*_groups(true), None, None, true)
        X3 = fitter.joints(truth)
        kp = {C: project_points(X3, rigs[C]) for C in rigs}
        kp0 = kp[2][:, 0].contiguous()
        frozen = free_mask(trans=False, log_scale=False)
        cases = [("views_c2", lambda: fitter.fit_keypoints_views(kp[2], rigs[2])),
                 ("views_c8", lambda: fitter.fit_keypoints_views(kp[8], rigs[8])),
                 ("views_c8_gm", lambda: fitter.fit_keypoints_views(kp[8], rigs[8], sigma2=10.0)),
                 ("kp_2d", lambda: fitter.fit_keypoints(joints2d=kp0, size=(640, 640), free=frozen)),
                 ("triangulate", lambda: fitter.triangulate(kp[8], rigs[8]))]
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
        lines.append(f"batch {B}:")
        med = {}
        for name, fn in cases:
            t = sorted(times[name])
            med[name] = statistics.median(t)
            r = fn()
            if name.startswith("views"):
                C = 2 if name == "views_c2" else 8
                px = ((fitter.project_views(r, rigs[C]) - kp[C]) ** 2).sum(3).flatten(1).mean(1).sqrt()
                mm = 1e3 * ((fitter.joints(r) - X3) ** 2).sum(2).mean(1).sqrt()
                what = (f"reaches, median (max) over the batch: 3-D {mm.median():.4f} ({mm.max():.4f}) mm, 2-D {px.median():.4f} "
                        f"({px.max():.4f}) px, fitted {int(torch.isfinite(r.cost).sum())} of {B}")
            elif name == "kp_2d":
                px = ((fitter.project(r, (640, 640)) - kp0) ** 2).sum(2).mean(1).sqrt()
                what = f"reaches 2-D {px.median():.4f} ({px.max():.4f}) px in its one view"
            else:
                what = f"{int(r[1].sum())} of {21 * B} joints, largest error {1e3 * float((r[0] - X3).abs().max()):.5f} mm"
            lines.append(f"  {name:11s} median {med[name]:9.4f} ms  min {t[0]:9.4f}  max {t[-1]:9.4f}   {what}")
        lines.append(f"  views_c8 / views_c2: {med['views_c8'] / med['views_c2']:.4f}   views_c2 / kp_2d: {med['views_c2'] / med['kp_2d']:.4f}"
                     f"   views_c8_gm / views_c8: {med['views_c8_gm'] / med['views_c8']:.4f}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
