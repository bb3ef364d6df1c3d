#!/usr/bin/env python
"""The on-device MANO fit to a track of keypoints in calibrated views (scat_mano_fit_seq_views) with 2 and with 8 cameras,
beside the three ways there were to fit such a clip: V = 778, tracks of 16 frames, S = 1 / 96 / 1024 tracks, 20 iterations,
tools/fit_views_bench.py's method (device events after warm-up around windows of fits, host launch time included, the cases
alternated inside every repeat, median and min..max).

  seq_views_c2   ManoFitter.fit_keypoints_views_sequence, 2 cameras a third of a turn apart, from the triangulated start
  seq_views_c8   the same with 8 cameras an eighth of a turn apart
  frames_c2/c8   (a) ManoFitter.fit_keypoints_views on the same S x 16 frames as one batch: no coupling along t
  tri_seq_c2     (b) ManoFitter.triangulate, then ManoFitter.fit_sequence on the 3-D points, weight 1 for a valid joint
  seq_kp_2d      (c) ManoFitter.fit_keypoints_sequence on camera 0's keypoints (a 640 x 640 frame, trans and log_scale frozen)
  seq_3d         ManoFitter.fit_sequence on the true joints: the neighbouring track kernel, the time to report beside

Then, at the middle batch, what the track buys on keypoints with 1 px of noise and on the same with one frame that only
camera 0 sees: joint RMS and acceleration error against the true joints for the track, (a) and (b).  No time is promised;
the numbers are what a run printed (profiles/fit_seq_views_bench.txt is such a run)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from fit_views_bench import JMAP, rig  # noqa: E402

SMOOTH = dict(rots=30.0, poses=30.0, betas=1e3, trans=3e4, scale=1e3)          # beside pixels squared
SMOOTH_3D = dict(rots=1e-4, poses=1e-4, betas=1e-2, trans=1e-1, scale=1e-1)    # beside metres squared
GAP = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 96, 1024])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=1, help="fits per timed window")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    from scat_amd import synth
    from scat_amd._lib import lib
    from scat_amd.fit import ManoFitter, SequenceFitResult, _groups, free_mask, project_points
    from scat_amd.mano import ManoModel

    lib().scat_check_device()
    dev = torch.device("cuda", 0)
    model = ManoModel.synthetic(1).to(dev)
    T = a.frames
    fitter = ManoFitter(model, joint_map=JMAP, iters=a.iters, w_pose=1e-2, w_beta=1e-2)
    fitter3 = ManoFitter(model, joint_map=JMAP, iters=a.iters)
    T_ = lambda x: torch.from_numpy(np.array(x))
    rigs = {C: rig(C, dev) for C in (2, 8)}
    lines = [f"V = {model.V}, tracks of {T} frames, {a.iters} LM iterations, {a.repeats} repeats, windows of {a.inner} fits, cases "
             f"alternated; ms per fit, device events around the window (host launch time included); {torch.cuda.get_device_name(0)}"]

    def tri_seq(kp, cams, w2=None):
        pts, valid = fitter3.triangulate(kp, cams, w2=w2)
        return fitter3.fit_sequence(pts, weights=valid.float(), smooth=SMOOTH_3D)

    def accel(X, X3):      # the mean over frame triples and joints of the error of the second difference, mm / frame^2
        d = lambda Y: Y[:, 2:] - 2 * Y[:, 1:-1] + Y[:, :-2]
        return 1e3 * (d(X) - d(X3)).norm(dim=3).mean((1, 2))

    rms = lambda X, X3: 1e3 * ((X - X3) ** 2).sum(3).mean(2).sqrt()      # [S,T] mm

    for S in a.batches:
        base = torch.cat([T_(synth.normal_like(190 + S, n, (S, 1, k), s)) for n, k, s in
                          (("rots", 3, 0.8), ("poses", 45, 0.2), ("betas", 10, 1.0), ("trans", 3, 0.02), ("log_scale", 1, 0.1))], dim=2)
        vel = torch.cat([T_(synth.normal_like(191 + S, n, (S, 1, k), s)) for n, k, s in
                         (("vrots", 3, 0.03), ("vposes", 45, 0.03), ("vbetas", 10, 0.0), ("vtrans", 3, 0.002), ("vscale", 1, 0.0))], dim=2)
        true = (base + (torch.arange(T).reshape(1, T, 1) - 0.5 * (T - 1)) * vel).float().to(dev)
        X3 = fitter.joints(SequenceFitResult(*_groups(true), None, None, true))
        kp = {C: project_points(X3.reshape(S * T, 21, 3), rigs[C]).reshape(S, T, C, 21, 2) for C in rigs}
        flat = {C: kp[C].reshape(S * T, C, 21, 2) for C in rigs}
        kp0 = kp[2][:, :, 0].contiguous()
        frozen = free_mask(trans=False, log_scale=False)
        cases = [("seq_views_c2", lambda: fitter.fit_keypoints_views_sequence(kp[2], rigs[2], smooth=SMOOTH)),
                 ("seq_views_c8", lambda: fitter.fit_keypoints_views_sequence(kp[8], rigs[8], smooth=SMOOTH)),
                 ("frames_c2", lambda: fitter.fit_keypoints_views(flat[2], rigs[2])),
                 ("frames_c8", lambda: fitter.fit_keypoints_views(flat[8], rigs[8])),
                 ("tri_seq_c2", lambda: tri_seq(kp[2], rigs[2])),
                 ("seq_kp_2d", lambda: fitter.fit_keypoints_sequence(joints2d=kp0, size=(640, 640), free=frozen,
                                                                     smooth=dict(rots=30.0, poses=30.0, betas=1e3))),
                 ("seq_3d", lambda: fitter3.fit_sequence(X3, smooth=SMOOTH_3D))]
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
        lines.append(f"{S} tracks:")
        med = {}
        for name, fn in cases:
            t = sorted(times[name])
            med[name] = statistics.median(t)
            r = fn()
            if name == "seq_kp_2d":
                what = f"fitted {int(torch.isfinite(r.cost).sum())} of {S} tracks"
            else:
                X = fitter.joints(r).reshape(S, T, 21, 3)
                mm = rms(X, X3).mean(1)
                n = int(torch.isfinite(r.cost).sum())
                what = f"reaches 3-D {mm.median():.4f} ({mm.max():.4f}) mm, median (max) over the tracks; fitted {n} of {r.cost.numel()}"
            lines.append(f"  {name:13s} median {med[name]:10.4f} ms  min {t[0]:10.4f}  max {t[-1]:10.4f}   {what}")
        lines.append("  " + "   ".join(f"seq_views_c2 / {n}: {med['seq_views_c2'] / med[n]:.4f}" for n in ("seq_3d", "frames_c2", "tri_seq_c2", "seq_kp_2d"))
                     + f"   seq_views_c8 / seq_views_c2: {med['seq_views_c8'] / med['seq_views_c2']:.4f}")
        if S != a.batches[len(a.batches) // 2]:
            continue
        noisy = kp[2] + T_(synth.normal_like(193 + S, "noise", tuple(kp[2].shape), 1.0)).float().to(dev)
        w1 = torch.ones(S, T, 2, 21, device=dev)
        w1[:, GAP, 1:] = 0.0
        for tag, w2 in (("1 px of noise", None), (f"1 px of noise, frame {GAP} seen by camera 0 only", w1)):
            tr = fitter.fit_keypoints_views_sequence(noisy, rigs[2], w2=w2, smooth=SMOOTH)
            fr = fitter.fit_keypoints_views(noisy.reshape(S * T, 2, 21, 2), rigs[2], w2=None if w2 is None else w2.reshape(S * T, 2, 21))
            ts = tri_seq(noisy, rigs[2], w2)
            lines.append(f"  C = 2, {tag}; mean over the tracks:")
            for name, r in (("track", tr), ("(a) frames", fr), ("(b) tri + seq", ts)):
                X = fitter.joints(r).reshape(S, T, 21, 3)
                ok = torch.isfinite(r.cost).reshape(S, -1)
                e = rms(X, X3)
                fitted = ok.expand(S, T) if ok.shape[1] == 1 else ok
                lines.append(f"    {name:14s} joint RMS {float(e[fitted].mean()):.4f} mm over the fitted frames, frame {GAP}: "
                             f"{float(e[:, GAP][fitted[:, GAP]].mean()) if bool(fitted[:, GAP].any()) else float('nan'):.4f} mm, "
                             f"acceleration error {float(accel(X, X3).mean()):.4f} mm / frame^2, frames not fitted {int((~fitted).sum())}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
