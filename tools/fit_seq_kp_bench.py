#!/usr/bin/env python
"""The keypoint-track fit against the two fits it composes, on the same frames, V = 778, 20 iterations from the same start:
device events after warm-up, medians over alternated repeats (the method of tools/fit_seq_bench.py), all columns from one
process on one box.

  (a) fit_keypoints_sequence  both terms, [S,T,21,3] and [S,T,21,2]: one launch (scat_mano_fit_seq_kp), one workgroup per
                              sequence walking its T frames three times per iteration; the workspace's allocation is inside
                              the window
  (b) fit_keypoints           the same S T frames as one batch, both terms: one workgroup per frame, no coupling
  (c) fit_sequence            the 3-D part of the same tracks alone: scat_mano_fit_seq, 62 unknowns, no camera

None computes what another does: (b) is what (a) replaces on a track, (c) is (a) without the 2-D term and the camera, and
the ratios are the price of the coupling and of the larger frame.  With --sweep, (a) is also timed with parts of a frame
switched off by its arguments (no 2-D term and a frozen camera; no smoothness, which leaves M_t zero but still walked), to
say which part of a frame's walk carries the difference to (c).  No ratio is gated.  With --out also writes the table to
a file (profiles/fit_seq_kp_bench.txt is such a run)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))
SMOOTH = dict(rots=1e-3, poses=1e-4, betas=1e-2, trans=1e-1, scale=1e-1)
SMOOTH_KP = dict(SMOOTH, cam_scale=1e-3, cam_trans=1e-1)
W2 = 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 16, 96, 16, 1024, 16], help="S T pairs")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sweep", action="store_true", help="also time (a) with parts of a frame switched off")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    from scat_amd import synth
    from scat_amd._lib import lib
    from scat_amd.fit import FIT_SEQ_KP_HEADER, ManoFitter
    from scat_amd.mano import ManoModel, mano_fwd
    from scat_amd.render import project_outputs

    L = lib()
    L.scat_check_device()
    ws_query = L.bind(FIT_SEQ_KP_HEADER).scat_mano_fit_seq_kp_ws
    dev = torch.device("cuda", 0)
    model = ManoModel.synthetic(1).to(dev)
    jmap = (0, 13, 14, 15, 20, 1, 2, 3, 16, 4, 5, 6, 17, 10, 11, 12, 19, 7, 8, 9, 18)
    fitter = ManoFitter(model, joint_map=jmap, iters=a.iters)
    lines = [f"V = {model.V}, {a.iters} LM iterations, {a.repeats} repeats, one fit per window, cases alternated; ms per fit, device "
             f"events around the window (host launch time included); smooth {SMOOTH_KP}, w2 {W2}; "
             f"{torch.cuda.get_device_name(0)}"]
    for S, T in zip(a.shapes[::2], a.shapes[1::2]):
        base = torch.cat([T_(synth.normal_like(70 + S + T, n, (S, 1, k), s)) for n, k, s in
                          (("rots", 3, 0.8), ("poses", 45, 0.4), ("betas", 10, 1.0), ("trans", 3, 0.05), ("log_scale", 1, 0.2))], dim=2)
        vel = torch.cat([T_(synth.normal_like(71 + S + T, n, (S, 1, k), s)) for n, k, s in
                         (("rots", 3, 0.01), ("poses", 45, 0.005), ("betas", 10, 0.0), ("trans", 3, 0.001), ("log_scale", 1, 0.0))], dim=2)
        t = torch.linspace(-1.0, 1.0, T).reshape(1, T, 1) * (0.5 * min(T, 32))
        true = (base + t * vel).float().reshape(S * T, 62).to(dev)
        out = mano_fwd(model, true[:, 0:3].contiguous(), true[:, 3:48].contiguous(), true[:, 48:58].contiguous())[:, :21]
        X = (torch.exp(true[:, 61]).reshape(-1, 1, 1) * out[:, list(jmap)] + true[:, None, 58:61]).contiguous()
        cam = torch.tensor([4.0, 0.02, -0.03], device=dev).expand(S * T, 3)
        U = project_outputs(torch.cat([cam, X.reshape(S * T, 63)], dim=1), 224, 224).contiguous()
        Xs, Us = X.reshape(S, T, 21, 3), U.reshape(S, T, 21, 2)
        w2 = torch.full((S, T, 21), W2, device=dev)
        P0 = fitter.fit_keypoints_sequence(Xs, Us, w2=w2, smooth=SMOOTH_KP, iters=1, free=0, free_cam=0).p      # the start
        P0f, P0s = P0.reshape(S * T, 65), P0[..., :62].contiguous()
        w2f = w2.reshape(S * T, 21)
        cases = [("a seq_kp", lambda: fitter.fit_keypoints_sequence(Xs, Us, w2=w2, smooth=SMOOTH_KP, init=P0)),
                 ("b kp", lambda: fitter.fit_keypoints(X, U, w2=w2f, init=P0f)),
                 ("c seq", lambda: fitter.fit_sequence(Xs, smooth=SMOOTH, init=P0s))]
        if a.sweep:
            cases += [("a no 2-D", lambda: fitter.fit_keypoints_sequence(Xs, smooth=SMOOTH_KP, init=P0, free_cam=0)),
                      ("a no smooth", lambda: fitter.fit_keypoints_sequence(Xs, Us, w2=w2, init=P0))]
        for _ in range(a.warmup):
            for _, fn in cases:
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in cases}
        for _ in range(a.repeats):
            for name, fn in cases:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        ra, rb, rc = (fn() for _, fn in cases[:3])

        def rms(J):
            dd = J.reshape(S * T, 21, 3) - X
            return (dd * dd).sum(2).mean(1).sqrt() * 1e3

        qa, qb, qc = rms(fitter.joints(ra)), rms(fitter.joints(rb)), rms(fitter.joints(rc))
        lines.append(f"S {S} T {T} ({S * T} frames, workspace {int(ws_query(S, T)) / 2 ** 20:.1f} MiB): joint RMS in mm, median (max) over "
                     f"the frames: a {qa.median():.4f} ({qa.max():.4f}), b {qb.median():.4f} ({qb.max():.4f}), c {qc.median():.4f} "
                     f"({qc.max():.4f}); accepted steps, min over the sequences: a {int(ra.accepted.min())}, c {int(rc.accepted.min())}")
        med = {}
        for name, _ in cases:
            ts = sorted(times[name])
            med[name] = statistics.median(ts)
            lines.append(f"  {name:12s} median {med[name]:10.4f} ms  min {ts[0]:10.4f}  max {ts[-1]:10.4f}")
        lines.append(f"  a / b: {med['a seq_kp'] / med['b kp']:.2f}; a / c: {med['a seq_kp'] / med['c seq']:.2f}; a / (T x iterations): "
                     f"{1e3 * med['a seq_kp'] / (T * a.iters):.1f} us, c / (T x iterations): {1e3 * med['c seq'] / (T * a.iters):.1f} us")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
