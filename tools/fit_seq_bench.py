#!/usr/bin/env python
"""The sequence fit against the per-frame fit on the same frames, V = 778, 20 iterations from the same start: device
events after warm-up, medians over alternated repeats (the method of tools/fit_bench.py).

  fit_sequence  ManoFitter.fit_sequence on [S,T,21,3]: one launch (scat_mano_fit_seq), one workgroup per sequence walking
                its T frames three times per iteration (assemble and factor, back-substitute, trial cost); the
                allocation of the workspace is inside the window
  fit           ManoFitter.fit on the same S T frames as one batch [S T,21,3]: one workgroup per frame, no coupling

The two do not compute the same thing: the second is what the first replaces on a track, and the ratio is the price of
the coupling, of walking the frames in order inside one workgroup, and of the factors' round trip through the
workspace.  Every case is a window of ``inner`` fits between two events (host launch time included); the cases
alternate inside every repeat.  No ratio is gated.  With --out also writes the table to a file
(profiles/fit_seq_bench.txt is such a run)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))
SMOOTH = dict(rots=1e-3, poses=1e-4, betas=1e-2, trans=1e-1, scale=1e-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 16, 96, 16, 1024, 16, 1, 256], help="S T pairs")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=1, help="fits per timed window")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    from scat_amd import synth
    from scat_amd._lib import lib
    from scat_amd.fit import ManoFitter
    from scat_amd.mano import ManoModel, mano_fwd

    L = lib()
    L.scat_check_device()
    dev = torch.device("cuda", 0)
    model = ManoModel.synthetic(1).to(dev)
    jmap = (0, 13, 14, 15, 20, 1, 2, 3, 16, 4, 5, 6, 17, 10, 11, 12, 19, 7, 8, 9, 18)
    fitter = ManoFitter(model, joint_map=jmap, iters=a.iters)
    lines = [f"V = {model.V}, {a.iters} LM iterations, {a.repeats} repeats, windows of {a.inner} fits, cases alternated; ms per "
             f"fit, device events around the window (host launch time included); smooth {SMOOTH}; "
             f"{torch.cuda.get_device_name(0)}"]
    for S, T in zip(a.shapes[::2], a.shapes[1::2]):
        base = torch.cat([T_(synth.normal_like(70 + S + T, n, (S, 1, k), s)) for n, k, s in
                          (("rots", 3, 0.8), ("poses", 45, 0.4), ("betas", 10, 1.0), ("trans", 3, 0.05), ("log_scale", 1, 0.2))], dim=2)
        vel = torch.cat([T_(synth.normal_like(71 + S + T, n, (S, 1, k), s)) for n, k, s in
                         (("rots", 3, 0.01), ("poses", 45, 0.005), ("betas", 10, 0.0), ("trans", 3, 0.001), ("log_scale", 1, 0.0))], dim=2)
        t = torch.linspace(-1.0, 1.0, T).reshape(1, T, 1) * (0.5 * min(T, 32))      # the same excursion for every T >= 32
        true = (base + t * vel).float().reshape(S * T, 62).to(dev)
        out = mano_fwd(model, true[:, 0:3].contiguous(), true[:, 3:48].contiguous(), true[:, 48:58].contiguous())[:, :21]
        X = (torch.exp(true[:, 61]).reshape(-1, 1, 1) * out[:, list(jmap)] + true[:, None, 58:61]).contiguous()
        Xs = X.reshape(S, T, 21, 3)
        P0 = fitter.fit_sequence(Xs, smooth=SMOOTH, iters=1, free=0).p      # the start, nothing solved for
        P0f = P0.reshape(S * T, 62)
        cases = [("fit_sequence", lambda: fitter.fit_sequence(Xs, smooth=SMOOTH, init=P0)),
                 ("fit", lambda: fitter.fit(X, init=P0f))]
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
        rs, rf = cases[0][1](), cases[1][1]()

        def rms(J):
            d = J.reshape(S * T, 21, 3) - X
            return (d * d).sum(2).mean(1).sqrt() * 1e3

        ra, rb = rms(fitter.joints(rs)), rms(fitter.joints(rf))
        lines.append(f"S {S} T {T} ({S * T} frames, workspace {int(L.scat_mano_fit_seq_ws(S, T)) / 2 ** 20:.1f} MiB): joint RMS in mm, "
                     f"median (max) over the frames: fit_sequence {ra.median():.4f} ({ra.max():.4f}), fit {rb.median():.4f} "
                     f"({rb.max():.4f}); accepted steps, min over the sequences {int(rs.accepted.min())}")
        med = {}
        for name, _ in cases:
            ts = sorted(times[name])
            med[name] = statistics.median(ts)
            lines.append(f"  {name:12s} median {med[name]:10.4f} ms  min {ts[0]:10.4f}  max {ts[-1]:10.4f}")
        lines.append(f"  fit_sequence / fit: {med['fit_sequence'] / med['fit']:.2f}; fit_sequence / (T x iterations): "
                     f"{1e3 * med['fit_sequence'] / (T * a.iters):.1f} us")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
