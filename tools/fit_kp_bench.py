#!/usr/bin/env python
"""The on-device MANO fit to keypoints (scat_mano_fit_kp) against scat_mano_fit and against a torch loop, V = 778, batch
1 / 96 / 1024, 20 iterations from the same start: tools/fit_bench.py's method (device events after warm-up around windows
of fits, host launch time included, the cases alternated inside every repeat, median and min..max).

  mano_fit      ManoFitter.fit: scat_mano_fit on the 3-D joints
  kp_3d         ManoFitter.fit_keypoints on the same 3-D joints with the 2-D term off: the new kernel on the old problem
  kp_both       fit_keypoints with the 3-D joints and their 2-D projections (w2 = 1e-6), the camera solved for
  kp_2d_gm      fit_keypoints with the 2-D keypoints alone, Geman-McClure (sigma2 = 10 px), trans and log_scale frozen
  torch_lm      kp_both's problem written with ManoLayer and torch.linalg in fp32 on the device (tools/fit_bench.py's
                TorchLM with the 42 reprojection rows and the three camera columns added)

No ratio is gated; the numbers are what a run printed (profiles/fit_kp_bench.txt is such a run)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fit_bench import T_, TorchLM  # noqa: E402

HALF = 112.0


class TorchLMKp(TorchLM):
    """include/scat_mano_fit_kp.h with both terms, quadratic, no limits: 105 rows, 65 unknowns"""

    def __init__(self, *a, w2=1e-6):
        super().__init__(*a)
        self.w2 = w2
        self.prior = torch.cat([self.prior, torch.zeros(3, device=self.dev)])
        self.wr = torch.cat([torch.ones(63, device=self.dev), torch.full((42,), w2, device=self.dev)])

    def rows(self, P, T3, T2):
        m = torch.exp(P[:, 61]).reshape(-1, 1, 1) * self.joints(P)[:, self.jm] + P[:, None, 58:61]
        u = (P[:, 62].reshape(-1, 1, 1) * (m[:, :, :2] + P[:, None, 63:65])) * HALF + HALF
        return torch.cat([(m - T3).reshape(-1, 63), (u - T2).reshape(-1, 42)], dim=1)

    def cost(self, P, T3, T2):
        r = self.rows(P, T3, T2)
        return (self.wr * r * r).sum(1) + self.w_pose * (P[:, 3:48] ** 2).sum(1) + self.w_beta * (P[:, 48:58] ** 2).sum(1)

    def fit(self, T3, T2, P0, iters):
        P, B = P0.clone(), P0.shape[0]
        lam = torch.full((B,), self.lambda0, device=self.dev)
        eye3 = torch.eye(3, device=self.dev).repeat(21, 1).unsqueeze(0)
        eye = torch.eye(65, device=self.dev).expand(B, 65, 65)
        for _ in range(iters):
            x, jm = self.jac(P)
            s, cs = torch.exp(P[:, 61]).reshape(B, 1, 1), P[:, 62].reshape(B, 1, 1)
            xm = x[:, self.jm]
            J3 = torch.cat([s * jm.reshape(B, 21, 3, 58)[:, self.jm].reshape(B, 63, 58), eye3.expand(B, 63, 3),
                            (s * xm).reshape(B, 63, 1)], dim=2)
            m = s * xm + P[:, None, 58:61]
            d = m[:, :, :2] + P[:, None, 63:65]
            Jc = torch.zeros(B, 21, 2, 3, device=self.dev)
            Jc[:, :, :, 0] = d * HALF
            Jc[:, :, 0, 1] = Jc[:, :, 1, 2] = (cs * HALF).reshape(B, 1)
            J2 = torch.cat([(cs * HALF) * J3.reshape(B, 21, 3, 62)[:, :, :2].reshape(B, 42, 62), Jc.reshape(B, 42, 3)], dim=2)
            J = torch.cat([torch.cat([J3, torch.zeros(B, 63, 3, device=self.dev)], dim=2), J2], dim=1)
            r = torch.cat([(m - T3).reshape(B, 63), ((cs * d) * HALF + HALF - T2).reshape(B, 42)], dim=1)
            c = (self.wr * r * r).sum(1) + self.w_pose * (P[:, 3:48] ** 2).sum(1) + self.w_beta * (P[:, 48:58] ** 2).sum(1)
            A = J.transpose(1, 2) @ (self.wr.reshape(1, 105, 1) * J) + torch.diag(self.prior)
            g = (J.transpose(1, 2) @ (self.wr * r).unsqueeze(2)).squeeze(2) + self.prior * P
            L, info = torch.linalg.cholesky_ex(A + lam.reshape(B, 1, 1) * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2)))
            ok = info == 0
            Pt = P - torch.cholesky_solve(g.unsqueeze(2), torch.where(ok.reshape(B, 1, 1), L, eye)).squeeze(2)
            take = ok & torch.isfinite(Pt).all(1) & (self.cost(Pt, T3, T2) < c)
            P = torch.where(take.unsqueeze(1), Pt, P)
            lam = torch.where(take, (lam * 0.1).clamp_min(1e-12), (lam * 10).clamp_max(1e12))
        return P


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
    from scat_amd.fit import ManoFitter, free_mask
    from scat_amd.mano import ManoLayer, ManoModel

    lib().scat_check_device()
    dev = torch.device("cuda", 0)
    model = ManoModel.synthetic(1).to(dev)
    jmap = (0, 13, 14, 15, 20, 1, 2, 3, 16, 4, 5, 6, 17, 10, 11, 12, 19, 7, 8, 9, 18)
    fitter = ManoFitter(model, joint_map=jmap, iters=a.iters)
    plain = TorchLMKp(ManoLayer(model), model.V, jmap, fitter.w_pose, fitter.w_beta, fitter.lambda0, dev)
    lines = [f"V = {model.V}, {a.iters} LM iterations, {a.repeats} repeats, windows of {a.inner} fits, cases alternated; ms per "
             f"fit, device events around the window (host launch time included); {torch.cuda.get_device_name(0)}"]
    for B in a.batches:
        true = torch.cat([T_(synth.normal_like(90 + B, n, (B, k), s)) for n, k, s in
                          (("rots", 3, 0.8), ("poses", 45, 0.4), ("betas", 10, 1.0), ("trans", 3, 0.05), ("log_scale", 1, 0.2))]
                         + [T_(synth.uniform(90 + B, "cam.s", (B, 1), 3.0, 5.0)), T_(synth.uniform(90 + B, "cam.t", (B, 2), -0.05, 0.05))],
                         dim=1).float().to(dev)
        T3 = (torch.exp(true[:, 61]).reshape(-1, 1, 1) * plain.joints(true)[:, plain.jm] + true[:, None, 58:61]).contiguous()
        T2 = ((true[:, 62].reshape(-1, 1, 1) * (T3[:, :, :2] + true[:, None, 63:65])) * HALF + HALF).contiguous()
        w2 = torch.full((B, 21), 1e-6, device=dev)
        P0 = fitter.fit_keypoints(T3, T2, w2=w2, iters=1, free=0, free_cam=0).p      # the closed-form start, nothing solved for
        P0_3d = P0[:, :62].contiguous()
        P0_2d = fitter.fit_keypoints(joints2d=T2, iters=1, free=0, free_cam=0).p
        cases = [("mano_fit", lambda: fitter.fit(T3, init=P0_3d).p),
                 ("kp_3d", lambda: fitter.fit_keypoints(T3, init=P0).p),
                 ("kp_both", lambda: fitter.fit_keypoints(T3, T2, w2=w2, init=P0).p),
                 ("kp_2d_gm", lambda: fitter.fit_keypoints(joints2d=T2, sigma2=10.0, init=P0_2d,
                                                           free=free_mask(trans=False, log_scale=False)).p),
                 ("torch_lm", lambda: plain.fit(T3, T2, P0, a.iters))]
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

        def rms(P):      # the 3-D joint RMS in mm and the reprojection RMS in pixels
            P = P if P.shape[1] == 65 else torch.cat([P, true[:, 62:]], dim=1)
            r = plain.rows(P, T3, T2)
            return ((r[:, :63] ** 2).reshape(-1, 21, 3).sum(2).mean(1).sqrt() * 1e3, (r[:, 63:] ** 2).reshape(-1, 21, 2).sum(2).mean(1).sqrt())

        r0 = rms(P0)
        lines.append(f"batch {B}: start, median (max) over the batch: 3-D joint RMS {r0[0].median():.3f} ({r0[0].max():.3f}) mm, "
                     f"reprojection RMS {r0[1].median():.3f} ({r0[1].max():.3f}) px")
        med = {}
        for name, fn in cases:
            t = sorted(times[name])
            med[name] = statistics.median(t)
            r3, r2 = rms(fn())
            what = f"3-D {r3.median():.4f} ({r3.max():.4f}) mm" if name in ("mano_fit", "kp_3d") else \
                (f"2-D {r2.median():.4f} ({r2.max():.4f}) px" if name == "kp_2d_gm" else
                 f"3-D {r3.median():.4f} ({r3.max():.4f}) mm, 2-D {r2.median():.4f} ({r2.max():.4f}) px")
            lines.append(f"  {name:9s} median {med[name]:9.4f} ms  min {t[0]:9.4f}  max {t[-1]:9.4f}   reaches {what}")
        lines.append(f"  kp_3d / mano_fit: {med['kp_3d'] / med['mano_fit']:.4f}   kp_both / mano_fit: {med['kp_both'] / med['mano_fit']:.4f}"
                     f"   kp_both / torch_lm: {med['kp_both'] / med['torch_lm']:.4f}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
