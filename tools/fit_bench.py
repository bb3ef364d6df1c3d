#!/usr/bin/env python
"""The on-device MANO fit against what a user has without it, V = 778, batch 1 / 96 / 1024, 20 iterations from the same
start: device events after warm-up, medians over alternated repeats.

  kernel_fit    ManoFitter.fit from a given start: one launch (scat_mano_fit), Jacobian, normal equations, Cholesky and the
                trial cost inside it
  torch_lm      the same Levenberg-Marquardt written with ManoLayer in fp32 on the device: per iteration one forward +
                backward of the layer at 63 x the batch with one-hot cotangents for the Jacobian rows (the full 778-vertex
                mesh each time), torch.linalg.cholesky_ex / cholesky_solve, one more forward for the trial cost, and the
                accept / reject as torch.where (no host synchronisation inside the loop)

Every case is a window of ``inner`` fits between two events (host launch time included); the cases alternate inside every
repeat so that drift hits both alike.  Prints the median and the spread, the joint RMS both reach, and the ratio; with
--out also writes the table to a file (profiles/fit_bench.txt is such a run).  Not measured here: the kernels alone
(without the launch and ManoFitter's allocation of p, cost and accepted), and how the kernel's time splits between the
Jacobian and the solve."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))


class TorchLM:
    """the fit of include/scat_mano_fit.h with ManoLayer and torch.linalg, fp32 on the device"""

    def __init__(self, layer, V, joint_map, w_pose, w_beta, lambda0, dev):
        self.layer, self.V, self.dev = layer, V, dev
        self.jm = torch.as_tensor(joint_map, device=dev)
        self.w_pose, self.w_beta, self.lambda0 = w_pose, w_beta, lambda0
        self.prior = torch.zeros(62, device=dev)
        self.prior[3:48], self.prior[48:58] = w_pose, w_beta
        self.dout = {}

    def joints(self, P):
        with torch.no_grad():
            return self.layer(P[:, 0:3], P[:, 3:48], P[:, 48:58])[:, :21]

    def jac(self, P):
        B = P.shape[0]
        if B not in self.dout:      # 63 one-hot cotangents on the joint rows per sample
            d = torch.zeros(B, 63, (21 + self.V) * 3, device=self.dev)
            d[:, torch.arange(63), torch.arange(63)] = 1.0
            self.dout[B] = d.reshape(B * 63, 21 + self.V, 3)
        Pr = P[:, :58].repeat_interleave(63, dim=0)
        r, p, b = (Pr[:, s].contiguous().requires_grad_(True) for s in (slice(0, 3), slice(3, 48), slice(48, 58)))
        out = self.layer(r, p, b)
        g = torch.autograd.grad(out, (r, p, b), self.dout[B])
        return out.detach()[::63, :21], torch.cat(g, dim=1).reshape(B, 63, 58)

    def cost(self, P, T):
        r = torch.exp(P[:, 61]).reshape(-1, 1, 1) * self.joints(P)[:, self.jm] + P[:, None, 58:61] - T
        return (r * r).sum((1, 2)) + self.w_pose * (P[:, 3:48] ** 2).sum(1) + self.w_beta * (P[:, 48:58] ** 2).sum(1)

    def fit(self, T, P0, iters):
        P, B = P0.clone(), P0.shape[0]
        lam = torch.full((B,), self.lambda0, device=self.dev)
        eye3 = torch.eye(3, device=self.dev).repeat(21, 1).unsqueeze(0)
        eye = torch.eye(62, device=self.dev).expand(B, 62, 62)
        for _ in range(iters):
            x, jm = self.jac(P)
            s = torch.exp(P[:, 61]).reshape(B, 1, 1)
            xm = x[:, self.jm]
            J = torch.cat([s * jm.reshape(B, 21, 3, 58)[:, self.jm].reshape(B, 63, 58), eye3.expand(B, 63, 3),
                           (s * xm).reshape(B, 63, 1)], dim=2)
            r = (s * xm + P[:, None, 58:61] - T).reshape(B, 63)
            c = (r * r).sum(1) + self.w_pose * (P[:, 3:48] ** 2).sum(1) + self.w_beta * (P[:, 48:58] ** 2).sum(1)
            A = J.transpose(1, 2) @ J + torch.diag(self.prior)
            g = (J.transpose(1, 2) @ r.unsqueeze(2)).squeeze(2) + self.prior * P
            L, info = torch.linalg.cholesky_ex(A + lam.reshape(B, 1, 1) * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2)))
            ok = info == 0
            Pt = P - torch.cholesky_solve(g.unsqueeze(2), torch.where(ok.reshape(B, 1, 1), L, eye)).squeeze(2)
            take = ok & torch.isfinite(Pt).all(1) & (self.cost(Pt, T) < c)
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
    from scat_amd.fit import ManoFitter
    from scat_amd.mano import ManoLayer, ManoModel

    lib().scat_check_device()
    dev = torch.device("cuda", 0)
    model = ManoModel.synthetic(1).to(dev)
    jmap = (0, 13, 14, 15, 20, 1, 2, 3, 16, 4, 5, 6, 17, 10, 11, 12, 19, 7, 8, 9, 18)
    fitter = ManoFitter(model, joint_map=jmap, iters=a.iters)
    plain = TorchLM(ManoLayer(model), model.V, jmap, fitter.w_pose, fitter.w_beta, fitter.lambda0, dev)
    lines = [f"V = {model.V}, {a.iters} LM iterations, {a.repeats} repeats, windows of {a.inner} fits, cases alternated; ms per "
             f"fit, device events around the window (host launch time included); {torch.cuda.get_device_name(0)}"]
    for B in a.batches:
        true = torch.cat([T_(synth.normal_like(90 + B, n, (B, k), s)) for n, k, s in
                          (("rots", 3, 0.8), ("poses", 45, 0.4), ("betas", 10, 1.0), ("trans", 3, 0.05), ("log_scale", 1, 0.2))],
                         dim=1).to(dev)
        T = (torch.exp(true[:, 61]).reshape(-1, 1, 1) * plain.joints(true)[:, plain.jm] + true[:, None, 58:61]).contiguous()
        P0 = fitter.fit(T, iters=1, free=0).p      # the Procrustes start, nothing solved for: the same start for both
        cases = [("kernel_fit", lambda: fitter.fit(T, init=P0).p), ("torch_lm", lambda: plain.fit(T, P0, a.iters))]
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

        def rms(P):
            d = torch.exp(P[:, 61]).reshape(-1, 1, 1) * plain.joints(P)[:, plain.jm] + P[:, None, 58:61] - T
            return (d * d).sum(2).mean(1).sqrt() * 1e3

        ra, rb, r0 = rms(cases[0][1]()), rms(cases[1][1]()), rms(P0)
        lines.append(f"batch {B}: joint RMS in mm, median (max) over the batch: start {r0.median():.3f} ({r0.max():.3f}), "
                     f"kernel_fit {ra.median():.4f} ({ra.max():.4f}), torch_lm {rb.median():.4f} ({rb.max():.4f})")
        med = {}
        for name, _ in cases:
            t = sorted(times[name])
            med[name] = statistics.median(t)
            lines.append(f"  {name:12s} median {med[name]:9.4f} ms  min {t[0]:9.4f}  max {t[-1]:9.4f}")
        lines.append(f"  kernel / torch: {med['kernel_fit'] / med['torch_lm']:.4f}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
