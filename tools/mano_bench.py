#!/usr/bin/env python
"""The MANO layer against what a user has without it, V = 778, batch 1 / 96 / 1024: device events after warm-up, medians
over alternated repeats.

  layer_fwd        ManoLayer forward under no_grad: one launch (scat_mano_fwd)
  layer_fwd_bwd    ManoLayer forward + backward of a fixed cotangent: two launches plus autograd's bookkeeping
  torch_fwd        the same arithmetic as plain torch-ROCm ops on the device in fp32 (einsum / matmul / a Python loop over the
                   15 chain joints), under no_grad
  torch_fwd_bwd    the same through torch autograd

Every case is a window of ``inner`` calls between two events (host launch time included: at batch 1 that is what a caller
waits for); the cases alternate inside every repeat so that drift hits all of them alike.  Prints the median and the spread
and the agreement of the two paths; with --out also writes the table to a file (profiles/mano_bench.txt is such a run)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def torch_rodrigues(r):
    t = (r * r).sum(-1)
    th = t.sqrt()
    a, b = torch.sin(th) / th, (1.0 - torch.cos(th)) / t
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    o = torch.zeros_like(x)
    S = torch.stack([o, -z, y, z, o, -x, -y, x, o], dim=-1).reshape(-1, 3, 3)
    return torch.eye(3, dtype=r.dtype, device=r.device) + a.reshape(-1, 1, 1) * S + b.reshape(-1, 1, 1) * (S @ S)


class TorchMano:
    """rot_pose_beta_to_mesh with torch ops on device tensors in fp32 (ordinary angles only: no care at theta = 0)"""

    def __init__(self, m, dev):
        self.vt, self.sd, self.pd = (T_(a).to(dev) for a in (m.v_template, m.shapedirs, m.posedirs))
        self.Jr, self.W, self.hm = (T_(a).to(dev) for a in (m.J_regressor, m.weights, m.hands_mean))
        self.parents, self.tips = list(m.parents), list(m.tips)
        self.eye = torch.eye(3, device=dev)

    def __call__(self, rots, poses, betas):
        B = rots.shape[0]
        R = torch_rodrigues((self.hm + poses).reshape(-1, 3)).reshape(B, 15, 3, 3)
        v_shaped = self.vt + torch.einsum("vck,bk->bvc", self.sd, betas)
        J = torch.einsum("jv,bvc->bjc", self.Jr, v_shaped)
        v_posed = v_shaped + torch.einsum("vck,bk->bvc", self.pd, (R - self.eye).reshape(B, 135))
        RG, t = [self.eye.expand(B, 3, 3)], [J[:, 0]]
        for i in range(1, 16):
            p = self.parents[i]
            RG.append(RG[p] @ R[:, i - 1])
            t.append((RG[p] @ (J[:, i] - J[:, p]).unsqueeze(2)).squeeze(2) + t[p])
        RG, t = torch.stack(RG, 1), torch.stack(t, 1)
        a = t - (RG @ J.unsqueeze(3)).squeeze(3)
        v = (torch.einsum("vi,birc->bvrc", self.W, RG) @ v_posed.unsqueeze(3)).squeeze(3) + torch.einsum("vi,bir->bvr", self.W, a)
        x = torch.cat([t, v[:, self.tips], v], dim=1) @ torch_rodrigues(rots).transpose(1, 2)
        return x - x[:, 1:2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 96, 1024])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=100, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    from scat_amd import synth
    from scat_amd._lib import lib
    from scat_amd.mano import ManoLayer, ManoModel

    lib().scat_check_device()
    dev = torch.device("cuda", 0)
    model = ManoModel.synthetic(1).to(dev)
    layer, plain = ManoLayer(model), TorchMano(model, dev)
    lines = [f"V = {model.V}, {a.repeats} repeats, windows of {a.inner} calls, cases alternated; ms per call, device events "
             f"around the window (host launch time included); {torch.cuda.get_device_name(0)}"]
    for B in a.batches:
        rots, poses, betas = (T_(synth.normal_like(70 + B, n, (B, k), s)).to(dev).requires_grad_(True)
                              for n, k, s in (("rots", 3, 0.8), ("poses", 45, 0.4), ("betas", 10, 1.0)))
        dout = T_(synth.normal_like(70 + B, "dout", (B, 21 + model.V, 3), 1.0)).to(dev)

        def fwd(f):
            with torch.no_grad():
                return f(rots, poses, betas)

        def fwd_bwd(f):
            return torch.autograd.grad(f(rots, poses, betas), (rots, poses, betas), dout)

        cases = [("layer_fwd", lambda: fwd(layer)), ("torch_fwd", lambda: fwd(plain)),
                 ("layer_fwd_bwd", lambda: fwd_bwd(layer)), ("torch_fwd_bwd", lambda: fwd_bwd(plain))]
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
        rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
        agree = [rel(fwd(layer), fwd(plain))] + [rel(x, y) for x, y in zip(fwd_bwd(layer), fwd_bwd(plain))]
        lines.append(f"batch {B}: the two paths agree to out {agree[0]:.2e} drots {agree[1]:.2e} dposes {agree[2]:.2e} "
                     f"dbetas {agree[3]:.2e} (max |a - b| / max |b|, both fp32)")
        med = {}
        for name, _ in cases:
            t = sorted(times[name])
            med[name] = statistics.median(t)
            lines.append(f"  {name:14s} median {med[name]:8.4f} ms  min {t[0]:8.4f}  max {t[-1]:8.4f}")
        lines.append(f"  layer / torch: forward {med['layer_fwd'] / med['torch_fwd']:.4f}, forward + backward "
                     f"{med['layer_fwd_bwd'] / med['torch_fwd_bwd']:.4f}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
