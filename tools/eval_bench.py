#!/usr/bin/env python
"""On-device evaluation against what it replaces, batch 96, device events after warm-up, medians over alternated repeats.

  torch_metrics     scat_amd.metrics on device tensors: mpjpe_mm + pa_mpjpe_mm + pck raw + pck of the aligned joints
                    (torch.linalg.svd on a batch of 3 x 3 matrices, a few dozen small launches)
  eval_accumulate   ops.eval_accumulate: the same scores, the 2-D error and the counts, two launches
  frame_mask        ops.eval_frame_mask on one [B,3,224,224] fp32 batch read again and again: at 58 MB it stays in the
                    256 MB Infinity Cache, so its rate is not an HBM rate
  frame_mask_cold   the same over a ring of distinct batches of more than 256 MB in all: every call reads from HBM
  forward           net(x) in eval mode under no_grad
  update            Evaluator.update: forward + frame mask + accumulate into the device table

Every case is a window of ``inner`` calls between two events; the cases alternate inside every repeat so that drift hits
all of them alike, and forward / update run in the order A B B A so that neither always follows the small kernels.  Prints
the median and the spread."""
import argparse
import os
import random
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=96)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=200, help="calls per timed window of the small cases")
    ap.add_argument("--inner-net", type=int, default=20, help="calls per timed window of the cases with a forward")
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from scat_amd import metrics as M
    from scat_amd import ops, synth
    from scat_amd._lib import lib
    from scat_amd.evaluator import Evaluator
    from scat_amd.models.hand_net import EncoderTransformer

    lib().scat_check_device()
    dev = torch.device("cuda", 0)
    B = a.batch
    opt = SimpleNamespace(vit_heads=8, pl_reg=False, iteration=3, pos_embed=True, mask_rate=0.2, vit_depth=3)
    net = EncoderTransformer(opt, T_(synth.mean_params(1)))
    net.load_state_dict(synth.to_torch(synth.encoder_transformer_state(1, 8)), strict=True)
    net.to(dev).eval()
    x = T_(synth.images(200, B)).to(dev)
    labels = T_(synth.labels(201, B)).to(dev)
    rnge = np.arange(20, 51, 5.0)
    th = T_(rnge.astype(np.float32)).to(dev)
    random.seed(1)
    with torch.no_grad():
        out = net(x)[0].clone()
    gt = labels[:, :63].contiguous()
    rec = torch.empty(8 + 2 * th.numel(), dtype=torch.float64, device=dev)
    ev = Evaluator(net, rnge, max_batches=4096)

    def torch_metrics():
        p, g = M._j(out), M._j(gt)
        al = M.procrustes_align(p, g)
        return M.mpjpe_mm(p, g), (al - g).norm(dim=-1).mean() * 1000.0, M.pck(p, g, th), M.pck(al, g, th)

    def forward():
        with torch.no_grad():
            return net(x)[0]

    ring = [x] + [x.clone() for _ in range(max(1, (300 << 20) // (x.numel() * 4)))]
    turn = [0]

    def frame_mask_cold():
        turn[0] = (turn[0] + 1) % len(ring)
        return ops.eval_frame_mask(ring[turn[0]])

    def update():
        if ev.n == ev.max_batches:
            ev.reset()
        return ev.update(x, labels)

    cases = [("torch_metrics", torch_metrics, a.inner),
             ("eval_accumulate", lambda: ops.eval_accumulate(out, labels, th, record=rec), a.inner),
             ("frame_mask", lambda: ops.eval_frame_mask(x), a.inner), ("frame_mask_cold", frame_mask_cold, a.inner),
             ("forward", forward, a.inner_net), ("update", update, a.inner_net), ("update", update, a.inner_net),
             ("forward", forward, a.inner_net)]
    for _ in range(a.warmup):
        for _, fn, _ in cases:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cases}
    for _ in range(a.repeats):
        for name, fn, inner in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner)
    # the two paths agree on what both compute (the torch path is fp32)
    r = rec.cpu().numpy()
    tm = [v.cpu().numpy() for v in torch_metrics()]
    print(f"agreement at batch {B}: mpjpe {r[4] / r[1]:.4f} vs {tm[0]:.4f} mm, pa_mpjpe {r[5] / r[1]:.4f} vs {tm[1]:.4f} mm, "
          f"pck max diff {np.abs(100 * r[8:8 + 7] / (21 * r[1]) - tm[2]).max():.2e}, "
          f"pck_pa max diff {np.abs(100 * r[15:22] / (21 * r[1]) - tm[3]).max():.2e}")
    print(f"batch {B}, {a.repeats} repeats, windows of {a.inner} calls ({a.inner_net} with a forward), cases alternated; "
          f"ms per call, device events around the window (host launch time included)")
    med = {}
    for name in dict.fromkeys(name for name, _, _ in cases):
        t = sorted(times[name])
        med[name] = statistics.median(t)
        extra = ""
        if name.startswith("frame_mask"):
            nbytes = x.numel() * 4
            extra = f"  bytes {nbytes / 1e6:6.1f} MB  {nbytes / med[name] / 1e6:7.1f} GB/s"
        print(f"{name:16s} median {med[name]:8.4f} ms  min {t[0]:8.4f}  max {t[-1]:8.4f}{extra}")
    print(f"eval_accumulate / torch_metrics = {med['eval_accumulate'] / med['torch_metrics']:.4f}")
    over = med["update"] - med["forward"]
    print(f"update - forward = {over:+.4f} ms = {100 * over / med['forward']:+.3f} % of the forward "
          f"(frame_mask + eval_accumulate alone: {med['frame_mask'] + med['eval_accumulate']:.4f} ms = "
          f"{100 * (med['frame_mask'] + med['eval_accumulate']) / med['forward']:.3f} %)")


if __name__ == "__main__":
    main()
