"""Device augmentation against the plain input kernel, batch 96, device events after warm-up.

Cases, alternated inside every repeat of one process so that drift hits all of them alike:
  preprocess_u8    the library's normalise + resize on a 256 x 256 CHW source
  warp_identity    augment_warp_u8 with the identity plan on the same source (same arithmetic, same bytes)
  flip             plan + warp on 640 x 480 HWC frames, mirror only
  rot              ... with a rotation on every sample
  rot_blur         ... with a rotation and a motion blur forced on every sample (the reference blurs one in six)
  rot_blur_drawn   DeviceAugment(rotation, motion_blur) as a user calls it: draws, pinned upload and both launches
Bytes are the algorithm's, from shapes: every source byte once (the warp reads only the crop, so this is an upper bound
on what it has to fetch) plus the fp32 output once.  Reports the median and the spread (min..max) over the repeats."""
import argparse
import os
import random
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def seeded_joints(rng, B, W, H):
    ctr = rng.uniform([220, 170], [W - 220, H - 170], (B, 1, 2))
    j2 = ctr + rng.uniform(-1, 1, (B, 21, 2)) * rng.uniform(40, 110, (B, 1, 1))
    return j2.astype(np.float32), rng.normal(0, 0.03, (B, 21, 3)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=96)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=50, help="launches per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from scat_amd import ops, synth
    from scat_amd._lib import lib
    from scat_amd.augment import DeviceAugment, pack_plan

    lib().scat_check_device()
    dev = torch.device("cuda", 0)
    B, W, H = a.batch, 640, 480
    rng = np.random.default_rng(1)
    small = torch.from_numpy(synth.randint_u8(100, "bench_images", (B, 3, 256, 256))).to(dev)
    ident = torch.from_numpy(np.stack([pack_plan([[1, 0, 0], [0, 1, 0]], 0, 0, 256, 256)] * B)).to(dev)
    frames = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    j2, j3 = (torch.from_numpy(t).to(dev) for t in seeded_joints(rng, B, W, H))

    def params(rot, blur):
        p = np.zeros((B, 4), dtype=np.int32)
        p[:, 0] = 1
        if rot:
            p[:, 3] = rng.integers(1, 361, B)
        if blur:
            p[:, 1], p[:, 2] = rng.integers(1, 11, B), rng.integers(0, 2, B)
        return torch.from_numpy(p).to(dev)

    p_flip, p_rot, p_rb = params(0, 0), params(1, 0), params(1, 1)
    aug = DeviceAugment(rotation=True, motion_blur=True)

    def full(p):
        labels, plan = ops.augment_plan(j2, j3, p, (W, H))
        return ops.augment_warp_u8(frames, plan, hwc=True)

    out_bytes = B * 3 * 224 * 224 * 4
    cases = [
        ("preprocess_u8", lambda: ops.preprocess_u8(small), small.numel() + out_bytes),
        ("warp_identity", lambda: ops.augment_warp_u8(small, ident, hwc=False), small.numel() + out_bytes),
        ("flip", lambda: full(p_flip), frames.numel() + out_bytes),
        ("rot", lambda: full(p_rot), frames.numel() + out_bytes),
        ("rot_blur", lambda: full(p_rb), frames.numel() + out_bytes),
        ("rot_blur_drawn", lambda: aug(frames, j2, j3), frames.numel() + out_bytes),
    ]
    random.seed(1)
    for _ in range(a.warmup):
        for _, fn, _ in cases:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cases}
    for _ in range(a.repeats):
        for name, fn, _ in cases:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.inner)
    print(f"batch {B}, {a.repeats} repeats x {a.inner} calls, cases alternated; ms per call, device events")
    for name, _, nbytes in cases:
        t = sorted(times[name])
        med = statistics.median(t)
        print(f"{name:16s} median {med:7.4f} ms  min {t[0]:7.4f}  max {t[-1]:7.4f}  "
              f"bytes {nbytes / 1e6:6.1f} MB  {nbytes / med / 1e6:7.1f} GB/s  {B / med * 1e3:9.0f} img/s")
    r = statistics.median(times["warp_identity"]) / statistics.median(times["preprocess_u8"])
    print(f"warp_identity / preprocess_u8 = {r:.3f}")


if __name__ == "__main__":
    main()
