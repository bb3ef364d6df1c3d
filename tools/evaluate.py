#!/usr/bin/env python
"""Score a checkpoint over a dataset on the GPU, as the reference's eval loop does (eval.py:788-1053).

  python tools/evaluate.py                                   synthetic weights, synthetic batches
  python tools/evaluate.py --ckpt model.pth --data set.npz   a reference-style state_dict; the .npz holds ``inputs``
                                                             [N,3,224,224] fp32 in [-1,1] (or uint8 with --u8) and
                                                             ``labels`` [N,105] or [N,166]

The last partial batch is dropped, as the reference's DataLoader(drop_last=True) does.  Prints the reference's
"*** Final Results ***" block (eval.py:1048-1053) and, beyond it, PA-MPJPE, the 2-D error, PCK at every threshold and
frames/s.  The reference's "MPJPE" line is computed after the alignment (eval.py:953 overwrites the prediction), so it is
the PA-MPJPE here; the un-aligned MPJPE is printed beside it."""
import argparse
import os
import random
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", help="state_dict saved with torch.save (train.py:237-246); default: the synthetic state")
    ap.add_argument("--data", help=".npz with inputs and labels; default: synthetic batches")
    ap.add_argument("--u8", action="store_true", help="inputs are uint8 [N,3,H,W]: resized and normalised on the GPU")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--batches", type=int, default=4, help="number of synthetic batches (without --data)")
    ap.add_argument("--mask-rate", type=float, default=0.2, help="the reference masks tokens in eval mode too")
    ap.add_argument("--seed", type=int, default=0, help="seeds python random, which draws the token mask")
    a = ap.parse_args()
    from scat_amd import synth
    from scat_amd._lib import lib
    from scat_amd.evaluator import Evaluator
    from scat_amd.models.hand_net import EncoderTransformer

    lib().scat_check_device()
    dev = torch.device("cuda", 0)
    opt = SimpleNamespace(vit_heads=8, pl_reg=False, iteration=3, pos_embed=True, mask_rate=a.mask_rate, vit_depth=3)
    net = EncoderTransformer(opt, T_(synth.mean_params(1)))
    sd = torch.load(a.ckpt, map_location="cpu") if a.ckpt else synth.to_torch(synth.encoder_transformer_state(1, 8))
    net.load_state_dict(sd, strict=True)
    net.to(dev)
    B = a.batch
    if a.data:
        d = np.load(a.data)
        n = d["inputs"].shape[0] // B
        batches = ((d["inputs"][i * B:(i + 1) * B], d["labels"][i * B:(i + 1) * B].astype(np.float32)) for i in range(n))
    else:
        n = a.batches
        batches = ((synth.images(300 + i, B), synth.labels(400 + i, B)) for i in range(n))
    ev = Evaluator(net, preprocess="u8" if a.u8 else None, max_batches=max(n, 1))
    random.seed(a.seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for x, lab in batches:
        ev.update(T_(x).to(dev, non_blocking=True), T_(lab).to(dev, non_blocking=True))
    r = ev.result()      # the one device-to-host copy: it waits for everything above
    dt = time.perf_counter() - t0
    print("*** Final Results ***")
    print()
    print("MPJPE: " + str(r["pa_mpjpe_mm"]))
    print("AUC: " + str(r["auc_pa"]))
    print()
    print(f"frames {r['frames']}  kept {r['frames_kept']}  blank {r['frames_skipped']}  degenerate {r['frames_degenerate']}  "
          f"batches {r['batches']} (without a kept frame: {r['batches_empty']})")
    print(f"MPJPE (no alignment) {r['mpjpe_mm']:.3f} mm   PA-MPJPE {r['pa_mpjpe_mm']:.3f} mm   2-D error {r['err2d_px']:.3f} px")
    print(f"AUC (no alignment) {r['auc']:.4f}   AUC after alignment {r['auc_pa']:.4f}   pooled over frames "
          f"{r['auc_pooled']:.4f} / {r['auc_pa_pooled']:.4f}")
    for t, p, q in zip(r["thresholds_mm"], r["pck"], r["pck_pa"]):
        print(f"PCK@{t:g} mm  {p:7.3f} %   after alignment {q:7.3f} %")
    print(f"{r['frames'] / dt:.1f} frames/s ({dt * 1e3:.1f} ms for {r['frames']} frames, host loading included)")


if __name__ == "__main__":
    main()
