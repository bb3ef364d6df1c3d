#!/usr/bin/env python
"""From 21 joints to a picture of the hand, all on the device: network output (or synthetic joints) -> ManoFitter ->
ManoFitter.mesh -> MeshRenderer + SkeletonOverlay -> one PNG with the samples side by side.

    python tools/fit_demo.py --out fit_demo.png                       # synthetic hands posed by the synthetic model
    python tools/fit_demo.py --network --out fit_demo.png             # an untrained EncoderTransformer's [B,66]

The mesh topology is tests/golden/hand_mesh.npz's (778 vertices); the MANO model is ManoModel.synthetic unless --mano
names a MANO pickle.  An untrained network predicts no hand, so with --network the picture shows the plumbing, and the
printed joint RMS says how far from any MANO pose its output is."""
import argparse
import os
import struct
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def write_png(path, rgb):
    """rgb: uint8 [H,W,3]; the standard library only"""
    H, W, _ = rgb.shape
    raw = b"".join(b"\x00" + rgb[y].tobytes() for y in range(H))
    chunk = lambda tag, data: struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--network", action="store_true", help="fit the output of an untrained EncoderTransformer")
    ap.add_argument("--mano", default=None, help="a MANO pickle (default: the synthetic model)")
    ap.add_argument("--out", default="fit_demo.png")
    a = ap.parse_args()
    from scat_amd import synth
    from scat_amd._lib import lib
    from scat_amd.fit import ManoFitter
    from scat_amd.mano import ManoLayer, ManoModel
    from scat_amd.render import MeshRenderer, SkeletonOverlay

    lib().scat_check_device()
    dev = torch.device("cuda", 0)
    B, S = a.batch, a.size
    model = (ManoModel.from_pickle(a.mano) if a.mano else ManoModel.synthetic(a.seed)).to(dev)
    T_ = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    if a.network:
        from types import SimpleNamespace

        from scat_amd.models.hand_net import EncoderTransformer

        opt = SimpleNamespace(vit_heads=8, pl_reg=False, iteration=3, pos_embed=True, mask_rate=0.0, vit_depth=3)
        net = EncoderTransformer(opt, torch.from_numpy(synth.mean_params(a.seed)))
        net.load_state_dict(synth.to_torch(synth.encoder_transformer_state(a.seed, 8)), strict=True)
        net = net.to(dev).eval()
        with torch.no_grad():
            out66 = net(T_(synth.images(a.seed + 1, B)))[0].float().contiguous()
    else:
        rots, poses, betas = (T_(synth.normal_like(a.seed, n, (B, k), s)) for n, k, s in
                              (("demo.rots", 3, 0.8), ("demo.poses", 45, 0.4), ("demo.betas", 10, 1.0)))
        cam = torch.tensor([[4.0, 0.0, 0.0]], device=dev).repeat(B, 1)
        pred = torch.cat([cam, rots, poses, betas], dim=1)
        with torch.no_grad():
            out66 = ManoLayer(model).params_to_outputs(pred).contiguous()
    fitter = ManoFitter(model, iters=a.iters)
    res = fitter.fit_outputs(out66)
    verts, joints = fitter.mesh(res), fitter.joints(res)
    d = joints - out66[:, 3:].reshape(B, 21, 3)
    rms = (d * d).sum(2).mean(1).sqrt() * 1e3
    print("joint RMS of the fit, mm:", [round(float(v), 4) for v in rms], "accepted steps:", res.accepted.tolist())
    faces = np.load(os.path.join(ROOT, "tests", "golden", "hand_mesh.npz"))["f"]
    rgb = MeshRenderer(faces, model.V, size=(S, S), device=dev).render(verts, out66[:, :3].contiguous(), want=("rgb",))["rgb"]
    rgb = SkeletonOverlay().draw_outputs(rgb.contiguous(), out66)      # the input joints over the fitted mesh
    write_png(a.out, np.concatenate(list(rgb.cpu().numpy()), axis=1))
    print(f"wrote {a.out}: {B} hands, {S} x {S} each")


if __name__ == "__main__":
    main()
