#!/usr/bin/env python
"""The renderer's cost, V = 778 / F = 1538 (tests/golden/hand_mesh.npz), 224 x 224, batch 1 / 96 / 1024: device events
after warm-up, medians over alternated repeats.

  render         MeshRenderer.render over a frame, want = rgb: two launches (scat_render_project, scat_render_raster)
  render_ids     the same without shading, want = face_id
  draw           SkeletonOverlay.draw of MANO_BONES over the rendered frames: one launch (scat_render_skeleton)

Every case is a window of ``inner`` calls between two events (host launch time included: at batch 1 that is what a caller
waits for); the cases alternate inside every repeat so that drift hits all of them alike.  The batch holds the six views
of the tests in turn, so tiles with many faces and empty tiles are both there.  There is nothing on the device to compare
against (the reference draws on the host, with an OpenGL context): no ratio, only what was measured and where.  With
--out also writes the table to a file (profiles/render_bench.txt is such a run)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 96, 1024])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import _render_oracle as RO
    from scat_amd._lib import lib
    from scat_amd.render import MeshRenderer, SkeletonOverlay

    lib().scat_check_device()
    dev = torch.device("cuda", 0)
    g = np.load(os.path.join(ROOT, "tests", "golden", "hand_mesh.npz"))
    vs, cams = RO.views(g["v"])
    H = W = 224
    renderer, overlay = MeshRenderer(g["f"], 778, size=(H, W), device=dev), SkeletonOverlay()
    lines = [f"V = 778, F = 1538, {H} x {W}, {a.repeats} repeats, windows of {a.inner} calls, cases alternated; ms per call, "
             f"device events around the window (host launch time included); {torch.cuda.get_device_name(0)}"]
    for B in a.batches:
        pick = np.arange(B) % len(vs)
        verts, cam = torch.from_numpy(vs[pick]).to(dev), torch.from_numpy(cams[pick]).to(dev)
        img = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev)
        j2d = torch.from_numpy(np.stack([RO.project_joints(RO.joints_of(vs[k]), cams[k], H, W) for k in pick]).astype(np.float32)).to(dev)
        rgb = renderer.render(verts, cam, img, want=("rgb",))["rgb"]
        cases = [("render", lambda: renderer.render(verts, cam, img, want=("rgb",))),
                 ("render_ids", lambda: renderer.render(verts, cam, None, want=("face_id",))),
                 ("draw", lambda: overlay.draw(rgb, j2d))]
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
        lines.append(f"batch {B}:")
        for name, _ in cases:
            t = sorted(times[name])
            lines.append(f"  {name:11s} median {statistics.median(t):8.4f} ms  min {t[0]:8.4f}  max {t[-1]:8.4f}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
