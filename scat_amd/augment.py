"""On-device sample augmentation: what dataset/load_STB.py:252-294 does to a sample on the host, per image, in PIL and
OpenCV (mirror, motion blur on one sample in six, rotation by a random angle, the crop around the hand, the resize to
224 x 224 and the matching label changes), as two launches on decoded uint8 frames that are already on the GPU.

    aug = DeviceAugment(rotation=True, motion_blur=True)
    inputs, labels = aug(u8, j2d, j3d)        # [B,3,224,224] fp32, [B,105] fp32: what TrainStep.__call__ takes

The random parameters come from python ``random`` in the reference's order, so a seeded run draws what the reference's
loader draws.  The operator itself is DESIGN.md section 8."""
from __future__ import annotations

import random

import numpy as np
import torch

from . import ops
from ._lib import ScatError


def draw_params(B, rotation=False, motion_blur=False, flip=True):
    """int32 [B,4] = (flip, k, vert, angle) per sample, consuming python ``random`` as load_STB.py:265-272 and
    motion_blur (load_STB.py:159,180) do: the use_blur draw, then only when it is 1 the kernel size and the direction
    (0 = vertical), then the angle."""
    p = np.zeros((B, 4), dtype=np.int32)
    p[:, 0] = int(bool(flip))
    for i in range(B):
        if motion_blur:
            if random.randint(0, 5) == 1:
                p[i, 1] = random.randint(1, 10)
                p[i, 2] = int(random.randint(0, 1) == 0)
        if rotation:
            p[i, 3] = random.randint(1, 360)
    return p


def pack_plan(minv, L, T, nw, nh, n=None, flip=0, k=0, vert=0, out=224):
    """One plan record (ops.AUGMENT_PLAN_FLOATS floats) built on the host, for callers that bring their own geometry:
    minv is the 2 x 3 map from canvas to source coordinates, (L, T, nw, nh) the integer crop box on the canvas."""
    minv = np.asarray(minv, dtype=np.float64).reshape(2, 3)
    if n is None:
        n = min(max(int(np.floor(nw / out + 0.5)), 1), 4)
    sx, sy, u0, v0 = nw / out, nh / out, L - 0.5, T - 0.5
    A = np.array([minv[0, 0] * sx, minv[0, 1] * sy, minv[0, 0] * u0 + minv[0, 1] * v0 + minv[0, 2],
                  minv[1, 0] * sx, minv[1, 1] * sy, minv[1, 0] * u0 + minv[1, 1] * v0 + minv[1, 2]], dtype=np.float64)
    rec = np.zeros(ops.AUGMENT_PLAN_FLOATS, dtype=np.float32)
    rec[:12] = A.view(np.float32)
    rec[12:20] = [L, T, nw, nh, n, int(bool(flip)), k, int(bool(vert))]
    return rec


class DeviceAugment:
    """u8 [B,H,W,3] (as a decoder leaves it) or [B,3,H,W] uint8, j2d [B,21,2] pixel coordinates in that frame, j3d
    [B,21,3], all on the GPU -> (inputs [B,3,224,224] fp32 in [-1,1], labels [B,105] fp32).  Two launches on the current
    stream, no host synchronisation, no device-to-host copy."""

    def __init__(self, rotation=False, motion_blur=False, flip=True, normalize_3d=True):
        self.rotation, self.motion_blur, self.flip, self.normalize_3d = rotation, motion_blur, flip, normalize_3d

    def __call__(self, u8, j2d, j3d):
        if u8.dim() != 4 or (u8.shape[3] != 3 and u8.shape[1] != 3):
            raise ScatError(f"DeviceAugment needs frames [B,H,W,3] or [B,3,H,W], got {tuple(u8.shape)}")
        hwc = u8.shape[3] == 3
        B = u8.shape[0]
        H, W = (u8.shape[1], u8.shape[2]) if hwc else (u8.shape[2], u8.shape[3])
        host = torch.empty((B, 4), dtype=torch.int32, pin_memory=True)   # from torch's pinned pool: stream-safe reuse
        host.numpy()[:] = draw_params(B, self.rotation, self.motion_blur, self.flip)
        params = host.to(u8.device, non_blocking=True)
        labels, plan = ops.augment_plan(j2d, j3d, params, (W, H), self.normalize_3d)
        return ops.augment_warp_u8(u8, plan, (224, 224), hwc=hwc), labels
