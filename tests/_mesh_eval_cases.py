"""Inputs of the mesh-scoring tests, shared by tests/test_mesh_eval.py (which asserts the conditions on them from the
oracle alone, without a GPU) and tests/test_gpu_mesh_eval.py (which runs the kernels on them).  Plain helper module."""
from __future__ import annotations

import functools
import os

import numpy as np

from scat_amd import synth

import _mesh_eval_oracle as MO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hand_mesh.npz")
SEED = 7300
MIN_MARGIN_MM = 1e-6      # every distance at least this far from every threshold: a count can not hinge on rounding
MIN_RATIO = 1e-3          # (sigma2 + sign(det K) sigma3) / sigma1: the optimal proper rotation is unique

# (T, F): the smallest case, the workload's, and the caps
THRESHOLDS = {
    "one": (np.array([20.0]), np.array([5.0])),
    "workload": (np.linspace(0.5, 50.0, 100), np.array([5.0, 15.0])),
    "caps": (np.linspace(0.5, 64.0, 128), np.array([2.5, 5.0, 7.5, 10.0, 15.0, 20.0, 25.0, 30.0])),
}
# (V, B, thresholds): V = 1 degenerate everywhere, 37 below a workgroup, 64 / 65 a wavefront edge, 257 a second query per
# thread, 778 the real mesh, 1024 the cap; B = 1, 6 (the special samples), 65 (a fold longer than a wavefront)
CASES = ([(V, 6, "workload") for V in (1, 37, 64, 65, 257, 778, 1024)]
         + [(65, 1, "workload"), (65, 65, "workload"), (778, 1, "workload")]
         + [(V, 6, t) for V in (37, 778) for t in ("one", "caps")])


def rot(a, b, c):
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return rz @ ry @ rx


@functools.lru_cache(maxsize=None)
def mesh(V):
    """V points of the hand of tests/golden/hand_mesh.npz, metres: a strided subsample below 778 vertices, the centroids
    of the first faces appended above"""
    d = np.load(GOLDEN)
    v, f = d["v"].astype(np.float64), d["f"]
    if V <= v.shape[0]:
        return v[np.linspace(0, v.shape[0] - 1, V).round().astype(int)] if V > 1 else v[:1]
    return np.concatenate([v, v[f[:V - v.shape[0]]].mean(axis=1)])


@functools.lru_cache(maxsize=None)
def inputs(V, B):
    """pred, gt [B,V,3] fp32 (read-only): gt = the mesh under a seeded rotation; an even sample has pred = gt + N(0, 4 mm),
    an odd one pred = scale in [0.7, 1.4] x rotation x gt + shift in +-3 cm + N(0, 4 mm); from B = 6 on sample 1 is planar,
    2 mirrored in x, 3 equal to gt, 4 shifted by 10 m"""
    seed = SEED + 7 * V + B
    base = mesh(V)
    ang = synth.uniform(seed, "gt_angles", (B, 3), -np.pi, np.pi)
    gt = np.stack([base @ rot(*ang[b]).T for b in range(B)])
    ang = synth.uniform(seed, "angles", (B, 3), -np.pi, np.pi)
    scale = synth.uniform(seed, "scale", (B,), 0.7, 1.4)
    shift = synth.uniform(seed, "shift", (B, 1, 3), -0.03, 0.03)
    noise = synth.normal_like(seed, "noise", (B, V, 3), 0.004).astype(np.float64)
    pred = gt + noise
    for b in range(1, B, 2):
        pred[b] = scale[b] * gt[b] @ rot(*ang[b]).T + shift[b] + noise[b]
    if B >= 6:
        gt[1, :, 2] = 0.0
        pred[1, :, 2] = 0.0
        pred[2] = gt[2] * np.array([-1.0, 1.0, 1.0]) + noise[2]
        pred[3] = gt[3]
        pred[4] += 10.0
    pred, gt = pred.astype(np.float32), gt.astype(np.float32)
    if B >= 6:
        assert np.array_equal(pred[3], gt[3])
    pred.setflags(write=False)
    gt.setflags(write=False)
    return pred, gt


@functools.lru_cache(maxsize=None)
def samples(V, B):
    """the oracle's distances of every sample of inputs(V, B), computed once"""
    pred, gt = inputs(V, B)
    return tuple(MO.sample(pred[b], gt[b]) for b in range(B))


def oracle(V, B, tset, keep=None):
    th, fth = THRESHOLDS[tset]
    return MO.batch(samples(V, B), th, fth, keep)
