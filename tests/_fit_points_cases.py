"""The fixed inputs of the tests of the MANO fit to a point cloud and what the fp64 oracle (tests/_fit_points_oracle.py)
makes of them, computed once per process and read-only: shared by tests/test_fit_points.py (no GPU),
tests/test_gpu_fit_points.py and tools/fit_points_gates.py.  The models, the seeded hands and the joints-fit start are
_fit_verts_cases.py's.  Needs no GPU."""
import functools

import numpy as np
import torch

from scat_amd import synth

import _fit_points_oracle as PO
import _fit_verts_oracle as VO
import _fit_oracle as FO
from _fit_verts_cases import JOINT_MAP, NB, T_, case, frozen, host_model, joints_case, layer_case, seeded  # noqa: F401

# (B, N, V): the smallest; sub-wavefront and odd; one point past the workgroup; more workgroups than one wave of them per
# XCD; both maxima (SCAT_FIT_POINTS_MAX_N, SCAT_MANO_MAX_V), where the static LDS is largest
ASSIGN_SHAPES = ((1, 1, 1), (3, 37, 37), (3, 257, 37), (65, 300, 778), (1, 8192, 1536))
FIT_V = (37, 778)
ROUNDS, ITERS = 12, 4            # the recovery runs
MONOTONE_ROUNDS = (1, 2, 4, 8)
TRIM = 0.03
MARGIN = 1e-12                   # relative best / second-best d2 margin that every random point must have in the oracle


@functools.lru_cache(maxsize=None)
def assign_case(B, N, V, weighted):
    """random vertices of a 0.1 m cloud and points 5 mm off randomly chosen ones, max_dist at about the median distance so
    that both sides of the trim are taken; weights in (0.5, 1.5) with every seventh point's zero -> verts, points, weights
    (or None), max_dist, and the oracle's assignment on these fp32 numbers"""
    seed = 9100 + 13 * B + N + V
    verts = synth.normal_like(seed, "cloud.verts", (B, V, 3), 0.1).astype(np.float32)
    pick = np.random.default_rng(seed).integers(0, V, size=(B, N))
    points = (np.take_along_axis(verts, pick[:, :, None], 1) +
              synth.normal_like(seed, "cloud.noise", (B, N, 3), 0.005)).astype(np.float32)
    weights = None
    if weighted:
        weights = (1.0 + 0.5 * np.tanh(synth.normal_like(seed, "cloud.w", (B, N), 1.0))).astype(np.float32)
        weights[:, ::7] = 0.0
    free = PO.assign(verts, points, weights, np.inf, margins=True)
    live = free["idx"] >= 0
    assert (free["margin"][live] > MARGIN).all(), float(free["margin"][live].min())
    max_dist = float(np.float32(np.median(free["dist"][live]))) if live.any() else 1.0
    want = PO.assign(verts, points, weights, max_dist)
    if N > 1:
        assert 0 < want["matched"].sum() < live.sum()
    return frozen([verts, points]) + (None if weights is None else frozen([weights])[0], max_dist, want)


@functools.lru_cache(maxsize=None)
def deliberate_case():
    """four hands of four vertices and four points on dyadic coordinates, max_dist = 0.25:
    0  vertices 0 and 1 identical: the lowest index wins
    1  a point exactly midway between vertices 0 and 1: the lowest index wins
    2  a point at distance exactly 0.25 (matched), one at the next fp32 above (not matched), one at exactly 0.25 from
       vertex 2
    3  every point 10 away: nothing matched"""
    base = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, 4]], np.float32)
    verts = np.stack([base] * 4)
    verts[0, 1] = verts[0, 0]
    verts[1, 1] = (0.25, 0, 0)
    up = np.nextafter(np.float32(0.25), np.float32(1))
    points = np.array([[[0.125, 0, 0], [0, 0.0625, 0], [0, 2, 0.125], [0, 0, 4]],
                       [[0.125, 0, 0], [0, 2, 0], [0, 0, 4.125], [0.25, 0.0625, 0]],
                       [[0.25, 0, 0], [up, 0, 0], [0, 2.25, 0], [0, 0, 4]],
                       [[10, 10, 10], [-10, 0, 0], [0, 12, 0], [0, 0, -6]]], np.float32)
    want = PO.assign(verts, points, None, 0.25)
    assert want["idx"].tolist() == [[0, 0, 2, 3], [0, 2, 3, 1], [0, 0, 2, 3], want["idx"][3].tolist()]
    assert want["matched"].tolist() == [[True] * 4, [True] * 4, [True, False, True, True], [False] * 4]
    assert np.isnan(want["vw"][3]).all() and want["stats"][3].tolist() == [0.0, 0.0, 0.0, 0.0]
    return frozen([verts, points]) + (0.25, want)


@functools.lru_cache(maxsize=None)
def cloud(V, kind):
    """the seeded hands' meshes as unordered clouds [NB,N,3] fp32: "shuffled" all V vertices in one shuffled order, "half"
    the V // 2 vertices of one side of the template (largest x), shuffled"""
    Tv = seeded(V)[2].numpy()
    rng = np.random.default_rng(4200 + V)
    if kind == "shuffled":
        sel = rng.permutation(V)
    else:
        assert kind == "half"
        side = np.argsort(-np.asarray(host_model(V).v_template)[:, 0], kind="stable")[:V // 2]
        sel = side[rng.permutation(len(side))]
    return frozen([np.ascontiguousarray(Tv[:, sel])])[0]


def start(V):
    """the joints fit of the same hands, rounded to fp32: what a caller would start from"""
    return joints_case(V)[1].float()


@functools.lru_cache(maxsize=None)
def icp_case(V, kind, max_dist=None, rounds=ROUNDS, iters=ITERS):
    """the oracle's ICP from the joints-fit start -> Pf, the vertex RMS against the true mesh at the start and at Pf [NB],
    the data costs of every assignment [rounds + 1, NB], which hands are recoverable (final RMS < 1e-4 m), and the P of every
    assignment [rounds + 1, NB, 62]"""
    m = host_model(V)
    Tv = seeded(V)[2]
    md = np.inf if max_dist is None else max_dist
    Pf, acc, costs, last, Ps = PO.icp(m, cloud(V, kind), None, start(V), rounds, iters, md, history=True)
    r0, rf = VO.rms(m, start(V), Tv).numpy(), VO.rms(m, Pf, Tv).numpy()
    return Pf, r0, rf, costs, rf < 1e-4, Ps


PARAM_V, PARAM_B = (1, 37, 778), (1, 3, 65)


@functools.lru_cache(maxsize=None)
def param_case(B, V):
    """_fit_verts_cases.case's rots, poses and betas with trans ~ N(0, 0.05) and log_scale ~ N(0, 0.2): P [B,62] fp32, the
    oracle's fp64 model points, and a cloud of N = 2 V + 3 points 3 mm off them with weights in (0.5, 1.5), some zero"""
    seed = 9300 + 7 * B + V
    P = np.concatenate([case(B, V)[0], synth.normal_like(seed, "trans", (B, 3), 0.05),
                        synth.normal_like(seed, "log_scale", (B, 1), 0.2)], axis=1).astype(np.float32)
    with torch.no_grad():
        x = VO.model_verts(host_model(V), T_(P).double()).numpy()
    N = 2 * V + 3
    pick = np.random.default_rng(seed).integers(0, V, size=(B, N))
    points = (np.take_along_axis(x, pick[:, :, None], 1) + synth.normal_like(seed, "cloud.noise", (B, N, 3), 0.003)).astype(np.float32)
    weights = (1.0 + 0.5 * np.tanh(synth.normal_like(seed, "cloud.w", (B, N), 1.0))).astype(np.float32)
    weights[:, ::5] = 0.0
    return frozen([P, x, points, weights])


@functools.lru_cache(maxsize=None)
def layer_cloud_case(V=778):
    """_fit_verts_cases.layer_case's hands (no translation, scale 1) as the pipeline sees them: the shuffled mesh as the
    cloud, and the oracle's ICP from the oracle's joints fit of the layer's 21 joints -> cloud, the final vertex RMS [NB]
    and which hands are recoverable"""
    import _mano_oracle as MO

    m = host_model(V)
    P, Tv = layer_case(V)[:2]
    with torch.no_grad():
        Tj = MO.forward(m, P[:, :3], P[:, 3:48], P[:, 48:58])[:, :21][:, list(JOINT_MAP)].float()
    w = torch.ones(NB, 21, dtype=torch.float64)
    P0 = FO.lm(m, Tj.double(), w, JOINT_MAP, FO.procrustes_start(m, Tj, w, JOINT_MAP), 20)[0].float()
    pts = np.ascontiguousarray(Tv.numpy()[:, np.random.default_rng(4300 + V).permutation(V)])
    Pf = PO.icp(m, pts, None, P0, ROUNDS, ITERS)[0]
    rf = VO.rms(m, Pf, Tv).numpy()
    return frozen([pts])[0], rf, rf < 1e-4
