"""The fixed inputs of the tests of the MANO fit to a track of meshes and of point clouds and what the fp64 oracle
(tests/_fit_seq_verts_oracle.py) makes of them, computed once per process and read-only: shared by
tests/test_fit_seq_verts.py (no GPU), tests/test_gpu_fit_seq_verts.py and tools/fit_seq_verts_gates.py.  The tracks are
_fit_seq_cases.track's unknowns (a hand that turns, flexes and drifts), the parity models and topologies _fit_plane_cases',
the quality model its smooth_model on the hand surface.  Needs no GPU."""
import functools

import numpy as np
import torch

from scat_amd import synth

import _fit_plane_cases as LC
import _fit_plane_oracle as LO
import _fit_points_oracle as PO
import _fit_seq_cases as SC
import _fit_seq_verts_oracle as QO
import _fit_verts_oracle as VO
from _fit_cases import T_, frozen, host_model

# the smoothness of the step, cost, start and gap cases: _fit_seq_cases.SMOOTH times 2, about V / 21 at V = 37, because
# the data term is summed over V vertices (the header's UNITS)
SMOOTH = dict(rots=2e-3, poses=2e-4, betas=2e-2, trans=2e-1, scale=2e-1)
TAU = 0.01
sm = SC.sm


@functools.lru_cache(maxsize=None)
def track(seed, S, T, V):
    """-> the true unknowns P [S,T,62] (fp64, exact in fp32) and the meshes they give [S,T,V,3] fp32"""
    P = SC.track(seed, S, T, V)[0]
    return P, QO.meshes(host_model(V), P).float()


def ones(S, T, V):
    return torch.ones(S, T, V, dtype=torch.float64)


def off_start(P, seed):
    """0.05 off the truth in every model unknown of every frame, exact in fp32"""
    S, T = P.shape[:2]
    P1 = P.clone()
    P1[:, :, :58] += 0.05 * T_(synth.normal_like(seed, "seqv.off", (S, T, 58), 1.0)).double()
    return P1.float().double()


@functools.lru_cache(maxsize=None)
def step_case(V, S, T, metric):
    """the oracle's one step with lambda = 1e-2 and SMOOTH from a start 0.05 off the truth -> targets, weights (None:
    ones), normals (None: Euclidean), the start, the step, its cost.  metric: weights in (0.5, 1.5) with every fifth
    vertex's zero, and the fp32 normals of the targets for _fit_plane_cases.topology(V), tau = TAU"""
    m = host_model(V)
    P, X = track(21, S, T, V)
    P1 = off_start(P, 23)
    w = n = None
    if metric:
        w = (1.0 + 0.5 * np.tanh(synth.normal_like(9700 + V + T, "seqv.w", (S, T, V), 1.0))).astype(np.float32)
        w[:, :, ::5] = 0.0
        w = T_(w)
        n = T_(LO.normals(X.reshape(S * T, V, 3).numpy(), *LC.topology(V)).astype(np.float32)).reshape(S, T, V, 3)
    Ps, c, acc = QO.lm(m, X.double(), ones(S, T, V) if w is None else w.double(), P1, 1, sm(SMOOTH),
                       None if n is None else n.double(), TAU, lambda0=1e-2)
    assert bool((acc == 1).all())
    return X, w, n, P1, Ps, c


@functools.lru_cache(maxsize=None)
def start_case():
    """V = 37, S = 2, T = 5: the tracks of the cost test, and the oracle's start"""
    P, X = track(25, 2, 5, 37)
    return P, X, QO.start(host_model(37), X, ones(2, 5, 37))


GAP_T, GAP_AT, GAP_ITERS = 5, 2, 8


@functools.lru_cache(maxsize=None)
def gap_case():
    """V = 37, S = 1, T = 5, frame 2 without weight -> the meshes, the weights, and the vertex RMS of frame 2 from the
    truth at the oracle's start and after its GAP_ITERS iterations with SMOOTH"""
    m = host_model(37)
    P, X = track(33, 1, GAP_T, 37)
    w = ones(1, GAP_T, 37)
    w[0, GAP_AT] = 0.0
    P0 = QO.start(m, X, w)
    Pf = QO.lm(m, X.double(), w, P0, GAP_ITERS, sm(SMOOTH))[0]
    at = lambda Q: float(QO.rms(m, Q, X)[0, GAP_AT])
    return X, w.float(), at(P0), at(Pf)


# a start far enough for a full Gauss-Newton step (lambda0 tiny) to overshoot: the rejected step of the determinism test
HARD_OFF, HARD_LAMBDA0, HARD_ITERS = 0.6, 1e-9, 6


@functools.lru_cache(maxsize=None)
def hard_case():
    """V = 37, S = 2, T = 3: the meshes and a start HARD_OFF off the truth in the 58 model unknowns (fp32)"""
    P, X = track(35, 2, 3, 37)
    P1 = P.clone()
    P1[:, :, :58] += HARD_OFF * T_(synth.normal_like(37, "seqv.hard", (2, 3, 58), 1.0)).double()
    return X, P1.float()


# ICP parity: V = 37, N = 257, a cloud 3 mm off randomly chosen model vertices of the truth, from a start 0.02 off.  Three
# rounds of one iteration: with 2 x 2 the fourth step of one sequence lowers the cost by less than fp32 resolves, the fp32
# oracle rejects it where fp64 accepts, and the figure then measures two paths, not rounding (the gates tool asserts that
# both precisions accept the same steps)
ICP_N, ICP_ROUNDS, ICP_ITERS, ICP_TRIM = 257, 3, 1, 0.05
ICP_SMOOTH = dict(rots=1e-2, poses=1e-3, betas=1e-1, trans=1.0, scale=1.0)
ICP_MARGIN = 1e-4      # relative best / second-best d2 margin every point must keep: four digits above fp32's error


@functools.lru_cache(maxsize=None)
def icp_case(S, T, gap=None):
    """-> points [S,T,N,3] fp32, the start [S,T,62] fp32 and the topology.  gap: a frame of sequence 0 whose points sit
    1 m away, so that nothing is inside ICP_TRIM"""
    V = 37
    m = host_model(V)
    P, X = track(41, S, T, V)
    rng = np.random.default_rng(4100 + 10 * S + T)
    pick = rng.integers(0, V, size=(S, T, ICP_N))
    pts = np.take_along_axis(X.double().numpy(), pick[..., None], 2) + synth.normal_like(43, "seqv.cloud", (S, T, ICP_N, 3), 0.003)
    if gap is not None:
        pts[0, gap] += 1.0
    P0 = P.clone()
    P0[:, :, :58] += 0.02 * T_(synth.normal_like(45, "seqv.icp.off", (S, T, 58), 1.0)).double()
    return frozen([pts.astype(np.float32)])[0], P0.float(), LC.topology(V)


@functools.lru_cache(maxsize=None)
def icp_run(S, T, plane, gap=None):
    """the oracle's ICP on icp_case -> P, accepted, data cost [S,T], the last assignment, and the smallest nearest-vertex
    margin of any point at the start and at the end (the GPU test needs it above ICP_MARGIN: no assignment flips)"""
    m = host_model(37)
    pts, P0, topo = icp_case(S, T, gap)
    P, acc, dc, a = QO.icp(m, pts, None, P0, topo if plane else None, ICP_ROUNDS, ICP_ITERS, sm(ICP_SMOOTH), TAU, ICP_TRIM)
    margin = np.inf
    for Pk in (P0.double(), P):
        x = QO.meshes(m, Pk).reshape(S * T, 37, 3).numpy()
        am = PO.assign(x, pts.reshape(S * T, ICP_N, 3), None, ICP_TRIM, margins=True)
        d = am["dist"]
        near_trim = np.abs(d - ICP_TRIM).min() / ICP_TRIM
        margin = min(margin, float(am["margin"].min()), float(near_trim))
    return P, acc, dc, a, margin


# The quality case: smooth_model() on the hand surface, QS tracks of QT frames, QN points on the faces of the true meshes
# with N(0, Q_NOISE) m on every coordinate; frame Q_GAP of every track has no points inside the trim (an occluded hand).
QS, QT, QN, Q_NOISE, Q_GAP, Q_TRIM = 1, 8, 512, 1e-3, 4, 0.03
Q_ROUNDS, Q_ITERS = 6, 3
# chosen with tools/fit_seq_verts_gates.py (DESIGN 20 has the table): the penalty is on the velocity, so rots, poses and
# trans, which move, are held loosely (ten times these weights cost the visible frames 1 mm), betas and scale, which do not, firmly
Q_SMOOTH = dict(rots=1e-2, poses=1e-2, betas=10.0, trans=3.0, scale=100.0)


@functools.lru_cache(maxsize=None)
def quality_inputs():
    """-> the true meshes [QS,QT,778,3] fp64, the clouds [QS,QT,QN,3] fp32, the start [QS,QT,62] fp32: the truth + 0.03
    N(0, 1) in the 58 model unknowns and + 3 mm in trans, frame by frame"""
    m = LC.smooth_model()
    base = LC.quality_inputs()[0][:QS]
    vel = np.zeros((QS, 62))
    vel[:, 0:3] = synth.normal_like(51, "seqv.q.rots", (QS, 3), 0.04)
    vel[:, 3:48] = synth.normal_like(51, "seqv.q.poses", (QS, 45), 0.02)
    vel[:, 58:61] = synth.normal_like(51, "seqv.q.trans", (QS, 3), 0.003)
    t = torch.arange(QT, dtype=torch.float64) - 0.5 * (QT - 1)
    P = (base[:, None, :] + t[None, :, None] * T_(vel)[:, None, :]).float().double()
    mesh = QO.meshes(m, P)
    faces = LC.topology(778)[0].astype(np.int64)
    pts = LC.surface_cloud(mesh.reshape(QS * QT, 778, 3).numpy(), faces, QN, 5700).reshape(QS, QT, QN, 3).astype(np.float64)
    pts += synth.normal_like(53, "seqv.q.noise", (QS, QT, QN, 3), Q_NOISE)
    pts[:, Q_GAP] += 1.0
    P0 = P.clone()
    P0[:, :, :58] += 0.03 * T_(synth.normal_like(55, "seqv.q.start", (QS, QT, 58), 1.0)).double()
    P0[:, :, 58:61] += 0.003 * T_(synth.normal_like(55, "seqv.q.start.t", (QS, QT, 3), 1.0)).double()
    return mesh, frozen([pts.astype(np.float32)])[0], P0.float()


def matched_margin(m, P, pts, trim):
    """the smallest best / second-best margin of any matched point of the clouds pts [S,T,N,3] at the model points of P"""
    S, T, N = pts.shape[:3]
    a = PO.assign(QO.meshes(m, P).reshape(S * T, -1, 3).numpy(), pts.reshape(S * T, N, 3), None, trim, margins=True)
    return float(a["margin"][a["matched"]].min())


@functools.lru_cache(maxsize=None)
def quality_case():
    """the oracle's track ICP (point-to-plane, Q_SMOOTH) and per-frame point-to-plane ICP (_fit_plane_oracle.icp on the
    frames flattened), both Q_ROUNDS x Q_ITERS from the same start -> dict of the acceleration error [QS] and the vertex
    RMS [QS,QT] of the start, the per-frame fits and the track fit, the track's P, and the smallest best / second-best margin of any
    matched point at the start and at the end (reported by the gates tool, not gated: a point that close to a tie moves the
    fit by nothing that the figures below could show)"""
    m, topo = LC.smooth_model(), LC.topology(778)
    mesh, pts, P0 = quality_inputs()
    Pf = LO.icp(m, pts.reshape(QS * QT, QN, 3), None, P0.reshape(QS * QT, 62), topo, Q_ROUNDS, Q_ITERS, TAU, Q_TRIM)[0]
    Pf = Pf.reshape(QS, QT, 62)
    Pq = QO.icp(m, pts, None, P0, topo, Q_ROUNDS, Q_ITERS, sm(Q_SMOOTH), TAU, Q_TRIM)[0]
    out = {"P": Pq, "margin": min(matched_margin(m, Q, pts, Q_TRIM) for Q in (P0.double(), Pq))}
    for name, Q in (("start", P0.double()), ("frame", Pf), ("track", Pq)):
        out["accel", name] = QO.accel(m, Q, mesh).numpy()
        out["rms", name] = QO.rms(m, Q, mesh).numpy()
    return out
