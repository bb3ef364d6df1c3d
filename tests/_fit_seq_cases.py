"""The fixed inputs of the sequence fit's tests and what the fp64 oracle (tests/_fit_seq_oracle.py) makes of them, computed
once per process and read-only: shared by tests/test_fit_seq.py (no GPU), tests/test_gpu_fit_seq.py and
tools/fit_seq_gates.py.  Models and the joint order are _fit_cases'.  Needs no GPU.

A track is linear in the unknowns: P[s,t] = base[s] + (t - (T - 1) / 2) vel[s], the base from _fit_oracle.seeded_case's
distributions, the velocity per frame N(0, 0.06) in rots, N(0, 0.03) in poses, N(0, 0.004) in trans, none in betas and
log_scale: a hand that turns, flexes and drifts and does not change size."""
import functools

import numpy as np
import torch

from scat_amd import synth

import _fit_oracle as FO
import _fit_seq_oracle as SO
from _fit_cases import JOINT_MAP, T_, host_model

# the smoothness the step, cost, start and gap cases run with (rots, poses, betas, trans, scale); units in the header
SMOOTH = dict(rots=1e-3, poses=1e-4, betas=1e-2, trans=1e-1, scale=1e-1)
# the smoothing case: targets with N(0, NOISE) m on every coordinate, T frames, and a smoothness that outweighs the data
# in what the data leaves loose.  Chosen so that condition (a) of tests/test_fit_seq.py holds; recorded there.
NOISE, NOISE_T, NOISE_S, NOISE_ITERS = 2e-3, 8, 2, 6
SMOOTH_NOISY = dict(rots=3e-2, poses=1e-2, betas=1e-1, trans=3.0, scale=1.0)


def sm(smooth):
    return tuple(float(smooth[k]) for k in ("rots", "poses", "betas", "trans", "scale"))


@functools.lru_cache(maxsize=None)
def track(seed, S, T, V):
    """-> the true unknowns P [S,T,62] (fp64, exactly representable in fp32) and the targets they give [S,T,21,3] fp32"""
    m = host_model(V)
    base, _ = FO.seeded_case(seed, S, m, JOINT_MAP)
    vel = np.zeros((S, 62))
    vel[:, 0:3] = synth.normal_like(seed, "seq.vel.rots", (S, 3), 0.06)
    vel[:, 3:48] = synth.normal_like(seed, "seq.vel.poses", (S, 45), 0.03)
    vel[:, 58:61] = synth.normal_like(seed, "seq.vel.trans", (S, 3), 0.004)
    t = torch.arange(T, dtype=torch.float64) - 0.5 * (T - 1)
    P = (base[:, None, :] + t[None, :, None] * T_(vel)[:, None, :]).float().double()
    with torch.no_grad():
        X = FO.model_joints(m, P.reshape(S * T, 62), JOINT_MAP).float().reshape(S, T, 21, 3)
    return P, X


def ones(S, T):
    return torch.ones(S, T, 21, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def step_case(V, S, T):
    """a start 0.05 off the truth in every model unknown of every frame, and the oracle's one step from there with
    lambda = 1e-2 and SMOOTH -> targets, the start, the step, its cost"""
    m = host_model(V)
    P, X = track(21, S, T, V)
    P1 = P.clone()
    P1[:, :, :58] += 0.05 * T_(synth.normal_like(23, "seq.off", (S, T, 58), 1.0)).double()
    P1 = P1.float().double()
    Ps, c, acc = SO.lm(m, X.double(), ones(S, T), JOINT_MAP, P1, 1, sm(SMOOTH), lambda0=1e-2)
    assert bool((acc == 1).all())
    return X, P1, Ps, c


@functools.lru_cache(maxsize=None)
def start_case():
    """V = 37, S = 2, T = 5: the tracks of the cost test, and the oracle's start"""
    P, X = track(25, 2, 5, 37)
    return P, X, SO.start(host_model(37), X, ones(2, 5), JOINT_MAP)


@functools.lru_cache(maxsize=None)
def pi_case():
    """V = 37, S = 1, T = 5: a global rotation about a fixed axis whose angle goes 2.7 .. 3.5, across pi between frames 2
    and 3, everything else at rest -> truth, targets, the oracle's start"""
    m = host_model(37)
    base, _ = FO.seeded_case(27, 1, m, JOINT_MAP)
    axis = np.array([0.36, -0.48, 0.8])
    P = base[:, None, :].repeat(1, 5, 1).clone()
    for t, ang in enumerate((2.7, 2.9, 3.1, 3.3, 3.5)):
        P[0, t, :3] = T_(ang * axis)
    P = P.float().double()
    with torch.no_grad():
        X = FO.model_joints(m, P.reshape(5, 62), JOINT_MAP).float().reshape(1, 5, 21, 3)
    return P, X, SO.start(m, X, ones(1, 5), JOINT_MAP)


def per_frame(m, X, iters, dt):
    """the frames fitted one by one, as ManoFitter.fit would: [S,T,62]"""
    S, T = X.shape[:2]
    Xf, w = X.reshape(S * T, 21, 3), torch.ones(S * T, 21, dtype=torch.float64)
    P0 = FO.procrustes_start(m, Xf, w, JOINT_MAP)
    return FO.lm(m, Xf.to(dt), w.to(dt), JOINT_MAP, P0.to(dt), iters)[0].reshape(S, T, 62)


@functools.lru_cache(maxsize=None)
def noisy_case():
    """V = 37: NOISE_S tracks of NOISE_T frames with noisy targets -> the true joints, the noisy targets, and the
    accel_error against the truth of the oracle's sequence fit and of its per-frame fits, each in fp64 and in fp32"""
    m, S, T = host_model(37), NOISE_S, NOISE_T
    P, X = track(29, S, T, 37)
    Xn = (X.double() + NOISE * T_(synth.normal_like(31, "seq.noise", (S, T, 21, 3), 1.0)).double()).float()
    P0 = SO.start(m, Xn, ones(S, T), JOINT_MAP)
    out = {}
    for name, dt in (("fp64", torch.float64), ("fp32", torch.float32)):
        Pq = SO.lm(m, Xn.to(dt), ones(S, T).to(dt), JOINT_MAP, P0.to(dt), NOISE_ITERS, sm(SMOOTH_NOISY))[0]
        out["seq", name] = SO.accel(m, Pq, JOINT_MAP, X).numpy()
        out["frame", name] = SO.accel(m, per_frame(m, Xn, NOISE_ITERS, dt), JOINT_MAP, X).numpy()
    return X, Xn, out


GAP_T, GAP_AT, GAP_ITERS = 5, 2, 8


@functools.lru_cache(maxsize=None)
def gap_case():
    """V = 37, S = 1, T = 5, frame 2 without weight -> the true joints, the targets, the weights, and the distance (RMS
    over the joints) of frame 2 from the truth at the oracle's start and after its GAP_ITERS iterations with SMOOTH"""
    m = host_model(37)
    P, X = track(33, 1, GAP_T, 37)
    w = ones(1, GAP_T)
    w[0, GAP_AT] = 0.0
    P0 = SO.start(m, X, w, JOINT_MAP)
    Pf = SO.lm(m, X.double(), w, JOINT_MAP, P0, GAP_ITERS, sm(SMOOTH))[0]
    rms = lambda Q: float(((SO.frame_joints(m, Q, JOINT_MAP)[0, GAP_AT] - X[0, GAP_AT].double()) ** 2).sum(1).mean().sqrt())
    return X, w.float(), rms(P0), rms(Pf)
