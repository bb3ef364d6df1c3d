"""The fixed inputs of the multi-view track fit's tests and what the oracle (tests/_fit_seq_views_oracle.py) makes of them
in fp64 and in fp32, computed once per process and read-only: shared by tests/test_fit_seq_views.py (no GPU),
tests/test_gpu_fit_seq_views.py and tools/fit_seq_views_gates.py.  Needs no GPU.

Rigs: _fit_views_cases.rig (C cameras on a circle of 0.5 m around the hand, fx = fy = 600).  Truth: _fit_views_cases.truth
at the middle of the track and a smooth motion along t: a constant velocity and a constant acceleration per sequence in
rots and poses (about 0.03 rad and 0.004 rad per frame) and in trans (2 mm and 0.3 mm per frame); betas and the scale are
constant along a track."""
import functools
import math

import numpy as np
import torch

from scat_amd import synth

import _fit_seq_views_oracle as QO
import _fit_views_cases as VC
import _fit_views_oracle as VO
from _fit_cases import JOINT_MAP, T_, host_model

ALL = VC.ALL
BOX, W_LIMIT, SIGMA2, OUTLIER_VIEW = VC.BOX, VC.W_LIMIT, VC.SIGMA2, VC.OUTLIER_VIEW
# pixels squared per (radian, radian, shape unit, metre, log-ratio) squared: at 100 px / rad and 1200 px / m (the header's
# UNITS) a step of 0.03 rad or 2 mm per frame costs about as much as a residual of a pixel in every view-joint
SMOOTH = (30.0, 30.0, 1e3, 3e4, 1e3)
NOISE_PX = 1.0


@functools.lru_cache(maxsize=None)
def truth(V, S, T, C, per=False, seed=3, pose_sd=1.0, wrap=False):
    """-> P [S,T,62] fp64 (exactly representable in fp32), X3 [S,T,21,3] fp64 the true joints, T2 [S,T,C,21,2] fp32 pixels,
    cams [Sc,C,16].  wrap: the last sequence's rots run along one axis from the angle pi - 0.6 to pi + 0.6, where the
    frames' own starts jump to the other representation"""
    m = host_model(V)
    P0 = VC.truth(V, S, C, per, seed, pose_sd)[0]
    vel = torch.zeros(S, 62, dtype=torch.float64)
    vel[:, :48] = T_(synth.normal_like(seed + 1, "seqviews.vel", (S, 48), 0.03)).double()
    vel[:, 58:61] = T_(synth.normal_like(seed + 1, "seqviews.vel.t", (S, 3), 0.002)).double()
    acc = torch.zeros(S, 62, dtype=torch.float64)
    acc[:, :48] = T_(synth.normal_like(seed + 2, "seqviews.acc", (S, 48), 0.004)).double()
    acc[:, 58:61] = T_(synth.normal_like(seed + 2, "seqviews.acc.t", (S, 3), 0.0003)).double()
    dt = torch.arange(T, dtype=torch.float64) - 0.5 * (T - 1)
    P = P0[:, None, :] + dt[None, :, None] * vel[:, None, :] + 0.5 * (dt ** 2)[None, :, None] * acc[:, None, :]
    if wrap:
        u = torch.tensor([0.6, 0.0, 0.8], dtype=torch.float64)
        P[S - 1, :, :3] = u[None, :] * (math.pi - 0.6 + 1.2 / (T - 1) * torch.arange(T, dtype=torch.float64))[:, None]
    P = P.float().double()
    cams = VC.rig(C, S if per else 1)
    pr = QO.Problem(JOINT_MAP, cams, torch.zeros(S, T, C, 21, 2))
    with torch.no_grad():
        X3 = QO.frame_joints(m, P, JOINT_MAP)
        T2 = VO.reproject(m, P.reshape(S * T, 62), QO.frames(pr)).float().reshape(S, T, C, 21, 2)
    return P, X3, T2, cams


@functools.lru_cache(maxsize=None)
def near_start(V, S, T, C, per=False, pose_sd=1.0):
    """the truth moved by 0.05 x N(0, 1) in the 58 model unknowns, the same offset in every frame of a sequence, fp32-exact"""
    P1 = truth(V, S, T, C, per, pose_sd=pose_sd)[0].clone()
    P1[:, :, :58] += 0.05 * T_(synth.normal_like(11, "seqviews.off", (S, 1, 58), 1.0)).double()
    return P1.float().double()


def with_outliers(T2):
    """T2 [S,T,C,21,2] with every keypoint of view OUTLIER_VIEW moved by 40 to 80 px in a seeded direction, and sel: the others"""
    S, T = T2.shape[:2]
    O2, sel = VC.with_outliers(T2.flatten(0, 1))
    return O2.reshape(T2.shape), sel.reshape(T2.shape[:4])


def with_noise(T2, seed=19):
    """T2 with N(0, NOISE_PX) on every pixel coordinate"""
    return T2 + NOISE_PX * T_(synth.normal_like(seed, "seqviews.noise", tuple(T2.shape), 1.0)).float()


@functools.lru_cache(maxsize=None)
def problem(name, V, S, T, C, per=False):
    """the configurations of the one-step and cost tests -> Problem"""
    _, _, T2, cams = truth(V, S, T, C, per)
    box = torch.full((45,), BOX)
    if name == "quad":
        return QO.Problem(JOINT_MAP, cams, T2, smooth=SMOOTH)
    if name == "gm":
        return QO.Problem(JOINT_MAP, cams, T2, sigma2=SIGMA2, smooth=SMOOTH)
    if name == "limits":
        return QO.Problem(JOINT_MAP, cams, T2, lo=-box, hi=box, w_limit=W_LIMIT, smooth=SMOOTH)
    if name == "gm_limits":
        return QO.Problem(JOINT_MAP, cams, with_outliers(T2)[0], lo=-box, hi=box, w_limit=W_LIMIT, sigma2=SIGMA2, smooth=SMOOTH)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def run(name, V, S, T, C, per, iters, dtype=torch.float64, lambda0=1e-2, history=False):
    """`iters` iterations of the oracle in dtype from near_start on problem(name) -> (P, cost, accepted[, costs, iterates])"""
    return QO.lm(host_model(V), problem(name, V, S, T, C, per), near_start(V, S, T, C, per).to(dtype), iters, lambda0, ALL, history)


def step_e32(name, V, S, T, C, per):
    """the error of the fp32 oracle's one step against the fp64 oracle's, max |a - b| / max |b|"""
    return QO.rel(run(name, V, S, T, C, per, 1, torch.float32)[0].numpy(), run(name, V, S, T, C, per, 1)[0].numpy())


@functools.lru_cache(maxsize=None)
def cost_e32(name, V, S, T, C, ks=(1, 2, 5, 10)):
    """{k: the oracle's cost function in fp32 against fp64 at its own fp64 iterate after k iterations from near_start}"""
    m, pr = host_model(V), problem(name, V, S, T, C)
    trace = run(name, V, S, T, C, False, max(ks), history=True)[4]
    out = {}
    with torch.no_grad():
        for k in ks:
            Pk = trace[k - 1].float()
            out[k] = QO.rel(QO.cost(m, Pk, pr).numpy(), QO.cost(m, Pk.double(), pr).numpy())
    return out


@functools.lru_cache(maxsize=None)
def start_case(V, S, T, C, per):
    """init = 1 on noise-free keypoints -> (Problem, P64, has, E32 of the start).  From T = 3 on the track has what the scan
    is for: frame 1 of sequence 0 is seen by one camera only (no start: it takes frame 0's), and from S = 2 on frame 0 of
    sequence 1 is seen by none (it takes frame 1's) and the last sequence crosses the angle pi (the unwrap)"""
    scan = T >= 3
    _, _, T2, cams = truth(V, S, T, C, per, wrap=scan and S >= 2)
    w2 = None
    if scan:
        w2 = torch.ones(S, T, C, 21)
        w2[0, 1, 1:] = 0.0
        if S >= 2:
            w2[1, 0] = 0.0
    pr = QO.Problem(JOINT_MAP, cams, T2, w2, smooth=SMOOTH)
    m = host_model(V)
    P64, has, fitted = QO.start(m, pr)
    P32 = QO.start(m, pr, torch.float32)[0]
    assert bool(fitted.all())
    return pr, P64, has, QO.rel(P32.numpy(), P64.numpy())


RECOVERY = dict(V=37, S=3, T=5, C=3, iters=20, lambda0=1e-3, pose_sd=0.5)
RECOVERY_CASES = ("clean", "noise", "outliers", "single_view", "unseen")
GAP_FRAME = 2


@functools.lru_cache(maxsize=None)
def recovery_problem(name="clean"):
    """the recovery cases on milder poses, S = 3 tracks of T = 5 frames, C = 3 -> (Problem, X3 the true joints, T2 the clean
    keypoints, sel the clean view-joints or None).
      clean        noise-free keypoints, from the triangulated start
      noise        N(0, 1 px) on every coordinate, from the triangulated start
      outliers     view OUTLIER_VIEW replaced by outliers in every frame, Geman-McClure, from recovery_near()
      single_view  noise as above; frame GAP_FRAME of every track is seen by camera 0 only: no start of its own, rows that count
      unseen       noise as above; frame GAP_FRAME of every track is seen by no camera: bridged by smoothness"""
    V, S, T, C = (RECOVERY[k] for k in "VSTC")
    _, X3, T2, cams = truth(V, S, T, C, pose_sd=RECOVERY["pose_sd"])
    if name == "clean":
        return QO.Problem(JOINT_MAP, cams, T2, smooth=SMOOTH), X3, T2, None
    if name == "outliers":
        O2, sel = with_outliers(T2)
        return QO.Problem(JOINT_MAP, cams, O2, sigma2=SIGMA2, smooth=SMOOTH), X3, T2, sel
    w2 = torch.ones(S, T, C, 21)
    if name == "single_view":
        w2[:, GAP_FRAME, 1:] = 0.0
    elif name == "unseen":
        w2[:, GAP_FRAME] = 0.0
    elif name != "noise":
        raise KeyError(name)
    return QO.Problem(JOINT_MAP, cams, with_noise(T2), w2, smooth=SMOOTH), X3, T2, None


@functools.lru_cache(maxsize=None)
def recovery_near():
    return near_start(RECOVERY["V"], RECOVERY["S"], RECOVERY["T"], RECOVERY["C"], pose_sd=RECOVERY["pose_sd"])


def figures(P, name="clean"):
    """the recovery figures of parameters P [S,T,62], per sequence: joint RMS to the true joints in metres, pixel RMS to
    the clean keypoints over the views that were not replaced, and the joint RMS of frame GAP_FRAME alone"""
    pr, X3, T2, sel = recovery_problem(name)
    m = host_model(RECOVERY["V"])
    return (QO.joint_rms(m, P, pr, X3).numpy(), QO.pixel_rms(m, P, pr, T2, sel).numpy(),
            QO.frame_joint_rms(m, P, pr, X3)[:, GAP_FRAME].numpy())


@functools.lru_cache(maxsize=None)
def recovery(name="clean", dtype=torch.float64):
    """the oracle in dtype on recovery_problem(name) -> (P, joint RMS [S], pixel RMS [S], joint RMS of the gap frame [S],
    the last two costs [2,S])"""
    m, pr = host_model(RECOVERY["V"]), recovery_problem(name)[0]
    if name == "outliers":
        P0 = recovery_near().to(dtype)
    else:
        P0, _, fitted = QO.start(m, pr, dtype)
        assert bool(fitted.all())
    P, _, _, hist, _ = QO.lm(m, pr, P0, RECOVERY["iters"], RECOVERY["lambda0"], history=True)
    return (P,) + figures(P, name) + (hist[-2:],)


@functools.lru_cache(maxsize=None)
def per_frame(name="noise", dtype=torch.float64):
    """_fit_views_oracle.lm frame by frame on the same keypoints (the frames that have a start of their own) -> P [S,T,62];
    a frame without a start keeps zeros"""
    m, pr = host_model(RECOVERY["V"]), recovery_problem(name)[0]
    fr = QO.frames(pr)
    P0, fitted = VO.start(m, fr, dtype)
    P = VO.lm(m, fr, P0, RECOVERY["iters"], RECOVERY["lambda0"])[0]
    return P.reshape(RECOVERY["S"], RECOVERY["T"], 62)
