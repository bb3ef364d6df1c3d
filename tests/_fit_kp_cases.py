"""The fixed inputs of the keypoint fit's tests and what the oracle (tests/_fit_kp_oracle.py) makes of them in fp64 and in
fp32, computed once per process and read-only: shared by tests/test_fit_kp.py (no GPU), tests/test_gpu_fit_kp.py and
tools/fit_kp_gates.py.  Needs no GPU.  Built from _fit_cases.host_model, JOINT_MAP and _fit_oracle.seeded_case.

Beside every fp64 result that a GPU gate reads there is E32, the error of the fp32 oracle against it on the same inputs
(max |a - b| / max |b|): the gate is 4 x E32."""
import functools

import numpy as np
import torch

from scat_amd import synth

import _fit_kp_oracle as KO
import _fit_oracle as FO
from _fit_cases import JOINT_MAP, T_, host_model

HALF = (112.0, 112.0)
W2 = 1e-6                                   # a pixel counts like a millimetre beside targets in metres
FREE_2D = ((1 << 62) - 1) & ~(0xF << 58)    # everything but trans and log_scale
OUTLIERS = 3


@functools.lru_cache(maxsize=None)
def truth(V, B=6, seed=3):
    """-> P [B,65] fp64 (exactly representable in fp32), T3 [B,21,3] fp32, T2 [B,21,2] fp32 pixels: the seeded hands of
    the 3-D fit's tests under a camera s in 3..5, tx, ty in -0.05..0.05"""
    m = host_model(V)
    P62, T3 = FO.seeded_case(seed, B, m, JOINT_MAP)
    cam = np.stack([synth.uniform(seed, "kp.cam.s", (B,), 3.0, 5.0), synth.uniform(seed, "kp.cam.tx", (B,), -0.05, 0.05),
                    synth.uniform(seed, "kp.cam.ty", (B,), -0.05, 0.05)], axis=1).astype(np.float32)
    P = torch.cat([P62, T_(cam).double()], dim=1)
    with torch.no_grad():
        T2 = KO.reproject(m, P, JOINT_MAP, HALF).float()
    return P, T3, T2


@functools.lru_cache(maxsize=None)
def near_start(V, B=6, seed=3):
    """the truth moved by 0.05 x N(0, 1) in the 58 model unknowns, fp32-exact"""
    P, _, _ = truth(V, B, seed)
    P1 = P.clone()
    P1[:, :58] += 0.05 * T_(synth.normal_like(11, "fit.off", (B, 58), 1.0)).double()
    return P1.float().double()


@functools.lru_cache(maxsize=None)
def outlier_targets(V, B=6, seed=3):
    """-> T3, T2 with three joints per hand moved by 5 cm / 40 px in a seeded direction, and inl [B,21] bool, the others"""
    _, T3, T2 = truth(V, B, seed)
    T3, T2, inl = T3.clone(), T2.clone(), torch.ones(B, 21, dtype=torch.bool)
    d3 = T_(synth.normal_like(17, "kp.out3", (B, OUTLIERS, 3), 1.0)).float()
    d2 = T_(synth.normal_like(17, "kp.out2", (B, OUTLIERS, 2), 1.0)).float()
    for b in range(B):
        for k in range(OUTLIERS):
            j = (4 + 7 * k + 3 * b) % 21
            T3[b, j] += 0.05 * d3[b, k] / d3[b, k].norm()
            T2[b, j] += 40.0 * d2[b, k] / d2[b, k].norm()
            inl[b, j] = False
    return T3, T2, inl


BOX = 0.3
# At near_start 17 to 30 of the 45 finger angles are outside +-0.3, and the oracle's first step at lambda = 1e-2 is rejected
# on every sample: the one-step test, which wants an accepted step, takes a box of +-0.8 instead.
WIDE_BOX = 0.8


@functools.lru_cache(maxsize=None)
def problem(name, V, B=6):
    """the configurations of the one-step, cost and recovery tests -> (Problem, free, free_cam)"""
    _, T3, T2 = truth(V, B)
    w2 = torch.full((B, 21), W2)
    box = (torch.full((45,), -BOX), torch.full((45,), BOX))
    if name == "both":
        return KO.Problem(JOINT_MAP, T3=T3, T2=T2, w2=w2, half=HALF), (1 << 62) - 1, 7
    if name == "2d":
        return KO.Problem(JOINT_MAP, T2=T2, half=HALF), FREE_2D, 7
    if name == "3d":      # scat_mano_fit's problem
        return KO.Problem(JOINT_MAP, T3=T3, half=HALF), (1 << 62) - 1, 0
    if name in ("gm", "quad_outliers", "gm_limits"):
        O3, O2, _ = outlier_targets(V, B)
        s3, s2 = (0.0, 0.0) if name == "quad_outliers" else (0.01, 10.0)
        lim = dict(lo=box[0], hi=box[1], w_limit=1e-2) if name == "gm_limits" else {}
        return KO.Problem(JOINT_MAP, T3=O3, T2=O2, w2=w2, sigma3=s3, sigma2=s2, half=HALF, **lim), (1 << 62) - 1, 7
    if name == "limits_wide":      # the one-step case: 1 to 4 limits active per hand at near_start, and the step is accepted
        wide = torch.full((45,), WIDE_BOX)
        return KO.Problem(JOINT_MAP, T3=T3, T2=T2, w2=w2, lo=-wide, hi=wide, w_limit=1e-2, half=HALF), (1 << 62) - 1, 7
    if name == "limits":           # condition (b)
        return KO.Problem(JOINT_MAP, T3=T3, T2=T2, w2=w2, lo=box[0], hi=box[1], w_limit=1e-2, half=HALF), (1 << 62) - 1, 7
    if name == "2d_prior":      # condition (c)
        return KO.Problem(JOINT_MAP, T2=T2, w_pose=1e-3, w_beta=1e-3, half=HALF), FREE_2D, 7
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def run(name, V, iters, B=6, lambda0=1e-2):
    """`iters` iterations of the fp64 oracle from near_start on problem(name) -> (P, cost, accepted)"""
    pr, free, fc = problem(name, V, B)
    return KO.lm(host_model(V), pr, near_start(V, B), iters, lambda0, free, fc)


@functools.lru_cache(maxsize=None)
def run32(name, V, iters, B=6, lambda0=1e-2):
    """the same in fp32 -> (P32, E32): the error of its p against run()'s, max |a - b| / max |b|"""
    pr, free, fc = problem(name, V, B)
    P32 = KO.lm(host_model(V), pr, near_start(V, B).float(), iters, lambda0, free, fc)[0]
    return P32, KO.rel(P32.numpy(), run(name, V, iters, B, lambda0)[0].numpy())


@functools.lru_cache(maxsize=None)
def cost_e32(name, V, ks=(1, 2, 5, 10), B=6, lambda0=1e-2):
    """{k: the oracle's cost function in fp32 against fp64 at its own fp64 iterate after k iterations from near_start}"""
    m = host_model(V)
    pr, free, fc = problem(name, V, B)
    trace = KO.lm(m, pr, near_start(V, B), max(ks), lambda0, free, fc, history=True)[4]
    out = {}
    with torch.no_grad():
        for k in ks:
            Pk = trace[k - 1].float()
            out[k] = KO.rel(KO.cost(m, Pk, pr).numpy(), KO.cost(m, Pk.double(), pr).numpy())
    return out


def mirrored_targets(V):
    """B = 4 hands at the zero pose seen by a camera: 0 an in-plane rotation of 0.4, 1 of 2.5 (beyond pi / 2), 2 mirrored
    (Rz(0.7) Ry(pi)), 3 mirrored and rotated by -2.2 -> P [4,65] fp64, T2 fp32"""
    m = host_model(V)
    P = torch.zeros(4, 65, dtype=torch.float64)
    R = lambda phi, mir: np.array([[np.cos(phi), -np.sin(phi), 0], [np.sin(phi), np.cos(phi), 0], [0, 0, 1.0]]) @ \
        (np.diag([-1.0, 1.0, -1.0]) if mir else np.eye(3))
    Rs = np.stack([R(0.4, False), R(2.5, False), R(0.7, True), R(-2.2, True)])
    P[:, 0:3] = FO.rot_to_axis_angle(torch.from_numpy(Rs)).float().double()
    P[:, 62], P[:, 63], P[:, 64] = T_(np.float32([3.5, 4.0, 3.0, 4.5])).double(), 0.02, -0.03
    P = P.float().double()
    with torch.no_grad():
        T2 = KO.reproject(m, P, JOINT_MAP, HALF).float()
    return P, T2


@functools.lru_cache(maxsize=None)
def start_case(kind, V, B):
    """init = 1 -> (Problem, P64, E32).  kind "3d": both terms, the Procrustes branch with the camera; "2d": the seeded
    hands from 2-D alone; "mirror": mirrored_targets (B = 4)"""
    m = host_model(V)
    if kind == "mirror":
        pr = KO.Problem(JOINT_MAP, T2=mirrored_targets(V)[1], half=HALF)
    else:
        pr = problem("both" if kind == "3d" else "2d", V, B)[0]
    P64, P32 = KO.start(m, pr, B), KO.start(m, pr, B, torch.float32)
    return pr, P64, KO.rel(P32.numpy(), P64.numpy())


@functools.lru_cache(maxsize=None)
def condition_c(V, dtype=torch.float64, B=6, iters=40):
    """2-D only from the closed-form start, w_pose = w_beta = 1e-3, lambda0 = 1e-3 -> (Problem, reprojection RMS of the
    start, of the oracle in dtype after `iters` iterations), pixels"""
    m = host_model(V)
    pr, free, fc = problem("2d_prior", V, B)
    P0 = KO.start(m, pr, B, dtype)
    Pf = KO.lm(m, pr, P0, iters, 1e-3, free, fc)[0]
    return pr, KO.rms2(m, P0, pr.T2, JOINT_MAP, HALF).numpy(), KO.rms2(m, Pf, pr.T2, JOINT_MAP, HALF).numpy()


def recovery_figures(name, V, P, B=6):
    """what the recovery gates hold for parameters P [B,65] on problem(name): the 3-D joint RMS (None without a 3-D term)
    and the reprojection RMS in pixels, against the clean targets, over the inliers for the outlier cases"""
    m = host_model(V)
    _, T3, T2 = truth(V, B)
    pr, _, _ = problem(name, V, B)
    sel = outlier_targets(V, B)[2] if name in ("gm", "quad_outliers", "gm_limits") else torch.ones(B, 21, dtype=torch.bool)
    r2 = KO.rms2(m, P, T2, JOINT_MAP, HALF, sel).numpy()
    if pr.T3 is None:
        return None, r2
    with torch.no_grad():
        d = ((KO.model_joints(m, P.double(), JOINT_MAP) - T3.double()) ** 2).sum(2)
    return ((d * sel).sum(1) / sel.sum(1)).sqrt().numpy(), r2


def px_floor(V, B=6):
    """1e-5 m in pixels, per sample: 1e-5 half cs_true"""
    return 1e-5 * HALF[0] * truth(V, B)[0][:, 62].numpy()
