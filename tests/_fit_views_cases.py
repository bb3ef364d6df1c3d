"""The fixed inputs of the multi-view fit's tests and what the oracle (tests/_fit_views_oracle.py) makes of them in fp64 and
in fp32, computed once per process and read-only: shared by tests/test_fit_views.py (no GPU), tests/test_gpu_fit_views.py
and tools/fit_views_gates.py.  Needs no GPU.

Rigs: C cameras on a circle of radius 0.5 m around the hand, in the plane y = 0, looking at the origin; fx = fy = 600,
centre (320, 240).  The cameras stand 2 pi / max(C, 3) apart, so that two of them are never face to face (their rays to
a joint near the centre would be parallel).  Truth: _fit_cases.params for the 58 model unknowns, trans ~ N(0, 0.02 m),
log_scale ~ N(0, 0.1)."""
import functools
import math

import numpy as np
import torch

from scat_amd import synth

import _fit_views_oracle as VO
from _fit_cases import JOINT_MAP, T_, host_model, params

RADIUS, FOCAL, CENTRE = 0.5, 600.0, (320.0, 240.0)
ALL = (1 << 62) - 1
BOX = 0.8          # +-0.8 rad: a few of the 45 angles are outside at near_start
W_LIMIT = 1e3      # pixels squared per radian squared
SIGMA2 = 10.0      # pixels
OUTLIER_VIEW = 1


def look_at(phi, height=0.0):
    """the camera at RADIUS (cos phi, height, sin phi) looking at the origin -> 16 floats"""
    o = RADIUS * np.array([math.cos(phi), height, math.sin(phi)])
    z = -o / np.linalg.norm(o)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return np.concatenate([R.reshape(9), -R @ o, [FOCAL, FOCAL, *CENTRE]])


@functools.lru_cache(maxsize=None)
def rig(C, Bc=1, seed=5, dtype=np.float32):
    """cams [Bc,C,16] fp32: Bc = 1 is the regular rig; a rig per sample turns each by a seeded angle and lifts its cameras
    by a seeded height within +-0.1 (times the radius).  dtype np.float64: the same before rounding, whose R are orthonormal
    to fp64"""
    turn = synth.uniform(seed, "views.turn", (Bc,), 0.0, 2 * math.pi) if Bc > 1 else np.full((1,), 0.3)
    lift = synth.uniform(seed, "views.lift", (Bc, C), -0.1, 0.1) if Bc > 1 else np.zeros((1, C))
    step = 2 * math.pi / max(C, 3)
    return T_(np.array([[look_at(float(turn[b]) + c * step, float(lift[b, c])) for c in range(C)] for b in range(Bc)], dtype=dtype))


@functools.lru_cache(maxsize=None)
def truth(V, B, C, per_sample=False, seed=3, pose_sd=1.0):
    """-> P [B,62] fp64 (exactly representable in fp32), X3 [B,21,3] fp64 the true joints, T2 [B,C,21,2] fp32 pixels, cams"""
    m = host_model(V)
    P58 = params(seed + 11 * B, B).copy()
    P58[:, 3:48] *= pose_sd
    P = np.concatenate([P58, synth.normal_like(seed, "views.trans", (B, 3), 0.02), synth.normal_like(seed, "views.log_scale", (B, 1), 0.1)], axis=1)
    P = T_(P.astype(np.float32)).double()
    cams = rig(C, B if per_sample else 1)
    pr = VO.Problem(JOINT_MAP, cams, torch.zeros(B, C, 21, 2))
    with torch.no_grad():
        X3 = VO.model_joints(m, P, JOINT_MAP)
        T2 = VO.reproject(m, P, pr).float()
    return P, X3, T2, cams


@functools.lru_cache(maxsize=None)
def near_start(V, B, C, per_sample=False):
    """the truth moved by 0.05 x N(0, 1) in the 58 model unknowns, fp32-exact"""
    P1 = truth(V, B, C, per_sample)[0].clone()
    P1[:, :58] += 0.05 * T_(synth.normal_like(11, "views.off", (B, 58), 1.0)).double()
    return P1.float().double()


def with_outliers(T2):
    """T2 [B,C,21,2] with every keypoint of view OUTLIER_VIEW moved by 40 to 80 px in a seeded direction, and sel [B,C,21]: the others"""
    B, T2 = T2.shape[0], T2.clone()
    d = T_(synth.normal_like(17, "views.out", (B, 21, 2), 1.0)).float()
    T2[:, OUTLIER_VIEW] += (40.0 + 40.0 * T_(synth.uniform(17, "views.out.len", (B, 21, 1), 0.0, 1.0)).float()) * d / d.norm(dim=2, keepdim=True)
    sel = torch.ones(T2.shape[:3], dtype=torch.bool)
    sel[:, OUTLIER_VIEW] = False
    return T2, sel


@functools.lru_cache(maxsize=None)
def problem(name, V, B, C, per_sample=False):
    """the configurations of the one-step, cost and recovery tests -> Problem"""
    _, _, T2, cams = truth(V, B, C, per_sample)
    box = torch.full((45,), BOX)
    if name == "quad":
        return VO.Problem(JOINT_MAP, cams, T2)
    if name == "gm":
        return VO.Problem(JOINT_MAP, cams, T2, sigma2=SIGMA2)
    if name == "limits":
        return VO.Problem(JOINT_MAP, cams, T2, lo=-box, hi=box, w_limit=W_LIMIT)
    if name == "gm_limits":
        return VO.Problem(JOINT_MAP, cams, with_outliers(T2)[0], lo=-box, hi=box, w_limit=W_LIMIT, sigma2=SIGMA2)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def run(name, V, B, C, per_sample, iters, dtype=torch.float64, lambda0=1e-2, history=False):
    """`iters` iterations of the oracle in dtype from near_start on problem(name) -> (P, cost, accepted[, costs, iterates])"""
    return VO.lm(host_model(V), problem(name, V, B, C, per_sample), near_start(V, B, C, per_sample).to(dtype), iters, lambda0, ALL, history)


def step_e32(name, V, B, C, per_sample):
    """the error of the fp32 oracle's one step against the fp64 oracle's, max |a - b| / max |b|"""
    return VO.rel(run(name, V, B, C, per_sample, 1, torch.float32)[0].numpy(), run(name, V, B, C, per_sample, 1)[0].numpy())


@functools.lru_cache(maxsize=None)
def cost_e32(name, V, B, C, ks=(1, 2, 5, 10)):
    """{k: the oracle's cost function in fp32 against fp64 at its own fp64 iterate after k iterations from near_start}"""
    m, pr = host_model(V), problem(name, V, B, C)
    trace = run(name, V, B, C, False, max(ks), history=True)[4]
    out = {}
    with torch.no_grad():
        for k in ks:
            Pk = trace[k - 1].float()
            out[k] = VO.rel(VO.cost(m, Pk, pr).numpy(), VO.cost(m, Pk.double(), pr).numpy())
    return out


@functools.lru_cache(maxsize=None)
def start_case(V, B, C, per_sample):
    """init = 1 on the quadratic problem -> (Problem, points64, valid, P64, E32 of the points, E32 of the start)"""
    m, pr = host_model(V), problem("quad", V, B, C, per_sample)
    pts, valid = VO.triangulate(pr)
    P64, P32 = VO.start(m, pr)[0], VO.start(m, pr, torch.float32)[0]
    return pr, pts, valid, P64, VO.rel(VO.triangulate(pr, torch.float32)[0].numpy(), pts.numpy()), VO.rel(P32.numpy(), P64.numpy())


@functools.lru_cache(maxsize=None)
def validity_case():
    """V = 37, B = 3, C = 3 with a rig per sample: sample 0's joint 5 is seen by one view, sample 1's joint 6 by none, and in
    sample 2 view 1 stands 0.3 mrad beside view 0 while joint 8 is seen by those two only -> (Problem, points64, valid, E32 of
    the points); all but these three joints are valid"""
    V, B, Cn = 37, 3, 3
    pr = problem("quad", V, B, Cn)
    w2 = torch.ones(B, Cn, 21)
    w2[0, 1:, 5], w2[1, :, 6], w2[2, 2, 8] = 0.0, 0.0, 0.0
    cams = pr.cams.expand(B, -1, -1).clone()
    cams[2, 1] = torch.tensor(look_at(0.3 + 3e-4), dtype=torch.float32)
    with torch.no_grad():
        T2 = VO.reproject(host_model(V), truth(V, B, Cn)[0], pr._replace(cams=cams)).float()
    pr = pr._replace(cams=cams, T2=T2, w2=w2)
    pts, valid = VO.triangulate(pr)
    return pr, pts, valid, VO.rel(VO.triangulate(pr, torch.float32)[0].numpy(), pts.numpy())


RECOVERY = dict(V=37, B=3, C=3, iters=20, lambda0=1e-3, pose_sd=0.5)


@functools.lru_cache(maxsize=None)
def recovery_problem(name="quad"):
    """the recovery cases: milder poses (sd 0.2 rad), C = 3.  "quad": noise-free keypoints, fitted from the triangulated
    start.  "gm_outliers" / "quad_outliers": view OUTLIER_VIEW replaced by outliers, with and without the robust loss, fitted
    from recovery_near(): with a third of the rays wrong the triangulated start is 2 cm off and one of the three hands ends
    in another minimum, in fp64 as in fp32 -> (Problem, X3 the true joints, T2 the clean keypoints, sel the clean view-joints
    or None)"""
    V, B, C = RECOVERY["V"], RECOVERY["B"], RECOVERY["C"]
    _, X3, T2, cams = truth(V, B, C, pose_sd=RECOVERY["pose_sd"])
    if name == "quad":
        return VO.Problem(JOINT_MAP, cams, T2), X3, T2, None
    O2, sel = with_outliers(T2)
    return VO.Problem(JOINT_MAP, cams, O2, sigma2=SIGMA2 if name == "gm_outliers" else 0.0), X3, T2, sel


@functools.lru_cache(maxsize=None)
def recovery_near():
    """the recovery truth moved by 0.05 x N(0, 1) in the 58 model unknowns, fp32-exact"""
    P1 = truth(RECOVERY["V"], RECOVERY["B"], RECOVERY["C"], pose_sd=RECOVERY["pose_sd"])[0].clone()
    P1[:, :58] += 0.05 * T_(synth.normal_like(11, "views.off", (RECOVERY["B"], 58), 1.0)).double()
    return P1.float().double()


def figures(P, name="quad"):
    """the recovery figures of parameters P [B,62], per sample: joint RMS to the true joints in metres, pixel RMS to the
    clean keypoints over the views that were not replaced"""
    pr, X3, T2, sel = recovery_problem(name)
    m = host_model(RECOVERY["V"])
    return VO.joint_rms(m, P, pr, X3).numpy(), VO.pixel_rms(m, P, pr, T2, sel).numpy()


@functools.lru_cache(maxsize=None)
def recovery(name="quad", dtype=torch.float64):
    """the oracle in dtype on recovery_problem(name) -> (P, joint RMS [B], pixel RMS [B])"""
    m, pr = host_model(RECOVERY["V"]), recovery_problem(name)[0]
    if name == "quad":
        P0, fitted = VO.start(m, pr, dtype)
        assert bool(fitted.all())
    else:
        P0 = recovery_near().to(dtype)
    P = VO.lm(m, pr, P0, RECOVERY["iters"], RECOVERY["lambda0"])[0]
    return (P,) + figures(P, name)
