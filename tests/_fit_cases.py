"""The fixed inputs of the MANO fit's tests and what the fp64 oracle (tests/_fit_oracle.py) makes of them, computed once per
process and read-only: shared by tests/test_fit.py (no GPU), tests/test_gpu_fit.py and tools/fit_gates.py.  Needs no GPU."""
import functools

import numpy as np
import torch

from scat_amd import synth

import _fit_oracle as FO

T_ = lambda a: torch.from_numpy(np.array(a))      # a copy: the shared inputs are read-only
# target joint j is the model's joint JOINT_MAP[j]: wrist, then thumb, index, middle, ring, pinky with their tips
JOINT_MAP = (0, 13, 14, 15, 20, 1, 2, 3, 16, 4, 5, 6, 17, 10, 11, 12, 19, 7, 8, 9, 18)


@functools.lru_cache(maxsize=None)
def host_model(V, seed=300):
    """V = "edge": 778 vertices and hands_mean = 0, so that the finger angles are poses themselves and the tiny angles of
    the edge batch reach the 15 chain rotations.  On the host: what the oracle reads."""
    from scat_amd.mano import ManoModel

    if V != "edge":
        return ManoModel.synthetic(seed + V, V)
    m = ManoModel.synthetic(341, 778)
    arrays = {k: getattr(m, k) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")}
    return ManoModel.from_arrays(dict(arrays, hands_mean=np.zeros(45, np.float32), tips=m.tips))


def frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


def params(seed, B):
    """rots ~ N(0, 0.8), poses ~ N(0, 0.4), betas ~ N(0, 1) as one [B,58] fp32 array"""
    return np.concatenate([synth.normal_like(seed, "rots", (B, 3), 0.8), synth.normal_like(seed, "poses", (B, 45), 0.4),
                           synth.normal_like(seed, "betas", (B, 10), 1.0)], axis=1)


@functools.lru_cache(maxsize=None)
def case(B, V):
    P = params(7000 + 7 * B + V, B)
    x, jac = FO.joints_jac(host_model(V), T_(P).double())
    return frozen([P]) + frozen([x.numpy(), jac.numpy()])


@functools.lru_cache(maxsize=None)
def edge_batch():
    """B = 8 on the hands_mean = 0 model, every angle of sample b (rots and the 15 fingers): 0 exactly zero, betas zero
    too; 1 components of 1e-20; 2 of 1e-6; 3 of 1e-3; 4, 5 theta^2 just below and just above 0.25, where the kernel
    switches from the series to the closed form; 6 theta = pi; 7 ordinary angles, betas = +-3"""
    P = params(7100, 8)
    P[0] = 0.0
    for b, eps in ((1, 1e-20), (2, 1e-6), (3, 1e-3), (4, 0.4999 / np.sqrt(3.0)), (5, 0.5001 / np.sqrt(3.0)),
                   (6, np.pi / np.sqrt(3.0))):
        P[b, :48] = np.float32(eps)
    t = (P[4:6, :3].astype(np.float64) ** 2).sum(1)
    assert t[0] < 0.25 < t[1]
    P[7, 48:] = 3.0 * np.where(np.arange(10) % 2 == 0, 1.0, -1.0)
    x, jac = FO.joints_jac(host_model("edge"), T_(P).double())
    return frozen([P]) + frozen([x.numpy(), jac.numpy()])


@functools.lru_cache(maxsize=None)
def recovery_case(V):
    """B = 6 seeded hands, the oracle's start and its 20 iterations from there (with their costs), computed once"""
    m = host_model(V)
    P, T = FO.seeded_case(3, 6, m, JOINT_MAP)
    w = torch.ones(6, 21, dtype=torch.float64)
    P0 = FO.procrustes_start(m, T, w, JOINT_MAP)
    Pf, c, acc, hist = FO.lm(m, T.double(), w, JOINT_MAP, P0, 20, history=True)
    return P, T, P0, Pf, FO.rms(m, Pf, T, JOINT_MAP).numpy(), hist.numpy()


@functools.lru_cache(maxsize=None)
def step_case(V):
    """a start 0.05 off the truth in every model unknown, and the oracle's one step from there with lambda = 1e-2"""
    m = host_model(V)
    P, T = FO.seeded_case(3, 6, m, JOINT_MAP)
    P1 = P.clone()
    P1[:, :58] += 0.05 * T_(synth.normal_like(11, "fit.off", (6, 58), 1.0)).double()
    P1 = P1.float().double()
    Ps, c, acc = FO.lm(m, T.double(), torch.ones(6, 21, dtype=torch.float64), JOINT_MAP, P1, 1, lambda0=1e-2)
    assert bool((acc == 1).all())
    return T, P1, Ps, c
