"""The fixed inputs of the tests of the MANO fit to a full mesh and what the fp64 oracle (tests/_fit_verts_oracle.py) makes of
them, computed once per process and read-only: shared by tests/test_fit_verts.py (no GPU), tests/test_gpu_fit_verts.py and
tools/fit_verts_gates.py.  The models, the parameter distributions and the edge batch are _fit_cases.py's.  Needs no GPU."""
import functools

import torch

from scat_amd import synth

import _fit_oracle as FO
import _fit_verts_oracle as VO
from _fit_cases import JOINT_MAP, T_, edge_batch, frozen, host_model, params

JAC_V, JAC_B = (1, 37, 778, 1536), (1, 3, 65)      # V = 1536: SCAT_MANO_MAX_V
FIT_V = (37, 778)
NB = 6                                             # hands of the recovery and step cases
ITERS = (1, 5, 20)


@functools.lru_cache(maxsize=None)
def case(B, V):
    """-> P [B,58] fp32, verts [B,V,3], jac [B,3V,58] (the oracle's, fp64)"""
    P = params(7300 + 7 * B + V, B)
    x, jac = VO.verts_jac(host_model(V), T_(P).double())
    return frozen([P]) + frozen([x.numpy(), jac.numpy()])


@functools.lru_cache(maxsize=None)
def edge_case():
    """_fit_cases.edge_batch's parameters on its hands_mean = 0 model: zero, 1e-20, the series / closed-form switch,
    theta = pi, betas = +-3"""
    P = edge_batch()[0]
    x, jac = VO.verts_jac(host_model("edge"), T_(P).double())
    return frozen([P]) + frozen([x.numpy(), jac.numpy()])


@functools.lru_cache(maxsize=None)
def seeded(V):
    """_fit_oracle.seeded_case's NB hands: the true P [NB,62] (fp64, exact in fp32), their 21 joints in JOINT_MAP's order and
    their meshes, both rounded to fp32"""
    m = host_model(V)
    P, Tj = FO.seeded_case(3, NB, m, JOINT_MAP)
    with torch.no_grad():
        Tv = VO.model_verts(m, P).float()
    return P, Tj, Tv


@functools.lru_cache(maxsize=None)
def recovery_case(V):
    """the oracle's start over the vertices and its 20 iterations from there -> P, Tv, P0, Pf, the final vertex RMS [NB] and
    the costs after every iteration [20,NB]"""
    m = host_model(V)
    P, _, Tv = seeded(V)
    w = torch.ones(NB, V, dtype=torch.float64)
    P0 = VO.procrustes_start(m, Tv, w)
    Pf, c, acc, hist = VO.lm(m, Tv.double(), w, P0, 20, history=True)
    return P, Tv, P0, Pf, VO.rms(m, Pf, Tv).numpy(), hist.numpy()


@functools.lru_cache(maxsize=None)
def joints_case(V):
    """the same hands fitted to their 21 joints by the joints oracle (20 iterations from its Procrustes start) -> the joint
    targets, Pf, and the vertex RMS [NB] that Pf leaves: the twist and shape that joints do not decide"""
    m = host_model(V)
    P, Tj, Tv = seeded(V)
    w = torch.ones(NB, 21, dtype=torch.float64)
    Pf, _, _ = FO.lm(m, Tj.double(), w, JOINT_MAP, FO.procrustes_start(m, Tj, w, JOINT_MAP), 20)
    return Tj, Pf, VO.rms(m, Pf, Tv).numpy()


@functools.lru_cache(maxsize=None)
def step_case(V):
    """a start 0.05 off the truth in every model unknown, and the oracle's one step from there with lambda = 1e-2"""
    m = host_model(V)
    P, _, Tv = seeded(V)
    P1 = P.clone()
    P1[:, :58] += 0.05 * T_(synth.normal_like(11, "fit.off", (NB, 58), 1.0)).double()
    P1 = P1.float().double()
    Ps, c, acc = VO.lm(m, Tv.double(), torch.ones(NB, V, dtype=torch.float64), P1, 1, lambda0=1e-2)
    assert bool((acc == 1).all())
    return Tv, P1, Ps, c


@functools.lru_cache(maxsize=None)
def layer_case(V=778):
    """the seeded hands as the layer poses them (no translation, scale 1): P, the mesh rounded to fp32, and the oracle's fit of
    it, as in recovery_case"""
    m = host_model(V)
    P = seeded(V)[0].clone()
    P[:, 58:] = 0.0
    with torch.no_grad():
        Tv = VO.verts(m, P).float()
    w = torch.ones(NB, V, dtype=torch.float64)
    P0 = VO.procrustes_start(m, Tv, w)
    Pf, c, acc, hist = VO.lm(m, Tv.double(), w, P0, 20, history=True)
    return P, Tv, P0, Pf, VO.rms(m, Pf, Tv).numpy(), hist.numpy()
