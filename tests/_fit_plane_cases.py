"""The fixed inputs of the tests of the MANO fit to a surface point cloud and what the fp64 oracle
(tests/_fit_plane_oracle.py) makes of them, computed once per process and read-only: shared by tests/test_fit_plane.py (no
GPU), tests/test_gpu_fit_plane.py and tools/fit_plane_gates.py.  Needs no GPU.

Two kinds of model.  Parity runs on host_model(V) of _fit_cases.py with ANY faces: they define normals, and parity needs no
surface.  The quality gate runs on smooth_model(), built on tests/golden/hand_mesh.npz so that posed meshes stay surfaces
and a cloud drawn on the faces means what a depth camera's does."""
import functools
import os

import numpy as np
import torch

from scat_amd import synth
from scat_amd.render import vertex_face_csr

import _fit_plane_oracle as LO
import _fit_points_oracle as PO
import _fit_verts_oracle as VO
from _fit_cases import params
from _fit_verts_cases import JOINT_MAP, NB, T_, frozen, host_model, seeded, step_case  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
# (B, N, V, F): the smallest; sub-wavefront and odd; one point past the workgroup; more workgroups than one wave of them per
# XCD, the hand mesh; all maxima (SCAT_FIT_POINTS_MAX_N, SCAT_MANO_MAX_V, SCAT_RENDER_MAX_F), where the static LDS is largest
SHAPES = ((1, 1, 1, 1), (3, 37, 37, 70), (3, 257, 37, 70), (65, 300, 778, 1538), (1, 8192, 1536, 4096))
TAUS = (0.0, 0.01, 1.0)
FIT_V = (37, 778)
ROUNDS, ITERS = 10, 4            # the quality runs
QB, QN = 4, 2048                 # hands and points of the quality case
TAU = 0.01                       # ManoFitter.fit_points_plane's default
MARGIN = 1e-12                   # relative best / second-best d2 margin that every surface point must have in the oracle
# vertices of topology(37) whose normal is zero, by route: in no face; only in a degenerate face (a repeated vertex); only
# in a pair of coincident faces of opposite winding, whose cross products cancel exactly
ZERO_37 = {"no face": (36,), "degenerate": (35,), "cancelling": (33, 34)}


@functools.lru_cache(maxsize=None)
def topology(V):
    """-> faces [F,3], vf_off [V+1], vf_idx [3F] int32.  V = 1: one face (0, 0, 0).  V = 37: 67 seeded faces on the vertices
    0..32 and the three of ZERO_37.  V = 778: the 1538 faces of hand_mesh.npz.  V = 1536: 4096 seeded faces"""
    rng = np.random.default_rng(5100 + V)
    tri = lambda n, hi: np.stack([rng.permutation(hi)[:3] for _ in range(n)])
    if V == 1:
        f = np.zeros((1, 3), np.int64)
    elif V == 37:
        f = np.concatenate([tri(67, 33), [[35, 35, 5], [34, 33, 7], [34, 7, 33]]])
        assert sorted(set(f.reshape(-1))) == list(range(36))
    elif V == 778:
        f = np.load(os.path.join(HERE, "golden", "hand_mesh.npz"))["f"].astype(np.int64)
    else:
        f = tri(4096, V)
    off, idx = vertex_face_csr(f, V)
    return frozen([f.astype(np.int32), off, idx])


@functools.lru_cache(maxsize=None)
def assign_case(B, N, V, weighted):
    """P [B,62] fp32 (rots, poses, betas of _fit_cases.params, trans ~ N(0, 0.05), log_scale ~ N(0, 0.2)) and a cloud 3 mm
    off randomly chosen model points of the fp64 oracle, weights in (0.5, 1.5) with every fifth point's zero -> P, points,
    weights (or None).  What the oracle makes of them is computed in the test, on the model points the kernel wrote"""
    seed = 9500 + 7 * B + V + N
    P = np.concatenate([params(seed, B), synth.normal_like(seed, "trans", (B, 3), 0.05),
                        synth.normal_like(seed, "log_scale", (B, 1), 0.2)], axis=1).astype(np.float32)
    with torch.no_grad():
        x = VO.model_verts(host_model(V), T_(P).double()).numpy()
    pick = np.random.default_rng(seed).integers(0, V, size=(B, N))
    points = (np.take_along_axis(x, pick[:, :, None], 1) + synth.normal_like(seed, "cloud.noise", (B, N, 3), 0.003)).astype(np.float32)
    weights = None
    if weighted:
        weights = (1.0 + 0.5 * np.tanh(synth.normal_like(seed, "cloud.w", (B, N), 1.0))).astype(np.float32)
        weights[:, ::5] = 0.0
    return frozen([P, points]) + (None if weights is None else frozen([weights])[0],)


@functools.lru_cache(maxsize=None)
def metric_case(V):
    """the NB seeded hands of _fit_verts_cases with their meshes as targets, per-vertex weights in (0.5, 1.5) with every
    fifth zero, the oracle's normals of the targets for topology(V) rounded to fp32 (what the kernel is given too), and
    step_case's start 0.05 off the truth -> Tv [NB,V,3] fp32, w [NB,V] fp32, n [NB,V,3] fp32, P1 [NB,62] fp64 (exact in fp32)"""
    Tv, P1 = step_case(V)[:2]
    w = (1.0 + 0.5 * np.tanh(synth.normal_like(9600 + V, "metric.w", (NB, V), 1.0))).astype(np.float32)
    w[:, ::5] = 0.0
    n = LO.normals(Tv.numpy(), *topology(V)).astype(np.float32)
    return Tv, T_(w), T_(n), P1


@functools.lru_cache(maxsize=None)
def metric_runs(V, tau):
    """the oracle on metric_case(V): one step with lambda0 = 1e-2 -> Ps, and 20 iterations -> P20 with the cost after every
    iteration [20,NB]"""
    Tv, w, n, P1 = metric_case(V)
    m = host_model(V)
    Ps, _, acc = LO.lm(m, Tv.double(), w.double(), n.double(), tau, P1, 1, lambda0=1e-2)
    assert bool((acc == 1).all())
    P20, c20, _, hist = LO.lm(m, Tv.double(), w.double(), n.double(), tau, P1, 20, history=True)
    return Ps, P20, hist.numpy()


@functools.lru_cache(maxsize=None)
def smooth_model():
    """A model on the hand surface of hand_mesh.npz: v_template its vertices; 16 joints, each the mean of the 8 vertices
    nearest to one of 16 farthest-point-sampled vertices (the J_regressor rows); dense skinning weights
    softmax(-|v - J_j|^2 / 2 sigma^2), sigma = 0.15 x the largest extent; shapedirs[:, :, k] = 0.05 (v - mean) A_k^T and
    posedirs[:, :, k] = 0.01 (v - mean) A_k^T with seeded 3 x 3 A_k ~ N(0, 1); hands_mean = 0, MANO's parents"""
    from scat_amd.mano import ManoModel

    v = np.load(os.path.join(HERE, "golden", "hand_mesh.npz"))["v"].astype(np.float64)
    V = v.shape[0]
    far = [int(np.argmax(((v - v.mean(0)) ** 2).sum(1)))]
    d = ((v - v[far[0]]) ** 2).sum(1)
    while len(far) < 16:
        far.append(int(np.argmax(d)))
        d = np.minimum(d, ((v - v[far[-1]]) ** 2).sum(1))
    Jr = np.zeros((16, V))
    for j, s in enumerate(far):
        Jr[j, np.argsort(((v - v[s]) ** 2).sum(1), kind="stable")[:8]] = 0.125
    J = Jr @ v
    sigma = 0.15 * float((v.max(0) - v.min(0)).max())
    e = -((v[:, None, :] - J[None, :, :]) ** 2).sum(2) / (2.0 * sigma * sigma)
    W = np.exp(e - e.max(1, keepdims=True))
    W /= W.sum(1, keepdims=True)
    c = v - v.mean(0)
    A = synth.normal_like(5200, "smooth.A", (10 + 135, 3, 3), 1.0).astype(np.float64)
    sd = np.stack([0.05 * c @ A[k].T for k in range(10)], 2)
    pd = np.stack([0.01 * c @ A[10 + k].T for k in range(135)], 2)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return ManoModel.from_arrays(dict(v_template=f32(v), shapedirs=f32(sd), posedirs=f32(pd), J_regressor=f32(Jr), weights=f32(W),
                                      hands_mean=np.zeros(45, np.float32), tips=tuple(far[:5])))


def surface_cloud(mesh, faces, N, seed):
    """N points uniform in barycentric coordinates on uniformly chosen faces of mesh [B,V,3] fp64, rounded to fp32"""
    rng = np.random.default_rng(seed)
    B = mesh.shape[0]
    f = faces[rng.integers(0, len(faces), size=(B, N))]                 # [B,N,3]
    u = rng.random((B, N, 2))
    flip = u.sum(2) > 1.0
    u[flip] = 1.0 - u[flip]
    bary = np.concatenate([1.0 - u.sum(2, keepdims=True), u], 2)        # [B,N,3]
    corners = np.take_along_axis(mesh[:, :, None, :], f.reshape(B, 3 * N, 1, 1), 1).reshape(B, N, 3, 3)
    return (bary[..., None] * corners).sum(2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def quality_inputs(seed=5300):
    """QB hands of smooth_model(): rots ~ N(0, 0.8), poses ~ N(0, 0.25), betas ~ N(0, 1), trans ~ N(0, 0.05), log_scale ~
    N(0, 0.1) -> the true P [QB,62] (fp64, exact in fp32), the true mesh (fp64), a cloud of QN points on its faces (fp32),
    and a start the truth + 0.03 N(0, 1) in the 58 model unknowns and + 3 mm N(0, 1) in trans (fp32)"""
    m = smooth_model()
    P = np.concatenate([synth.normal_like(seed, n, (QB, k), s) for n, k, s in
                        (("rots", 3, 0.8), ("poses", 45, 0.25), ("betas", 10, 1.0), ("trans", 3, 0.05), ("log_scale", 1, 0.1))],
                       axis=1).astype(np.float32)
    Pt = T_(P).double()
    with torch.no_grad():
        mesh = VO.model_verts(m, Pt).numpy()
    pts = surface_cloud(mesh, topology(778)[0].astype(np.int64), QN, seed + 1)
    P0 = P.copy()
    P0[:, :58] += 0.03 * synth.normal_like(seed + 2, "start.model", (QB, 58), 1.0)
    P0[:, 58:61] += 0.003 * synth.normal_like(seed + 2, "start.trans", (QB, 3), 1.0)
    return Pt, T_(mesh), frozen([pts])[0], T_(P0.astype(np.float32))


@functools.lru_cache(maxsize=None)
def layer_plane_case():
    """quality_inputs' hands as the layer poses them (no translation, scale 1), as the pipeline sees them: a cloud of QN
    points on the faces of the fp64 mesh, and the oracle's point-to-plane ICP (ROUNDS x ITERS, TAU) from the oracle's
    joints fit of the layer's 21 joints -> P [QB,62], the cloud, the mesh (fp64), and the vertex RMS [QB] that the joints
    fit alone leaves and that the ICP ends at"""
    import _fit_oracle as FO
    import _mano_oracle as MO

    m = smooth_model()
    P = quality_inputs()[0].clone()
    P[:, 58:] = 0.0
    with torch.no_grad():
        out = MO.forward(m, P[:, :3], P[:, 3:48], P[:, 48:58])
    mesh, Tj = out[:, 21:], out[:, :21][:, list(JOINT_MAP)].float()
    w = torch.ones(QB, 21, dtype=torch.float64)
    P0 = FO.lm(m, Tj.double(), w, JOINT_MAP, FO.procrustes_start(m, Tj, w, JOINT_MAP), 20)[0].float()
    pts = surface_cloud(mesh.numpy(), topology(778)[0].astype(np.int64), QN, 5500)
    Pf = LO.icp(m, pts, None, P0, topology(778), ROUNDS, ITERS, TAU)[0]
    return P, frozen([pts])[0], mesh, vertex_rms(P0, mesh), vertex_rms(Pf, mesh)


def vertex_rms(P, mesh, model=None):
    """[B]: the root of the mean squared distance of the model's vertices at P from mesh, in the mesh's unit"""
    return VO.rms(smooth_model() if model is None else model, P, mesh).numpy()


@functools.lru_cache(maxsize=None)
def quality_case(tau=TAU, rounds=ROUNDS, iters=ITERS):
    """the oracle's point-to-plane ICP and its nearest-vertex ICP on quality_inputs, both rounds x iters from the same
    start -> the vertex RMS [QB] of the start, of nearest-vertex and of point-to-plane, and point-to-plane's P.  ASSERTS on
    the oracle alone that point-to-plane ends below nearest-vertex on every hand, and that every point of the cloud has a
    best / second-best margin above MARGIN at the start and at the end"""
    m, topo = smooth_model(), topology(778)
    _, mesh, pts, P0 = quality_inputs()
    Pn = PO.icp(m, pts, None, P0, rounds, iters)[0]
    Pp = LO.icp(m, pts, None, P0, topo, rounds, iters, tau)[0]
    r0, rn, rp = vertex_rms(P0, mesh), vertex_rms(Pn, mesh), vertex_rms(Pp, mesh)
    assert (rp < rn).all(), (rp, rn)
    for Pk in (P0.double(), Pp):
        with torch.no_grad():
            a = PO.assign(VO.model_verts(m, Pk).numpy(), pts, None, np.inf, margins=True)
        assert (a["margin"] > MARGIN).all(), float(a["margin"].min())
    return r0, rn, rp, Pp
