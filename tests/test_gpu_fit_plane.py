"""The MANO fit to a surface point cloud on a real MI355X (include/scat_mano_fit_plane.h, scat_amd/fit.py) against the fp64
oracle of tests/_fit_plane_oracle.py and inside guard bands.  Inputs and models come from scat_amd.synth and
tests/golden/hand_mesh.npz.

The normals are IEEE fp64 on fp32 numbers on both sides, rounded to fp32 once: held to 2^-23 (one rounding of a number in
[-1, 1] is 2^-24, doubled for slack), the zero normals exactly.  The assignment keeps the bits of scat_mano_cloud_assign;
its metric data cost is held to the order of one fp64 sum (1e-12).  Every gate that compares fp32 with fp64 is 4 x the error
of the oracle itself run in fp32 on the CPU against its fp64 run on the same inputs (E32 below, printed by
tools/fit_plane_gates.py), normalised max |a - b| / max |b|: the project's rule for the MANO gates."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_plane_oracle as LO  # noqa: E402
import _fit_points_oracle as PO  # noqa: E402
import _fit_verts_oracle as VO  # noqa: E402
from _fit_plane_cases import (FIT_V, ITERS, JOINT_MAP, NB, QB, ROUNDS, SHAPES, TAU, TAUS, T_, ZERO_37, assign_case, host_model,  # noqa: E402
                              layer_plane_case, metric_case, metric_runs, quality_case, quality_inputs, smooth_model, topology,
                              vertex_rms)
from _fit_points_cases import TRIM, cloud, start  # noqa: E402
from _guard import Arena  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
# The oracle in fp32 on the CPU against itself in fp64, max |a - b| / max |b|, as tools/fit_plane_gates.py printed them.
#   step   the accepted p after one metric LM step from metric_case(V) (lambda 1e-2), per tau
#   cost   the oracle's metric cost function at its own iterate after 20 iterations of metric_case(V), per tau
E32 = {
    ("step", 37, 0.0): 4.565e-06, ("cost", 37, 0.0): 7.165e-07, ("step", 37, 0.01): 1.595e-06, ("cost", 37, 0.01): 1.102e-07,
    ("step", 37, 1.0): 6.890e-07, ("cost", 37, 1.0): 9.532e-08,
    ("step", 778, 0.0): 7.277e-07, ("cost", 778, 0.0): 1.087e-07, ("step", 778, 0.01): 2.520e-07, ("cost", 778, 0.01): 7.510e-08,
    ("step", 778, 1.0): 2.893e-07, ("cost", 778, 1.0): 1.031e-07,
}
GATE = {k: 4.0 * v for k, v in E32.items()}


def on_device(m):
    return m if m.device is not None else m.to(DEV)


def model(V):
    return on_device(host_model(V))


@pytest.fixture(scope="module", autouse=True)
def device():
    from scat_amd._lib import lib

    lib().scat_check_device()


def fitter(m, **kw):
    from scat_amd.fit import ManoFitter

    return ManoFitter(on_device(m), joint_map=JOINT_MAP, **kw)


def dev(a):
    return None if a is None else (a if isinstance(a, torch.Tensor) else T_(a)).to(DEV)


def topo_d(V):
    from scat_amd.fit import Topology

    return Topology(*(dev(a) for a in topology(V)))


def bits(t):
    return t.cpu().numpy().tobytes()


def same_bits(a, b):
    return all(bits(x) == bits(y) for x, y in zip(a, b))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_assign_plane_normals_and_metric_cost(shape, weighted):
    """the normals against the fp64 oracle on the kernel's own model points; scat_mesh_normals on those points gives their
    bits; every output that scat_mano_cloud_assign has keeps its bits; idx exact and stats[3] to 1e-12 against the oracle"""
    from scat_amd.fit import mano_cloud_assign, mano_cloud_assign_plane, mesh_normals

    B, N, V, F = shape
    P, points, weights = assign_case(B, N, V, weighted)
    faces = topology(V)
    assert faces[0].shape == (F, 3)
    m, t = model(V), topo_d(V)
    c, nrm, mp = mano_cloud_assign_plane(m, dev(P), dev(points), dev(weights), t, 0.01, TAU, want_model_pts=True)
    ref, mp_ref = mano_cloud_assign(m, dev(P), dev(points), dev(weights), 0.01, want_model_pts=True)
    assert bits(mp) == bits(mp_ref) and same_bits(c[:6], ref[:6])
    assert nrm.shape == (B, V, 3) and nrm.dtype == torch.float32 and bits(mesh_normals(mp, t)) == bits(nrm)
    x, got = mp.cpu().numpy(), nrm.cpu().numpy()
    want = LO.normals(x, *faces)
    e = float(np.abs(got - want).max())
    print(f"{shape} weighted {weighted}: normals {e:.3e} (gate 2^-23 = {2.0 ** -23:.3e}), {int((want == 0).all(2).sum())} zero")
    assert np.isfinite(got).all() and e <= 2.0 ** -23
    zero = (want == 0).all(2)
    assert (got[zero] == 0).all() and (got[~zero] != 0).any(1).all()
    if V == 37:
        assert zero[:, sorted(v for vs in ZERO_37.values() for v in vs)].all() and zero.sum() == 4 * B
    a = PO.assign(x, points, weights, 0.01)
    assert (c.idx.cpu().numpy() == a["idx"]).all() and (c.matched.cpu().numpy() == a["stats"][:, 2]).all()
    # the header's expression on the numbers the kernel has: its model points, its normals, and tau as the fp32 it is passed as
    dc, dw = c.data_cost.cpu().numpy(), LO.assign_cost(x, points, weights, a["idx"], a["matched"], got, float(np.float32(TAU)))
    print(f"{shape} weighted {weighted}: metric data cost {dc[:3]}, the oracle's {dw[:3]}, the Euclidean {ref.data_cost.cpu().numpy()[:3]}")
    assert np.isfinite(dc).all() and (np.abs(dc - dw) <= 1e-12 * dw).all()
    assert (dc <= ref.data_cost.cpu().numpy() * (1 + 1e-12)).all()      # rho <= |r|^2 for a unit or zero normal
    if weighted:
        assert bool((c.idx[:, ::5] == -1).all())
    # tau = 1 is the Euclidean cost, to the order of the sum
    c1 = mano_cloud_assign_plane(m, dev(P), dev(points), dev(weights), t, 0.01, 1.0)[0]
    e1, r1 = c1.data_cost.cpu().numpy(), ref.data_cost.cpu().numpy()
    assert (np.abs(e1 - r1) <= 1e-12 * r1).all()


def run_metric(V, tau, iters, lambda0):
    from scat_amd.fit import mano_fit_verts_metric

    Tv, w, n, P1 = metric_case(V)
    p = P1.float().to(DEV)
    cost, acc = mano_fit_verts_metric(model(V), Tv.to(DEV), w.to(DEV), n.to(DEV), p, iters, tau, lambda0, 1e-6, 1e-6)
    return p, cost, acc


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("V", FIT_V)
def test_metric_solve_matches_the_oracle(V, tau):
    """one step (lambda0 = 1e-2) against the oracle's step, and the cost after 20 iterations against the oracle's cost
    function at the returned p, both given the oracle's normals; at tau = 1 the step is fit_vertices' on the same data"""
    Tv, w, n, P1 = metric_case(V)
    Ps, _, hist = metric_runs(V, tau)
    p, cost1, acc = run_metric(V, tau, 1, 1e-2)
    assert acc.tolist() == [1] * NB
    e = VO.rel(p.cpu().numpy(), Ps.numpy())
    print(f"V {V} tau {tau}: one step {e:.3e} (gate {GATE[('step', V, tau)]:.3e} = 4 x {E32[('step', V, tau)]:.3e})")
    assert e <= GATE[("step", V, tau)]
    if tau == 1.0:
        r = fitter(host_model(V), lambda0=1e-2).fit_vertices(Tv.to(DEV), w.to(DEV), init=P1.float().to(DEV), iters=1)
        e = VO.rel(p.cpu().numpy(), r.p.cpu().numpy())
        print(f"V {V} tau 1: against fit_vertices {e:.3e}, the same bits: {bits(p) == bits(r.p)}")
        assert e <= GATE[("step", V, tau)] and r.accepted.tolist() == [1] * NB
    p20, cost20, acc20 = run_metric(V, tau, 20, 1e-3)
    with torch.no_grad():
        want = LO.cost(host_model(V), p20.cpu().double(), Tv.double(), w.double(), n.double(), tau, 1e-6, 1e-6)
    e = VO.rel(cost20.cpu().double().numpy(), want.numpy())
    print(f"V {V} tau {tau}: cost after 20 {cost20.cpu().numpy()} (the oracle's own run {hist[-1]}), against the oracle's at p "
          f"{e:.3e} (gate {GATE[('cost', V, tau)]:.3e} = 4 x {E32[('cost', V, tau)]:.3e}), accepted {acc20.tolist()}")
    assert e <= GATE[("cost", V, tau)]
    assert bool((cost20 < cost1).all()) and bool((acc20 >= 1).all()) and bool((acc20 <= 20).all())


@pytest.mark.parametrize("V", FIT_V)
def test_fit_points_plane_is_assign_plane_and_metric_fit_composed(V):
    from scat_amd.fit import mano_cloud_assign_plane, mano_fit_verts_metric

    f, m, t, faces = fitter(host_model(V)), model(V), topo_d(V), topology(V)[0]
    pts, p0, k = dev(cloud(V, "shuffled")), start(V).to(DEV), 3
    p, accs = p0.clone(), []
    for _ in range(2):
        c, n = mano_cloud_assign_plane(m, p, pts, None, t, TRIM, TAU)
        accs.append(mano_fit_verts_metric(m, c.vertex_target, c.vertex_weight, n, p, k, TAU, f.lambda0, f.w_pose, f.w_beta)[1])
        if len(accs) == 1:
            one = f.fit_points_plane(pts, p0, faces, rounds=1, iters=k, max_dist=TRIM)
            assert bits(one.p) == bits(p) and torch.equal(one.accepted, accs[0]) and bool((accs[0] > 0).all())
    two = f.fit_points_plane(pts, p0, faces, rounds=2, iters=k, max_dist=TRIM)
    assert bits(two.p) == bits(p) and torch.equal(two.accepted, accs[0] + accs[1])
    # the result describes the returned p, in the plane metric
    c = mano_cloud_assign_plane(m, two.p, pts, None, t, TRIM, TAU)[0]
    assert bits(two.idx) == bits(c.idx) and bits(two.dist) == bits(c.dist) and torch.equal(two.matched, c.matched)
    assert bits(two.data_cost) == bits(c.data_cost.float()) and bits(two.rms) == bits((c.data_cost / c.matched_weight).sqrt().float())
    assert bits(p0) == bits(start(V))      # the start is not modified
    # no state but p passes between rounds: a rounds, then b - a from its result, are b rounds
    again = f.fit_points_plane(pts, one, faces, rounds=1, iters=k, max_dist=TRIM)
    assert same_bits(again[:6], two[:6]) and same_bits(again[7:], two[7:]) and torch.equal(again.accepted + one.accepted, two.accepted)


def test_recovers_hands_from_a_surface_cloud():
    """the smooth model on the hand surface, 2048 points on the faces of the true mesh, the start 1.7 - 10 mm off: per hand
    the vertex RMS against the true mesh <= 2 x the fp64 oracle's + 1e-5 m, the project's recovery gate, and below the
    device's own nearest-vertex fit_points at the same rounds x iterations"""
    from scat_amd.render import MeshRenderer

    r0, rn, want, _ = quality_case()
    _, mesh, pts, P0 = quality_inputs()
    f = fitter(smooth_model())
    ren = MeshRenderer(topology(778)[0], 778, device=DEV)
    r = f.fit_points_plane(dev(pts), P0.to(DEV), ren, rounds=ROUNDS, iters=ITERS)
    near = f.fit_points(dev(pts), P0.to(DEV), rounds=ROUNDS, iters=ITERS)
    got, gn = vertex_rms(r.p.cpu(), mesh), vertex_rms(near.p.cpu(), mesh)
    for b in range(QB):
        print(f"hand {b}: start {1e3 * r0[b]:.3f} mm, point-to-plane {1e3 * got[b]:.4f} mm (oracle {1e3 * want[b]:.4f} mm, gate "
              f"{1e3 * (2 * want[b] + 1e-5):.4f} mm), nearest vertex {1e3 * gn[b]:.4f} mm (oracle {1e3 * rn[b]:.4f} mm), accepted "
              f"{int(r.accepted[b])}, matched {int(r.matched[b])}, plane rms {1e3 * float(r.rms[b]):.4f} mm")
    assert torch.isfinite(r.p).all() and r.matched.tolist() == [pts.shape[1]] * QB
    assert (got <= 2 * want + 1e-5).all(), (got, want)
    assert (got < gn).all(), (got, gn)
    # the renderer and the plain array are the same topology; the result goes where any result goes
    again = f.fit_points_plane(dev(pts), P0.to(DEV), topology(778)[0], rounds=ROUNDS, iters=ITERS)
    assert same_bits(again, r)
    n = f.vertex_normals(r, ren)
    assert n.shape == (QB, 778, 3) and bits(n) == bits(f.vertex_normals(f.mesh(r), topology(778)[0]))
    assert float((n.double().pow(2).sum(2).sqrt() - 1).abs().max()) < 1e-6
    out = ren.render(f.mesh(r), torch.tensor([[4.0, 0.0, 0.0]] * QB, device=DEV), want=("mask",))
    assert bool(out["mask"].any())


def test_outliers_and_zero_weights_do_not_count():
    """the clean cloud under max_dist = 0.03, the same with a tenth more points interleaved 10 m away (trimmed every
    round), and with points of weight 0 at +-1e6 and 3e37 interleaved: the same bits in p, data_cost and accepted"""
    V = 37
    f, faces = fitter(host_model(V)), topology(V)[0]
    clean, p0 = cloud(V, "shuffled"), start(V).to(DEV)
    nb, N = clean.shape[:2]
    rows, far, zero, w = [], [], [], []
    for n in range(N):
        rows.append((clean[:, n], 1.0))
        if n % 10 == 3:
            rows.append((None, 0.0))
    fill = iter([1e6, -1e6, 3e37] * N)
    for q, wt in rows:
        far.append(q if q is not None else far[-1] + np.float32(10.0))
        zero.append(q if q is not None else np.full((nb, 3), next(fill), np.float32))
        w.append(wt)
    far, zero = np.stack(far, 1), np.stack(zero, 1)
    w = np.broadcast_to(np.array(w, np.float32), (nb, len(w))).copy()
    keep = torch.from_numpy(w[0] > 0)
    a = f.fit_points_plane(dev(clean), p0, faces, max_dist=TRIM)
    b = f.fit_points_plane(dev(far), p0, faces, max_dist=TRIM)
    c = f.fit_points_plane(dev(zero), p0, faces, weights=dev(w), max_dist=TRIM)
    assert bool((a.accepted > 0).all()) and int(a.matched.min()) > 0
    for other in (b, c):
        assert bits(other.p) == bits(a.p) and bits(other.data_cost) == bits(a.data_cost) and torch.equal(other.accepted, a.accepted)
        assert torch.equal(other.matched, a.matched) and bits(other.idx[:, keep]) == bits(a.idx) and bits(other.rms) == bits(a.rms)
    assert bool((c.idx[:, ~keep] == -1).all()) and bool((b.dist[:, ~keep] > 9.0).all())


def test_frozen_unknowns_keep_their_bits():
    from scat_amd.fit import free_mask

    V = 37
    f, faces = fitter(host_model(V)), topology(V)[0]
    pts, p0 = dev(cloud(V, "shuffled")), start(V).to(DEV)
    r = f.fit_points_plane(pts, p0, faces, free=free_mask(betas=False, log_scale=False))
    assert torch.equal(r.betas, p0[:, 48:58]) and torch.equal(r.p[:, 61], p0[:, 61])
    assert not torch.equal(r.poses, p0[:, 3:48]) and bool((r.accepted > 0).all())


def test_unusable_hands_are_not_fitted():
    """a point that is not finite, a weight that is negative or not finite, a start that is not finite: data_cost +inf,
    accepted 0, p the start bit for bit, zero normals; a normal that is not finite passed to the metric solve: cost +inf,
    accepted 0, p untouched; the hands beside them have the bits of a run without them"""
    from scat_amd.fit import mano_cloud_assign_plane, mano_fit_verts_metric

    V = 37
    f, faces = fitter(host_model(V)), topology(V)[0]
    pts, w, p0 = cloud(V, "shuffled").copy(), np.ones((6, V), np.float32), start(V).clone()
    pts[1, 7, 2], pts[3, 36, 0] = np.nan, np.inf
    w[4, 0], w[5, 20] = -1.0, np.nan
    p0[2, 50] = float("nan")
    good, bad = [0], [1, 2, 3, 4, 5]
    r = f.fit_points_plane(dev(pts), p0.to(DEV), faces, weights=dev(w), max_dist=TRIM)
    ref = f.fit_points_plane(dev(pts[good]), p0[good].to(DEV), faces, weights=dev(w[good]), max_dist=TRIM)
    for b in bad:
        assert float(r.data_cost[b]) == float("inf") and int(r.accepted[b]) == 0 and int(r.matched[b]) == 0
        assert bits(r.p[b]) == bits(p0[b]) and float(r.rms[b]) == float("inf")
        assert bool((r.idx[b] == -1).all()) and bool((r.dist[b] == 0).all())
    assert same_bits([x[good] for x in r], ref) and bool((ref.accepted > 0).all())
    c, n = mano_cloud_assign_plane(model(V), p0.to(DEV), dev(pts), dev(w), topo_d(V), TRIM, TAU)
    assert torch.isnan(c.vertex_weight[bad]).all() and bool((n[bad] == 0).all()) and bool((n[good] != 0).any())
    Tv, wv, nv, P1 = metric_case(V)
    nv = nv.clone()
    nv[1, 5, 2], nv[4, 36, 0] = float("nan"), float("inf")
    p = P1.float().to(DEV)
    cost, acc = mano_fit_verts_metric(model(V), Tv.to(DEV), wv.to(DEV), nv.to(DEV), p, 3, TAU, 1e-3, 1e-6, 1e-6)
    keep = [0, 2, 3, 5]
    pk = P1.float()[keep].to(DEV)
    ck, ak = mano_fit_verts_metric(model(V), Tv[keep].to(DEV), wv[keep].to(DEV), nv[keep].to(DEV), pk, 3, TAU, 1e-3, 1e-6, 1e-6)
    for b in (1, 4):
        assert float(cost[b]) == float("inf") and int(acc[b]) == 0 and bits(p[b]) == bits(P1.float()[b])
    assert bits(p[keep]) == bits(pk) and bits(cost[keep]) == bits(ck) and torch.equal(acc[keep], ak) and bool((ak > 0).all())


def test_same_call_same_bits():
    B, N, V, F = SHAPES[3]
    P, points, weights = assign_case(B, N, V, True)
    f, faces = fitter(host_model(V)), topology(V)[0]
    run = lambda: f.fit_points_plane(dev(points), dev(P), faces, weights=dev(weights), rounds=2, iters=2, max_dist=0.01)
    a, b = run(), run()
    assert same_bits(a, b) and int(a.matched.min()) > 0


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_entry_points_inside_guard_bands(fill):
    """every operand of the four launching entry points between poisoned bands at pointer skews 0, 1 and 3 floats (stats
    holds doubles and keeps to 8 bytes; the workspace, exactly the queried size, to 16): bands intact, every output
    element written, results bit for bit those of the plain run outside the arena; a workspace one byte short is refused"""
    from scat_amd._lib import ScatError, lib
    from scat_amd.fit import FIT_PLANE_HEADER, mano_cloud_assign_plane, mano_fit_verts_metric, mesh_normals

    L, V, N, B, F = lib(), 37, 37, 3, 70
    ns = L.bind(FIT_PLANE_HEADER)
    m, t = model(V), topo_d(V)
    pts, p0 = T_(cloud(V, "shuffled")[:B]), start(V)[:B].clone()
    w = torch.full((B, N), 0.75)
    w[:, 5] = 0.0
    Tv, wv, nv, P1 = (x[:B] for x in metric_case(V))
    with torch.no_grad():
        verts = VO.model_verts(host_model(V), p0.double()).float()
    stream = torch.cuda.current_stream().cuda_stream
    f = fitter(host_model(V))
    plain = [mesh_normals(verts.to(DEV), t)]
    pm = P1.float().to(DEV)
    cm, am = mano_fit_verts_metric(m, Tv.to(DEV), wv.to(DEV), nv.to(DEV), pm, 3, TAU, 1e-3, 1e-6, 1e-6)
    plain += [pm, cm, am]
    c, n, mp = mano_cloud_assign_plane(m, p0.to(DEV), pts.to(DEV), w.to(DEV), t, TRIM, TAU, want_model_pts=True)
    plain += [mp, n, c.idx, c.dist, c.vertex_weight, c.vertex_target]
    stats = torch.stack([torch.zeros(B, dtype=torch.float64, device=DEV), c.matched_weight, c.matched.double(), c.data_cost], 1)
    r = f.fit_points_plane(pts.to(DEV), p0.to(DEV), topology(V)[0], weights=w.to(DEV), rounds=2, iters=3, max_dist=TRIM)
    plain += [r.p, r.data_cost, r.accepted, r.idx, r.dist]
    assert bool((r.accepted > 0).all()) and int(r.matched.min()) > 0 and bool((am > 0).all())
    nbytes = int(ns.scat_mano_fit_points_plane_ws(B, N, V, F))
    arena = Arena(DEV, fill, nbytes=16 << 20)
    for skew in (0, 1, 3):
        arena.reset()
        mod = [arena.place(x.cpu(), skew, name=nm) for nm, x in (("blend", m.blend), ("joint_t", m.joint_t), ("joint_s", m.joint_s),
                                                                ("weights_t", m.weights_t), ("hands_mean", m.hands_mean_d))]
        mpt = [x.data_ptr() for x in mod]
        tp = [arena.place(x.cpu(), skew, name=nm).data_ptr() for nm, x in zip(("faces", "vf_off", "vf_idx"), t)]
        vd, qd, wd = arena.place(verts, skew, name="verts"), arena.place(pts, skew, name="points"), arena.place(w, skew, name="w")
        outs = [arena.place((B, V, 3), skew, name="n.normals", out=True)]
        ns.scat_mesh_normals(vd.data_ptr(), *tp, outs[0].data_ptr(), B, V, F, stream)
        assert L.scat_last_kernel() == b"mesh_normals_v37_f70"
        td, wvd, nd = arena.place(Tv, skew, name="targets"), arena.place(wv, skew, name="vweights"), arena.place(nv, skew, name="normals")
        p = arena.place(P1.float(), skew, name="m.p", out=True)
        cost = arena.place((B,), skew, name="m.cost", out=True)
        acc = arena.place((B,), skew, dtype=torch.int32, name="m.accepted", out=True)
        ns.scat_mano_fit_verts_metric(*mpt, td.data_ptr(), wvd.data_ptr(), nd.data_ptr(), p.data_ptr(), cost.data_ptr(), acc.data_ptr(),
                                      B, V, m.parents_packed, 3, TAU, 1e-3, 1e-6, 1e-6, (1 << 62) - 1, stream)
        assert L.scat_last_kernel() == b"mano_fit_verts_metric_v37_i3"
        outs += [p, cost, acc]
        pd = arena.place(p0, skew, name="p")
        o = [arena.place((B, V, 3), skew, name="a.model_pts", out=True), arena.place((B, V, 3), skew, name="a.normals", out=True),
             arena.place((B, N), skew, dtype=torch.int32, name="a.idx", out=True), arena.place((B, N), skew, name="a.dist", out=True),
             arena.place((B, V), skew, name="a.vw", out=True), arena.place((B, V, 3), skew, name="a.vtarget", out=True)]
        st = arena.place((B, 4), skew & 2, dtype=torch.float64, name="a.stats", out=True)
        ns.scat_mano_cloud_assign_plane(*mpt, pd.data_ptr(), qd.data_ptr(), wd.data_ptr(), *tp, TRIM, TAU, *(x.data_ptr() for x in o),
                                        st.data_ptr(), B, N, V, F, m.parents_packed, stream)
        assert L.scat_last_kernel() == b"mano_cloud_assign_plane_v37_n37_f70"
        outs += o
        p = arena.place(p0, skew, name="p.fit", out=True)
        cost = arena.place((B,), skew, name="data_cost", out=True)
        acc = arena.place((B,), skew, dtype=torch.int32, name="accepted", out=True)
        idx = arena.place((B, N), skew, dtype=torch.int32, name="c.idx", out=True)
        dist = arena.place((B, N), skew, name="c.dist", out=True)
        ws = arena.place((nbytes,), 0, dtype=torch.uint8, name="ws", out=True, finite=False)
        fit_args = lambda nb: (*mpt, qd.data_ptr(), wd.data_ptr(), *tp, p.data_ptr(), cost.data_ptr(), acc.data_ptr(), idx.data_ptr(),
                               dist.data_ptr(), ws.data_ptr(), nb, B, N, V, F, m.parents_packed, 2, 3, TRIM, TAU, 1e-3, 1e-6, 1e-6,
                               (1 << 62) - 1, stream)
        with pytest.raises(ScatError, match=rf"workspace of {nbytes - 1} bytes, {nbytes} needed"):
            ns.scat_mano_fit_points_plane(*fit_args(nbytes - 1))
        ns.scat_mano_fit_points_plane(*fit_args(nbytes))
        assert L.scat_last_kernel() == b"mano_fit_points_plane_v37_n37_r2_i3"
        outs += [p, cost, acc, idx, dist]
        torch.cuda.synchronize()
        arena.check()
        for got, want in zip(outs, plain):
            assert bits(got) == bits(want), skew
        assert bits(st) == bits(stats), skew


def test_layer_to_joints_fit_to_plane_fit_to_evaluator():
    """ManoLayer's [B,21+V,3] -> its 21 joints -> fit -> fit_points_plane on a cloud drawn on the faces of the true mesh ->
    mesh -> MeshEvaluator: on every hand the mean vertex error is below the joints fit's and within the recovery gate (a
    mean of distances is at most their RMS)"""
    from scat_amd.mano import ManoLayer
    from scat_amd.mesh_evaluator import MeshEvaluator

    V = 778
    m = on_device(smooth_model())
    P, pts, _, left0, want = layer_plane_case()
    Pd = P.float().to(DEV)
    with torch.no_grad():
        out = ManoLayer(m)(Pd[:, :3].contiguous(), Pd[:, 3:48].contiguous(), Pd[:, 48:58].contiguous())
    f = fitter(smooth_model())
    rj = f.fit(out[:, :21][:, list(JOINT_MAP)].contiguous())
    r = f.fit_points_plane(dev(pts), rj, topology(V)[0], rounds=ROUNDS, iters=ITERS)
    assert r.rots.shape == (QB, 3) and r.poses.shape == (QB, 45) and r.betas.shape == (QB, 10) and r.trans.shape == (QB, 3)
    assert r.scale.shape == (QB,) and r.data_cost.shape == (QB,) and r.accepted.dtype == torch.int32 and r.p.shape == (QB, 62)
    assert r.matched.tolist() == [pts.shape[1]] * QB and r.idx.shape == (QB, pts.shape[1]) and r.rms.shape == (QB,)
    verts, joints = f.mesh(r), f.joints(r)
    assert verts.shape == (QB, V, 3) and verts.is_cuda and joints.shape == (QB, 21, 3)
    again = f.fit_vertices(out[:, 21:].contiguous(), init=r, iters=1)      # any entry point starts from it like from a FitResult
    assert again.p.shape == (QB, 62) and f.fit_points(dev(pts), r, rounds=1).p.shape == (QB, 62)
    ev = MeshEvaluator()
    ev.update(verts, out[:, 21:].contiguous())
    res = ev.result()
    gate_mm = 1e3 * (2 * want + 1e-5)
    per_hand = 1e3 * (verts - out[:, 21:]).double().pow(2).sum(2).sqrt().mean(1).cpu().numpy()
    left = 1e3 * (f.mesh(rj) - out[:, 21:]).double().pow(2).sum(2).sqrt().mean(1).cpu().numpy()
    print(f"MPVPE {res['mpvpe_mm']:.5f} mm; per hand {per_hand} mm, gates {gate_mm} mm, the joints fit alone {left} mm (the "
          f"oracle's joints fit: RMS {1e3 * left0} mm)")
    assert res["frames_kept"] == QB
    assert (per_hand <= gate_mm).all() and (left > per_hand).all()
