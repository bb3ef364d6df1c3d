"""The MANO fit to a track of meshes and of point clouds on a real MI355X (include/scat_mano_fit_seq_verts.h,
ManoFitter.fit_vertices_sequence and fit_points_sequence) against the fp64 oracle of tests/_fit_seq_verts_oracle.py and
inside guard bands.  V = 37 (one full tile of 32 vertices and a partial one of 5), S <= 3, T in {1, 2, 3, 5} (no neighbour,
ends only, one interior frame, several), N = 257 (no multiple of the four points the assignment reads at a time) unless
stated; V = 778, T = 3 once.

Every gate that compares fp32 with fp64 is 4 x the error of the oracle itself run in fp32 on the CPU against its fp64 run
on the same inputs (E32 below, printed by tools/fit_seq_verts_gates.py), normalised max |a - b| / max |b|: the rule of
tests/test_gpu_fit_seq.py.  None of the figures comes from the kernel."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_oracle as FO  # noqa: E402
import _fit_plane_cases as LC  # noqa: E402
import _fit_seq_verts_cases as G  # noqa: E402
import _fit_seq_verts_oracle as QO  # noqa: E402
from _fit_cases import JOINT_MAP, host_model  # noqa: E402
from _guard import Arena  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ALL = (1 << 62) - 1
# The oracle in fp32 on the CPU against itself in fp64, max |a - b| / max |b|, as tools/fit_seq_verts_gates.py printed them.
#   step      the accepted p after one LM step from step_case(V, 2, T, metric) (lambda 1e-2, SMOOTH), key (V, T, metric)
#   cost      the oracle's cost function at its own iterate after k iterations from start_case()'s start
#   start     the oracle's start from zero-pose vertices in fp32 against fp64, on start_case()
#   icp       the p after ICP_ROUNDS x ICP_ITERS of icp_case(2, 3, gap), solves in fp32 (both precisions accept the same
#             steps: the tool asserts it), key (plane, gap)
#   quality   acceleration error [QS] and vertex RMS per frame [QS,QT] of the track ICP on quality_inputs(), solves in fp32
E32 = {
    ("step", 37, 1, False): 5.421e-07, ("step", 37, 1, True): 3.405e-06, ("step", 37, 2, False): 4.609e-07,
    ("step", 37, 2, True): 1.115e-06, ("step", 37, 3, False): 5.106e-07, ("step", 37, 3, True): 1.511e-06,
    ("step", 37, 5, False): 6.957e-07, ("step", 37, 5, True): 1.590e-06, ("step", 778, 3, False): 6.622e-07,
    ("cost", 1): 2.803e-08, ("cost", 2): 5.696e-08, ("cost", 5): 1.668e-07, ("cost", 10): 1.668e-07,
    ("start",): 3.611e-08,
    ("icp", False, None): 2.034e-07, ("icp", True, None): 1.223e-06, ("icp", False, 1): 2.182e-07, ("icp", True, 1): 1.594e-06,
    ("quality", "accel"): 2.442e-06, ("quality", "rms"): 6.179e-05,
}
GATE = {k: 4.0 * v for k, v in E32.items()}
GATE_VERTS_STEP_37 = 4.0 * 8.849e-07      # tests/test_gpu_fit_verts.py's ("step", 37): ManoFitter.fit_vertices' own step gate


def model(V):
    m = host_model(V)
    return m if m.device is not None else m.to(DEV)


@pytest.fixture(scope="module", autouse=True)
def device():
    from scat_amd._lib import lib

    lib().scat_check_device()


def fitter(V, **kw):
    from scat_amd.fit import ManoFitter

    return ManoFitter(model(V), joint_map=JOINT_MAP, **kw)


def solve(V, X, w, n, P0, iters, smooth, lambda0=1e-3, free=ALL, tau=G.TAU):
    """scat_mano_fit_seq_verts through its plain wrapper (the normals have no place in fit_vertices_sequence) -> p, cost,
    accepted.  P0 None: init = 1"""
    from scat_amd.fit import mano_fit_seq_verts

    d = lambda t: None if t is None else t.float().contiguous().to(DEV)
    p = torch.empty(*X.shape[:2], 62, device=DEV) if P0 is None else d(P0).clone()
    cost, acc = mano_fit_seq_verts(model(V), d(X), d(w), d(n), p, iters, 1 if P0 is None else 0, tau, lambda0, 1e-6, 1e-6,
                                   G.sm(smooth), free)
    return p, cost, acc


def held(tag, key, got, want):
    e = FO.rel(got, want)
    print(f"{tag}: {e:.3e} (gate {GATE[key]:.3e} = 4 x {E32[key]:.3e})")
    assert np.isfinite(got).all(), (tag, key)
    assert e <= GATE[key], (tag, key, e, GATE[key])


def same_bits(a, b):
    return all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("V,T,metric", [(37, T, k) for T in (1, 2, 3, 5) for k in (False, True)] + [(778, 3, False)])
def test_one_step_matches_the_oracle(V, T, metric):
    X, w, n, P1, Ps, c = G.step_case(V, 2, T, metric)
    p, cost, acc = solve(V, X, w, n, P1, 1, G.SMOOTH, lambda0=1e-2)
    assert acc.tolist() == [1, 1] and p.shape == (2, T, 62)
    held(f"V {V} T {T} metric {metric}: one step", ("step", V, T, metric), p.cpu().numpy(), Ps.numpy())
    if not metric:      # the same through the public method
        r = fitter(V, lambda0=1e-2).fit_vertices_sequence(X.to(DEV), smooth=G.SMOOTH, init=P1.float().to(DEV), iters=1)
        assert same_bits((r.p, r.cost, r.accepted), (p, cost, acc)) and r.rots.shape == (2, T, 3) and r.scale.shape == (2, T)


def test_cost_is_monotone_and_is_the_oracles():
    m = model(37)
    P, X, P0 = G.start_case()
    f = fitter(37)
    costs = []
    for k in (1, 2, 5, 10):
        r = f.fit_vertices_sequence(X.to(DEV), smooth=G.SMOOTH, iters=k)
        assert bool((r.accepted <= k).all()) and bool((r.accepted >= 0).all())
        c = r.cost.cpu().double()
        costs.append(c)
        with torch.no_grad():
            want = QO.cost(m, r.p.cpu().double(), X.double(), G.ones(2, 5, 37), None, 1.0, f.w_pose, f.w_beta, G.sm(G.SMOOTH))
        held(f"iters {k}: cost {c.numpy()} against the oracle's at p", ("cost", k), c.numpy(), want.numpy())
    for a, b in zip(costs, costs[1:]):
        assert bool((b <= a).all())
    assert bool((costs[-1] < costs[0]).all())


def test_start_matches_the_oracle():
    """with every unknown frozen no step can be taken, and init = 1 returns the start itself and its cost"""
    P, X, P0 = G.start_case()
    f = fitter(37)
    r0 = f.fit_vertices_sequence(X.to(DEV), smooth=G.SMOOTH, free=0, iters=1)
    assert r0.accepted.tolist() == [0, 0] and bool(torch.isfinite(r0.cost).all())
    held("start", ("start",), r0.p.cpu().numpy(), P0.numpy())
    r = f.fit_vertices_sequence(X.to(DEV), smooth=G.SMOOTH, iters=5)
    assert bool((r.cost < r0.cost).all()) and bool((r.accepted > 0).all())


def test_single_frames_without_smoothness_agree_with_the_mesh_fit():
    """T = 1 and s_* = 0: the track kernels on one-frame sequences and ManoFitter.fit_vertices on the same frames, one step
    from the same start; they agree to the sum of the two kernels' step gates, and in fact bit for bit: with one frame and
    no smoothness the track kernel stages, damps, factors and back-substitutes the numbers that the frame kernel summed in the
    mesh kernel's order"""
    X, _, _, P1, _, _ = G.step_case(37, 2, 1, False)
    f = fitter(37, lambda0=1e-2)
    p0 = P1.float().to(DEV)
    a = f.fit_vertices_sequence(X.to(DEV), init=p0, iters=1)
    b = f.fit_vertices(X[:, 0].to(DEV), init=p0[:, 0], iters=1)
    assert a.accepted.tolist() == [1, 1] and b.accepted.tolist() == [1, 1]
    assert f.joints(a).shape == (2, 1, 21, 3) and f.mesh(a).shape == (2, 1, 37, 3)
    e, gate = FO.rel(a.p[:, 0].cpu().numpy(), b.p.cpu().numpy()), GATE[("step", 37, 1, False)] + GATE_VERTS_STEP_37
    print(f"T = 1 against the mesh fit: p {e:.3e} (gate {gate:.3e})")
    assert e <= gate
    assert same_bits((a.p[:, 0],), (b.p,))


def test_frozen_unknowns_keep_their_bits_in_every_frame():
    from scat_amd.fit import free_mask

    X, _, _, P1, _, _ = G.step_case(37, 2, 3, False)
    p0 = P1.float().to(DEV)
    r = fitter(37).fit_vertices_sequence(X.to(DEV), smooth=G.SMOOTH, init=p0, iters=8, free=free_mask(betas=False, log_scale=False))
    assert torch.equal(r.betas, p0[:, :, 48:58]) and torch.equal(r.p[:, :, 61], p0[:, :, 61])
    assert not torch.equal(r.poses, p0[:, :, 3:48]) and bool((r.accepted > 0).all())


def test_zero_weight_frames_are_bridged_and_legal():
    m = host_model(37)
    X, w, r0, rf = G.gap_case()
    f = fitter(37, iters=G.GAP_ITERS)
    res = []
    for fill in (1e6, -3.25):
        Xg = X.clone()
        Xg[0, G.GAP_AT] = fill
        res.append(f.fit_vertices_sequence(Xg.to(DEV), w.to(DEV), smooth=G.SMOOTH))
    assert same_bits(res[0], res[1])      # the frame's targets do not reach the result
    at = float(QO.rms(m, res[0].p.cpu(), X)[0, G.GAP_AT])
    print(f"bridged frame: {1e3 * at:.4f} mm from the truth, oracle {1e3 * rf:.4f} mm, start {1e3 * r0:.3f} mm")
    assert at <= 2 * rf + 1e-5 and bool((res[0].accepted > 0).all())
    # no data at all: legal, the priors and the smoothness alone; from the Procrustes start (zeros) nothing can improve
    z = f.fit_vertices_sequence(X.to(DEV), torch.zeros(1, G.GAP_T, 37, device=DEV), smooth=G.SMOOTH)
    assert float(z.cost[0]) == 0.0 and int(z.accepted[0]) == 0 and torch.equal(z.p, torch.zeros_like(z.p))
    p0 = G.off_start(G.track(33, 1, G.GAP_T, 37)[0], 23).float().to(DEV)
    z = f.fit_vertices_sequence(X.to(DEV), torch.zeros(1, G.GAP_T, 37, device=DEV), smooth=G.SMOOTH, init=p0)
    assert bool(torch.isfinite(z.p).all()) and int(z.accepted[0]) > 0 and 0.0 < float(z.cost[0]) < float("inf")


# the plane metric has no start of its own (init = 1 is refused with normals), so its case runs from the caller's start only
@pytest.mark.parametrize("what,with_init", [(w, i) for w in ("targets", "weights", "negative") for i in (False, True)]
                         + [("normals", True)])
def test_a_bad_sequence_is_not_fitted_and_leaves_the_others_alone(what, with_init):
    metric = what == "normals"
    X, w, n, P1, _, _ = G.step_case(37, 2, 3, metric)
    cat = lambda t: None if t is None else torch.cat([t, t[:1]], 0)
    X3, w3, n3, P3 = cat(X), cat(w), cat(n), cat(P1)
    if w3 is None:
        w3 = torch.ones(3, 3, 37)
    bad = {"targets": X3, "weights": w3, "normals": n3, "negative": w3}[what].clone()
    bad[1, 2, 7] = -1.0 if what == "negative" else float("nan")
    args = dict(targets=X3, weights=w3, normals=n3)
    init = P3 if with_init else None
    ref = solve(37, X3, w3, n3, init, 4, G.SMOOTH)
    args["weights" if what == "negative" else what] = bad
    p, cost, acc = solve(37, args["targets"], args["weights"], args["normals"], init, 4, G.SMOOTH)
    assert float(cost[1]) == float("inf") and int(acc[1]) == 0
    assert torch.equal(p[1], P3[1].float().to(DEV) if with_init else torch.zeros(3, 62, device=DEV))
    assert same_bits([t[[0, 2]] for t in (p, cost, acc)], [t[[0, 2]] for t in ref]) and bool((ref[2] > 0).all())


def test_a_start_that_is_not_finite_refuses_its_sequence():
    X, _, _, P1, _, _ = G.step_case(37, 2, 3, False)
    P = P1.float().clone()
    P[0, 1, 5] = float("inf")
    p, cost, acc = solve(37, X, None, None, P, 3, G.SMOOTH)
    ref = solve(37, X, None, None, P1, 3, G.SMOOTH)
    assert float(cost[0]) == float("inf") and int(acc[0]) == 0 and p[0].cpu().numpy().tobytes() == P[0].numpy().tobytes()
    assert same_bits([t[1:] for t in (p, cost, acc)], [t[1:] for t in ref])


def test_same_call_same_bits_no_dependence_on_S_and_a_rejected_step_keeps_p():
    P, X, P0 = G.start_case()
    X3 = torch.cat([X, X[:1] + 0.01], 0)
    f = fitter(37, iters=5)
    a, b = (f.fit_vertices_sequence(X3.to(DEV), smooth=G.SMOOTH) for _ in range(2))
    assert same_bits(a, b)
    for s in range(3):
        one = f.fit_vertices_sequence(X3[s:s + 1].to(DEV), smooth=G.SMOOTH)
        assert same_bits(one, [t[s:s + 1] for t in a]), s
    # hard_case: a full Gauss-Newton step from far away.  The oracle (fp32 and fp64, tools/fit_seq_verts_gates.py) accepts
    # the first step of sequence 1 and rejects every later one, while sequence 0 accepts all
    Xh, Ph = G.hard_case()
    runs = [solve(37, Xh, None, None, Ph, k, G.SMOOTH, lambda0=G.HARD_LAMBDA0) for k in range(1, G.HARD_ITERS + 1)]
    accs = [r[2].tolist() for r in runs]
    print(f"hard_case: accepted after 1..{G.HARD_ITERS} iterations {accs}")
    rejected = [(k, s) for k in range(1, G.HARD_ITERS) for s in range(2) if accs[k][s] == accs[k - 1][s] and accs[k][s] > 0]
    assert rejected, accs      # a rejected step after an accepted one is reached
    for k, s in rejected:      # its p and its cost are the accepted one's, bit for bit
        assert same_bits([runs[k][0][s], runs[k][1][s]], [runs[k - 1][0][s], runs[k - 1][1][s]]), (k, s)
    assert any(accs[k][s] > accs[k - 1][s] for k in range(1, G.HARD_ITERS) for s in range(2))      # and steps are taken after it


def test_without_an_accepted_step_p_is_untouched():
    P, X, P0 = G.start_case()
    p0 = P.float().to(DEV)
    keep = p0.clone()
    r = fitter(37).fit_vertices_sequence(X.to(DEV), smooth=G.SMOOTH, init=p0, free=0, iters=3)
    assert r.accepted.tolist() == [0, 0] and torch.equal(r.p, keep) and torch.equal(p0, keep)
    assert bool(torch.isfinite(r.cost).all())


def icp(f, pts, P0, topo, plane, **kw):
    return f.fit_points_sequence(torch.from_numpy(np.array(pts)).to(DEV), P0.to(DEV), faces=topo[0] if plane else None,
                                 smooth=G.ICP_SMOOTH, rounds=G.ICP_ROUNDS, iters=G.ICP_ITERS, max_dist=G.ICP_TRIM, w_tangent=G.TAU,
                                 **kw)


def last_assignment(f, r, pts, topo, plane):
    """the assignment launch on its own at r.p: idx, dist and the data cost (rounded to fp32 as the loop rounds it)"""
    from scat_amd.fit import mano_cloud_assign_plane

    S, T, N = pts.shape[:3]
    q = torch.from_numpy(np.array(pts)).reshape(S * T, N, 3).to(DEV)
    p = r.p.flatten(0, 1).contiguous()
    if plane:
        c = mano_cloud_assign_plane(f.model, p, q, None, f._topology("test", topo[0], q.device), G.ICP_TRIM, G.TAU)[0]
    else:
        c = f.nearest_vertices(p, q, None, G.ICP_TRIM)
    return c.idx.reshape(S, T, N), c.dist.reshape(S, T, N), c.data_cost.float().reshape(S, T), c.matched.reshape(S, T)


@pytest.mark.parametrize("plane", [False, True])
def test_icp_matches_the_oracle(plane):
    pts, P0, topo = G.icp_case(2, 3)
    Po, acc, dc, a, margin = G.icp_run(2, 3, plane)
    assert margin > G.ICP_MARGIN      # no assignment is near a tie or near the trim: fp32 flips none
    f = fitter(37)
    r = icp(f, pts, P0, topo, plane)
    assert r.p.shape == (2, 3, 62) and r.data_cost.shape == (2, 3) and r.idx.shape == (2, 3, G.ICP_N) and r.accepted.shape == (2,)
    held(f"ICP plane {plane}: p after {G.ICP_ROUNDS} x {G.ICP_ITERS}", ("icp", plane, None), r.p.cpu().numpy(), Po.numpy())
    assert r.accepted.tolist() == acc.tolist()
    assert np.array_equal(r.idx.cpu().numpy().reshape(6, -1), a["idx"]) and np.array_equal(r.matched.cpu().numpy().reshape(-1),
                                                                                          a["stats"][:, 2].astype(np.int64))
    idx, dist, cost, matched = last_assignment(f, r, pts, topo, plane)
    assert same_bits((r.idx, r.dist, r.data_cost, r.matched), (idx, dist, cost, matched))
    assert f.mesh(r).shape == (2, 3, 37, 3) and f.mesh(r).flatten(0, 1).shape == (6, 37, 3)
    assert same_bits(icp(f, pts, P0, topo, plane), r)


@pytest.mark.parametrize("plane", [False, True])
def test_fit_points_sequence_is_assign_and_track_solve_composed(plane):
    """one round at S 2, T 3, V 37, N 64 (the first 64 points of icp_case's frames): the loop is the assignment over the S T
    frames, scat_mano_fit_seq_verts on its targets, weights and normals, and the assignment again, bit for bit.  Every
    frame has matched weight: the public solve does not see the assignment's stats, so it would take a frame in which
    nothing matched, whose weights are a NaN row, for unusable where the loop bridges it"""
    from scat_amd.fit import mano_cloud_assign_plane, mano_fit_seq_verts

    S, T, V, N, k = 2, 3, 37, 64, 2
    pts, P0, topo = G.icp_case(S, T)
    pts = torch.from_numpy(np.ascontiguousarray(np.array(pts)[:, :, :N])).to(DEV)
    f, q = fitter(V), pts.reshape(S * T, N, 3)

    def assign(p):
        if not plane:
            return f.nearest_vertices(p, q, None, G.ICP_TRIM), None
        return mano_cloud_assign_plane(f.model, p, q, None, f._topology("test", topo[0], q.device), G.ICP_TRIM, G.TAU)

    p = P0.to(DEV).clone()
    c, n = assign(p.view(S * T, 62))
    assert bool((c.matched_weight > 0).all()) and bool(torch.isfinite(c.vertex_weight).all())      # the precondition
    cost, acc = mano_fit_seq_verts(f.model, c.vertex_target.view(S, T, V, 3), c.vertex_weight.view(S, T, V),
                                   None if n is None else n.view(S, T, V, 3), p, k, 0, G.TAU, f.lambda0, f.w_pose, f.w_beta,
                                   G.sm(G.ICP_SMOOTH))
    c = assign(p.view(S * T, 62))[0]
    r = f.fit_points_sequence(pts, P0.to(DEV), faces=topo[0] if plane else None, smooth=G.ICP_SMOOTH, rounds=1, iters=k,
                              max_dist=G.ICP_TRIM, w_tangent=G.TAU)
    assert bool((acc > 0).all()) and not torch.equal(p, P0.to(DEV))
    assert same_bits((r.p, r.accepted, r.idx, r.dist, r.data_cost),
                     (p, acc, c.idx.view(S, T, N), c.dist.view(S, T, N), c.data_cost.float().view(S, T)))


@pytest.mark.parametrize("plane", [False, True])
def test_icp_bridges_a_frame_where_nothing_matches(plane):
    pts, P0, topo = G.icp_case(2, 3, 1)
    Po, acc, dc, a, margin = G.icp_run(2, 3, plane, 1)
    assert margin > G.ICP_MARGIN
    f = fitter(37)
    r = icp(f, pts, P0, topo, plane)
    assert r.matched[0].tolist()[1] == 0 and float(r.rms[0, 1]) == float("inf") and float(r.data_cost[0, 1]) == 0.0
    assert bool((r.matched[1] > 0).all()) and bool((r.matched[0, [0, 2]] > 0).all()) and bool(torch.isfinite(r.rms[1]).all())
    assert bool((r.accepted > 0).all()) and not torch.equal(r.p[0, 1], P0[0, 1].to(DEV))      # its sequence is fitted, it too
    held(f"ICP with a gap, plane {plane}", ("icp", plane, 1), r.p.cpu().numpy(), Po.numpy())
    assert r.accepted.tolist() == acc.tolist()
    idx, dist, cost, matched = last_assignment(f, r, pts, topo, plane)
    assert same_bits((r.idx, r.dist, r.data_cost, r.matched), (idx, dist, cost, matched))


@pytest.mark.parametrize("plane", [False, True])
def test_icp_refuses_the_sequence_of_a_point_that_is_not_finite(plane):
    pts, P0, topo = G.icp_case(2, 3)
    bad = np.array(pts)
    bad[1, 2, 100, 1] = np.inf
    f = fitter(37)
    r, ref = icp(f, bad, P0, topo, plane), icp(f, pts, P0, topo, plane)
    assert int(r.accepted[1]) == 0 and torch.equal(r.p[1], P0[1].to(DEV)) and float(r.data_cost[1, 2]) == float("inf")
    assert bool(torch.isfinite(r.data_cost[1, :2]).all()) and int(r.matched[1, 2]) == 0 and bool((r.idx[1, 2] == -1).all())
    assert same_bits([t[0] for t in r], [t[0] for t in ref]) and int(ref.accepted[1]) > 0
    # a start that is not finite: the same
    Pb = P0.clone()
    Pb[0, 0, 3] = float("nan")
    r = icp(f, pts, Pb, topo, plane)
    assert int(r.accepted[0]) == 0 and float(r.data_cost[0, 0]) == float("inf") and same_bits([t[1] for t in r], [t[1] for t in ref])
    assert r.p[0].cpu().numpy().tobytes() == Pb[0].numpy().tobytes()


def test_the_device_reproduces_the_oracles_quality():
    """the quality case of tests/test_fit_seq_verts.py (smooth model, noisy surface clouds along a smooth track, one
    occluded frame): the device's acceleration error and its vertex RMS of every frame against the true meshes are the fp64
    oracle's to 4 x what the fp32 oracle is off by, both ways, and its acceleration error is below that of the device's own
    per-frame point-to-plane ICP"""
    from scat_amd.fit import ManoFitter

    m = LC.smooth_model()
    q = G.quality_case()
    mesh, pts, P0 = G.quality_inputs()
    f = ManoFitter(m.to(DEV))
    faces = LC.topology(778)[0]
    cloud = torch.from_numpy(np.array(pts)).to(DEV)
    r = f.fit_points_sequence(cloud, P0.to(DEV), faces=faces, smooth=G.Q_SMOOTH, rounds=G.Q_ROUNDS, iters=G.Q_ITERS,
                              max_dist=G.Q_TRIM, w_tangent=G.TAU)
    pf = f.fit_points_plane(cloud.flatten(0, 1), P0.flatten(0, 1).to(DEV), faces, rounds=G.Q_ROUNDS, iters=G.Q_ITERS,
                            max_dist=G.Q_TRIM, w_tangent=G.TAU)
    vis = [t for t in range(G.QT) if t != G.Q_GAP]
    acc, rms = QO.accel(m, r.p.cpu(), mesh).numpy(), QO.rms(m, r.p.cpu(), mesh).numpy()
    facc = QO.accel(m, pf.p.cpu().reshape(G.QS, G.QT, 62), mesh).numpy()
    print(f"accel mm: device track {1e3 * acc}, oracle {1e3 * q['accel', 'track']}, device per frame {1e3 * facc}; rms mm: device "
          f"{1e3 * rms}, oracle {1e3 * q['rms', 'track']}")
    assert np.isfinite(r.p.cpu().numpy()).all() and bool((r.accepted > 0).all())
    assert int(r.matched[0, G.Q_GAP]) == 0 and bool((r.matched[0, vis] > 0).all())
    held("quality: acceleration error", ("quality", "accel"), acc, q["accel", "track"])
    held("quality: vertex RMS per frame", ("quality", "rms"), rms, q["rms", "track"])
    assert (acc < facc).all()
    assert f.mesh(r).flatten(0, 1).shape == (G.QS * G.QT, 778, 3)


def _model_ptrs(arena, m, skew):
    return [arena.place(t.cpu(), skew, name=n).data_ptr() for n, t in (
        ("blend", m.blend), ("joint_t", m.joint_t), ("joint_s", m.joint_s), ("weights_t", m.weights_t), ("hands_mean", m.hands_mean_d))]


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_the_mesh_track_inside_guard_bands(fill):
    """every operand, the workspace at exactly the queried size included, between poisoned bands at pointer skews 0, 1 and
    3 floats (the workspace stays 16-byte aligned), both metrics and both starts: bands intact, every output element
    written, results bit for bit those of the plain run; one byte short, a misaligned workspace: SCAT_E_WORKSPACE"""
    from scat_amd._lib import ScatError, lib
    from scat_amd.fit import FIT_SEQ_VERTS_HEADER

    ns, L, V, S, T = lib().bind(FIT_SEQ_VERTS_HEADER), lib(), 37, 3, 3
    m = model(V)
    X, w, n, P1, _, _ = G.step_case(V, 2, T, True)
    cat = lambda t: torch.cat([t, t[:1]], 0).float()
    X, w, n, P1 = cat(X), cat(w), cat(n), cat(P1)
    w[2, 1] = 0.0
    s5 = G.sm(G.SMOOTH)
    stream = torch.cuda.current_stream().cuda_stream
    cases = [(None, 1), (None, 0), (n, 0)]      # (normals, init)
    plain = {i: [t.cpu().numpy() for t in solve(V, X, w, nn, None if init else P1, 3, G.SMOOTH)] for i, (nn, init) in enumerate(cases)}
    need = int(ns.scat_mano_fit_seq_verts_ws(S, T, V))
    assert need > 0
    arena = Arena(DEV, fill, nbytes=16 << 20)
    for skew in (0, 1, 3):
        arena.reset()
        mp = _model_ptrs(arena, m, skew)
        tg, wd, nd = (arena.place(t, skew, name=k) for k, t in (("targets", X), ("weights", w), ("normals", n)))
        for i, (nn, init) in enumerate(cases):
            p = arena.place((S, T, 62), skew, name="p", out=True) if init else arena.place(P1, skew, name="p0", out=True)
            cost = arena.place((S,), skew, name="cost", out=True)
            acc = arena.place((S,), skew, dtype=torch.int32, name="accepted", out=True)
            ws = arena.place((need,), 0, dtype=torch.uint8, name="ws", out=True, finite=False)
            call = lambda ws_ptr, nbytes: ns.scat_mano_fit_seq_verts(
                *mp, tg.data_ptr(), wd.data_ptr(), 0 if nn is None else nd.data_ptr(), p.data_ptr(), cost.data_ptr(), acc.data_ptr(),
                ws_ptr, nbytes, S, T, V, m.parents_packed, 3, init, G.TAU, 1e-3, 1e-6, 1e-6, *s5, ALL, stream)
            for ptr, nbytes in ((ws.data_ptr(), need - 1), (ws.data_ptr() + 4, need)):
                with pytest.raises(ScatError, match=r"\(-3\)"):
                    call(ptr, nbytes)
            call(ws.data_ptr(), need)
            assert L.scat_last_kernel() == (b"mano_fit_seq_verts_v37_t3_i3" if nn is None else b"mano_fit_seq_verts_metric_v37_t3_i3")
            torch.cuda.synchronize()
            arena.check()
            for got, want in zip((p, cost, acc), plain[i]):
                assert got.cpu().numpy().tobytes() == want.tobytes(), (skew, i)


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_the_cloud_track_inside_guard_bands(fill):
    """scat_mano_fit_points_seq with and without a topology, with and without idx / dist, every operand between poisoned
    bands; the int32 topology at a 2-byte offset is refused"""
    from scat_amd._lib import ScatError, lib
    from scat_amd.fit import FIT_SEQ_VERTS_HEADER

    ns, L, V, S, T, N = lib().bind(FIT_SEQ_VERTS_HEADER), lib(), 37, 2, 3, G.ICP_N
    m = model(V)
    pts, P0, topo = G.icp_case(S, T, 1)
    f = fitter(V)
    s5 = G.sm(G.ICP_SMOOTH)
    stream = torch.cuda.current_stream().cuda_stream
    F = int(topo[0].shape[0])
    plain = {plane: icp(f, pts, P0, topo, plane) for plane in (False, True)}
    arena = Arena(DEV, fill, nbytes=16 << 20)
    for skew in (0, 1, 3):
        for plane in (False, True):
            for outs in (True, False):
                arena.reset()
                mp = _model_ptrs(arena, m, skew)
                q = arena.place(torch.from_numpy(np.array(pts)), skew, name="points")
                tp = [arena.place(torch.from_numpy(np.array(t)), skew, name=k).data_ptr() if plane else 0
                      for k, t in zip(("faces", "vf_off", "vf_idx"), topo)]
                p = arena.place(P0, skew, name="p", out=True)
                cost = arena.place((S, T), skew, name="data_cost", out=True)
                acc = arena.place((S,), skew, dtype=torch.int32, name="accepted", out=True)
                idx = arena.place((S, T, N), skew, dtype=torch.int32, name="idx", out=True) if outs else None
                dist = arena.place((S, T, N), skew, name="dist", out=True) if outs else None
                need = int(ns.scat_mano_fit_points_seq_ws(S, T, N, V, F if plane else 0))
                ws = arena.place((need,), 0, dtype=torch.uint8, name="ws", out=True, finite=False)
                call = lambda tpp, ws_ptr, nbytes: ns.scat_mano_fit_points_seq(
                    *mp, q.data_ptr(), 0, *tpp, p.data_ptr(), cost.data_ptr(), acc.data_ptr(), idx.data_ptr() if outs else 0,
                    dist.data_ptr() if outs else 0, ws_ptr, nbytes, S, T, N, V, F if plane else 0, m.parents_packed, G.ICP_ROUNDS,
                    G.ICP_ITERS, G.ICP_TRIM, G.TAU, 1e-3, 1e-6, 1e-6, *s5, ALL, stream)
                for ptr, nbytes in ((ws.data_ptr(), need - 1), (ws.data_ptr() + 8, need)):
                    with pytest.raises(ScatError, match=r"\(-3\)"):
                        call(tp, ptr, nbytes)
                if plane:
                    with pytest.raises(ScatError, match="int32 operands must be 4-byte aligned"):
                        call([tp[0], tp[1] + 2, tp[2]], ws.data_ptr(), need)
                call(tp, ws.data_ptr(), need)
                torch.cuda.synchronize()
                arena.check()
                want = plain[plane]
                got = [(p, want.p), (cost, want.data_cost), (acc, want.accepted)] + ([(idx, want.idx), (dist, want.dist)] if outs else [])
                for g, wnt in got:
                    assert g.cpu().numpy().tobytes() == wnt.cpu().numpy().tobytes(), (skew, plane, outs)
