"""The MANO fit to a full mesh on a real MI355X (include/scat_mano_fit_verts.h, scat_amd/fit.py) against the fp64 oracle of
tests/_fit_verts_oracle.py and inside guard bands.  Inputs and models come from scat_amd.synth.

Every gate that compares fp32 with fp64 is 4 x the error of the oracle itself run in fp32 on the CPU against its fp64 run
on the same inputs (E32 below, printed by tools/fit_verts_gates.py), normalised max |a - b| / max |b|: the project's rule
for the MANO gates.  The factor covers the kernel's different order of sums (forward mode, folded regressor, tiles) and
device sin / cos / exp being a unit or two in the last place off libm."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_oracle as FO  # noqa: E402
import _fit_verts_oracle as VO  # noqa: E402
from _fit_verts_cases import (FIT_V, ITERS, JAC_B, JAC_V, JOINT_MAP, NB, T_, case, edge_case, host_model, joints_case,  # noqa: E402
                              layer_case, recovery_case, seeded, step_case)
from _guard import Arena  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
# The oracle in fp32 on the CPU against itself in fp64, max |a - b| / max |b|, as tools/fit_verts_gates.py printed them.
#   verts, jac   the mesh and its Jacobian on the inputs of case(B, V) and of edge_case()
#   jjac         the joints' Jacobian of tests/_fit_oracle.py on the inputs of case(3, V): the tips cross-check's other side
#   step         the accepted p after one LM step from step_case(V) (lambda 1e-2)
#   cost         the oracle's cost function at its own iterate after k iterations of recovery_case(V)
E32 = {
    ("verts", 1, 1): 2.803e-07, ("jac", 1, 1): 3.521e-07, ("verts", 3, 1): 5.424e-07, ("jac", 3, 1): 4.418e-07,
    ("verts", 65, 1): 8.875e-07, ("jac", 65, 1): 8.157e-07, ("verts", 1, 37): 1.319e-07, ("jac", 1, 37): 1.646e-07,
    ("verts", 3, 37): 1.234e-07, ("jac", 3, 37): 1.970e-07, ("verts", 65, 37): 2.801e-07, ("jac", 65, 37): 2.155e-07,
    ("verts", 1, 778): 2.230e-07, ("jac", 1, 778): 2.031e-07, ("verts", 3, 778): 1.761e-07, ("jac", 3, 778): 2.097e-07,
    ("verts", 65, 778): 2.945e-07, ("jac", 65, 778): 2.825e-07, ("verts", 1, 1536): 1.662e-07, ("jac", 1, 1536): 1.892e-07,
    ("verts", 3, 1536): 2.016e-07, ("jac", 3, 1536): 1.792e-07, ("verts", 65, 1536): 2.425e-07, ("jac", 65, 1536): 2.241e-07,
    ("verts", "edge"): 3.419e-07, ("jac", "edge"): 2.402e-07, ("jjac", 3, 37): 1.445e-07, ("jjac", 3, 778): 2.117e-07,
    ("step", 37): 8.849e-07, ("step", 778): 1.986e-07,
    ("cost", 37, 1): 1.154e-07, ("cost", 37, 5): 1.244e-06, ("cost", 37, 20): 7.846e-08,
    ("cost", 778, 1): 1.418e-07, ("cost", 778, 5): 5.367e-08, ("cost", 778, 20): 5.367e-08,
}
GATE = {k: 4.0 * v for k, v in E32.items()}
# scat_mano_bwd's own gates (tests/test_gpu_mano.py: 4 x the reference's fp32 error), for the cross-check
GATE_BWD = {"drots": 6.244e-07, "dposes": 5.980e-07, "dbetas": 8.672e-07}


def model(V):
    m = host_model(V)
    return m if m.device is not None else m.to(DEV)


@pytest.fixture(scope="module", autouse=True)
def device():
    from scat_amd._lib import lib

    lib().scat_check_device()


def run_jac(m, P):
    from scat_amd.fit import mano_verts_jac

    P = T_(P).to(DEV)
    x, jac = mano_verts_jac(m, P[:, :3], P[:, 3:48], P[:, 48:58])
    return x.cpu().numpy(), jac.cpu().numpy()


def held(tag, key, got, want):
    e = VO.rel(got, want)
    print(f"{tag}: {key[0]} {e:.3e} (gate {GATE[key]:.3e} = 4 x {E32[key]:.3e})")
    assert np.isfinite(got).all(), (tag, key)
    assert e <= GATE[key], (tag, key, e, GATE[key])


# V = 1 and 37: below, and no multiple of, the tile of 32 vertices and the workgroup of 256; V = 1536: SCAT_MANO_MAX_V.
# B = 65: more workgroups than one wave of them per XCD.
@pytest.mark.parametrize("V", JAC_V)
@pytest.mark.parametrize("B", JAC_B)
def test_vertex_jacobian_matches_the_oracle(B, V):
    P, x, jac = case(B, V)
    gx, gj = run_jac(model(V), P)
    assert gx.shape == (B, V, 3) and gj.shape == (B, 3 * V, 58)
    held(f"B {B} V {V}", ("verts", B, V), gx, x)
    held(f"B {B} V {V}", ("jac", B, V), gj, jac)


def test_vertex_jacobian_edge_batch():
    P, x, jac = edge_case()
    gx, gj = run_jac(model("edge"), P)
    held("edge", ("verts", "edge"), gx, x)
    held("edge", ("jac", "edge"), gj, jac)
    for b in range(8):      # sample by sample as well, so that no large sample carries a small one
        e = VO.rel(gj[b], jac[b])
        print(f"  sample {b}: jac {e:.3e}")
        assert e <= GATE[("jac", "edge")], (b, e)


@pytest.mark.parametrize("V", FIT_V)
def test_vertex_jacobian_agrees_with_the_backward_kernel(V):
    """row 3 v + c of the Jacobian is scat_mano_bwd's gradient for the one-hot cotangent on vertex v, component c: 3 V
    cotangents per sample in one launch; the two kernels agree to the sum of their gates"""
    from scat_amd.mano import mano_bwd

    B, R = 3, 3 * V
    P, _, _ = case(B, V)
    m = model(V)
    _, gj = run_jac(m, P)
    Pr = T_(P).to(DEV).repeat_interleave(R, dim=0).contiguous()
    dout = torch.zeros(B * R, 21 + V, 3, device=DEV)
    dout.view(B, R, -1)[:, torch.arange(R), 63 + torch.arange(R)] = 1.0
    dr, dp, db = mano_bwd(m, Pr[:, :3].contiguous(), Pr[:, 3:48].contiguous(), Pr[:, 48:58].contiguous(), dout)
    rows = torch.cat([dr, dp, db], dim=1).reshape(B, R, 58).cpu().numpy()
    for name, sl in (("drots", slice(0, 3)), ("dposes", slice(3, 48)), ("dbetas", slice(48, 58))):
        e, gate = VO.rel(gj[:, :, sl], rows[:, :, sl]), GATE[("jac", B, V)] + GATE_BWD[name]
        print(f"V {V} {name}: jac vs bwd {e:.3e} (gate {gate:.3e})")
        assert e <= gate, (name, e, gate)


@pytest.mark.parametrize("V", FIT_V)
def test_tip_rows_agree_with_the_joints_jacobian(V):
    """the five tips are vertices: their rows here and rows 48..62 of scat_mano_joints_jac, to the sum of the two gates"""
    from scat_amd.fit import mano_joints_jac

    B = 3
    P, _, _ = case(B, V)
    m = model(V)
    _, gj = run_jac(m, P)
    Pd = T_(P).to(DEV)
    _, jj = mano_joints_jac(m, Pd[:, :3], Pd[:, 3:48], Pd[:, 48:58])
    rows = [3 * t + c for t in m.tips for c in range(3)]
    e, gate = VO.rel(gj[:, rows], jj.cpu().numpy()[:, 48:63]), GATE[("jac", B, V)] + GATE[("jjac", B, V)]
    print(f"V {V}: tip rows against the joints' Jacobian {e:.3e} (gate {gate:.3e})")
    assert e <= gate


def fitter(V, **kw):
    from scat_amd.fit import ManoFitter

    return ManoFitter(model(V), joint_map=JOINT_MAP, **kw)


def same_bits(a, b):
    return all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("V", FIT_V)
def test_one_step_matches_the_oracle(V):
    Tv, P1, Ps, c = step_case(V)
    r = fitter(V, lambda0=1e-2).fit_vertices(Tv.to(DEV), init=P1.float().to(DEV), iters=1)
    assert r.accepted.tolist() == [1] * NB
    e = VO.rel(r.p.cpu().numpy(), Ps.numpy())
    print(f"V {V}: one step {e:.3e} (gate {GATE[('step', V)]:.3e} = 4 x {E32[('step', V)]:.3e})")
    assert e <= GATE[("step", V)]


@pytest.mark.parametrize("V", FIT_V)
def test_cost_is_monotone_and_is_the_oracles(V):
    m = model(V)
    P, Tv, P0, _, _, _ = recovery_case(V)
    f = fitter(V)
    Td, costs = Tv.to(DEV), []
    for k in ITERS:
        r = f.fit_vertices(Td, iters=k)
        assert bool((r.accepted <= k).all()) and bool((r.accepted >= 0).all())
        c = r.cost.cpu().double()
        costs.append(c)
        # the oracle's cost function at the returned p, in the metric of every gate here
        with torch.no_grad():
            want = VO.cost(m, r.p.cpu().double(), Tv.double(), torch.ones(NB, V, dtype=torch.float64), f.w_pose, f.w_beta)
        e = VO.rel(c.numpy(), want.numpy())
        print(f"V {V} iters {k}: cost {c.numpy()}, against the oracle's at p {e:.3e} (gate {GATE[('cost', V, k)]:.3e} = 4 x "
              f"{E32[('cost', V, k)]:.3e})")
        assert e <= GATE[("cost", V, k)], (k, e)
    for a, b in zip(costs, costs[1:]):
        assert bool((b <= a).all())
    assert bool((costs[-1] < costs[0]).all())


@pytest.mark.parametrize("V", FIT_V)
def test_recovers_seeded_hands(V):
    """per sample, vertex RMS <= 2 x the fp64 oracle's final RMS + 1e-5 m, the form of the joints gate (the factor: another
    accept / reject history in fp32; the floor: fp32 rounding at a 0.1 - 0.3 m hand).  The same hands fitted to their 21
    joints keep a strictly larger vertex error, the twist and shape that joints leave open, and that fit as a warm start
    reaches the same gate."""
    m = model(V)
    P, Tv, P0, Pf, want, _ = recovery_case(V)
    Tj, _, _ = joints_case(V)
    f = fitter(V, w_pose=1e-6, w_beta=1e-6, iters=20)
    r = f.fit_vertices(Tv.to(DEV))
    rj = f.fit(Tj.to(DEV))
    rw = f.fit_vertices(Tv.to(DEV), init=rj)
    got, warm = VO.rms(m, r.p.cpu(), Tv).numpy(), VO.rms(m, rw.p.cpu(), Tv).numpy()
    start = VO.rms(m, P0, Tv).numpy()
    left = (f.mesh(rj).cpu().double() - Tv.double()).pow(2).sum(2).mean(1).sqrt().numpy()
    for b in range(NB):
        print(f"V {V} hand {b}: start {1e3 * start[b]:.3f} mm, oracle {1e3 * want[b]:.4f} mm, kernel {1e3 * got[b]:.4f} mm, "
              f"warm from the joints fit {1e3 * warm[b]:.4f} mm (gate {1e3 * (2 * want[b] + 1e-5):.4f} mm), the joints fit "
              f"alone {1e3 * left[b]:.3f} mm, accepted {int(r.accepted[b])} / {int(rw.accepted[b])}")
    assert np.isfinite(r.p.cpu().numpy()).all() and np.isfinite(rw.p.cpu().numpy()).all()
    assert (got <= 2 * want + 1e-5).all(), (got, want)
    assert (warm <= 2 * want + 1e-5).all(), (warm, want)
    assert (left > got).all(), (left, got)
    # ManoFitter.mesh is the oracle's model_verts at the returned p, to fp32 rounding of a 0.1 - 0.3 m hand
    assert np.abs(f.mesh(r).cpu().numpy() - VO.model_verts(m, r.p.cpu().double()).numpy()).max() < 1e-6


def test_zero_weight_vertices_do_not_count():
    V = 37
    _, Tv, _, _, _, _ = recovery_case(V)
    f = fitter(V)
    w = torch.ones(NB, V)
    w[:, 4], w[2, 9], w[:, 33:] = 0.0, 0.0, 0.0
    far = Tv.clone()
    far[:, 4], far[2, 9], far[:, 33:] = 1e6, -1e6, 3e37
    a, b = f.fit_vertices(Tv.to(DEV), w.to(DEV)), f.fit_vertices(far.to(DEV), w.to(DEV))
    assert same_bits(a, b)
    assert bool((a.accepted > 0).all())
    p0 = a.p.clone()
    a, b = f.fit_vertices(Tv.to(DEV), w.to(DEV), init=p0, iters=3), f.fit_vertices(far.to(DEV), w.to(DEV), init=p0, iters=3)
    assert same_bits(a, b)


def test_frozen_unknowns_keep_their_bits():
    from scat_amd.fit import free_mask

    V = 37
    Tv, P1, _, _ = step_case(V)
    f = fitter(V)
    p0 = P1.float().to(DEV)
    r1 = f.fit_vertices(Tv.to(DEV), init=p0, iters=1, free=free_mask(betas=False, log_scale=False))
    r = f.fit_vertices(Tv.to(DEV), init=p0, iters=8, free=free_mask(betas=False, log_scale=False))
    assert torch.equal(r.betas, p0[:, 48:58]) and torch.equal(r.p[:, 61], p0[:, 61])
    assert not torch.equal(r.poses, p0[:, 3:48]) and bool((r.accepted > 0).all())
    c0 = VO.cost(model(V), P1, Tv.double(), torch.ones(NB, V, dtype=torch.float64), f.w_pose, f.w_beta)
    assert bool((r.cost.cpu().double() < c0).all()) and bool((r.cost <= r1.cost).all())


@pytest.mark.parametrize("with_init", [False, True])
def test_unusable_hands_are_not_fitted(with_init):
    """a target or weight that is not finite, or a negative weight, anywhere in a hand: cost +inf, accepted 0, p the start;
    the hands beside it are fitted as if it were not there"""
    V = 37
    _, Tv, P0, _, _, _ = recovery_case(V)
    f = fitter(V, iters=6)
    T6, w = Tv.clone(), torch.ones(NB, V)
    T6[1, 7, 2], T6[3, 36, 0] = float("nan"), float("inf")
    w[4, 0], w[5, 20] = -1.0, float("nan")
    good, bad = [0, 2], [1, 3, 4, 5]
    init = P0.float().to(DEV) if with_init else None
    r = f.fit_vertices(T6.to(DEV), w.to(DEV), init=init)
    ref = f.fit_vertices(Tv[good].to(DEV), w[good].to(DEV), init=None if init is None else init[good])
    assert torch.isfinite(r.p).all()
    for b in bad:
        assert float(r.cost[b]) == float("inf") and int(r.accepted[b]) == 0
        assert torch.equal(r.p[b], init[b] if with_init else torch.zeros(62, device=DEV))
    assert same_bits([x[good] for x in r], ref) and bool((ref.accepted > 0).all())


def test_same_call_same_bits():
    P, _, _ = case(65, 778)
    a, b = run_jac(model(778), P), run_jac(model(778), P)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    _, Tv, _, _, _, _ = recovery_case(778)
    f = fitter(778)
    assert same_bits(f.fit_vertices(Tv.to(DEV)), f.fit_vertices(Tv.to(DEV)))


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_both_kernels_inside_guard_bands(fill):
    """every operand of both entry points between poisoned bands at pointer skews 0, 1 and 3 floats: bands intact, every
    output element written, results bit for bit those of the skew-0 run and of the plain run outside the arena"""
    from scat_amd._lib import lib
    from scat_amd.fit import FIT_VERTS_HEADER, mano_verts_jac

    L, V, B = lib(), 37, 3
    ns = L.bind(FIT_VERTS_HEADER)
    m = model(V)
    P, _, _ = case(B, V)
    _, Tv, P0, _, _, _ = recovery_case(V)
    Tv, w = Tv[:B], torch.full((B, V), 0.75)
    stream = torch.cuda.current_stream().cuda_stream
    Pd = T_(P).to(DEV)
    plain = [t.cpu().numpy() for t in mano_verts_jac(m, Pd[:, :3], Pd[:, 3:48], Pd[:, 48:58])]
    r = fitter(V, iters=4).fit_vertices(Tv.to(DEV), w.to(DEV))
    plain += [r.p.cpu().numpy(), r.cost.cpu().numpy(), r.accepted.cpu().numpy()]
    r = fitter(V, iters=4).fit_vertices(Tv.to(DEV), w.to(DEV), init=P0[:B].float().to(DEV))
    plain += [r.p.cpu().numpy(), r.cost.cpu().numpy(), r.accepted.cpu().numpy()]
    arena = Arena(DEV, fill, nbytes=16 << 20)
    for skew in (0, 1, 3):
        arena.reset()
        mod = [arena.place(t.cpu(), skew, name=n) for n, t in (("blend", m.blend), ("joint_t", m.joint_t), ("joint_s", m.joint_s),
                                                               ("weights_t", m.weights_t), ("hands_mean", m.hands_mean_d))]
        mp = [t.data_ptr() for t in mod]
        rots, poses, betas = (arena.place(T_(P[:, s]), skew, name=n) for n, s in
                              (("rots", slice(0, 3)), ("poses", slice(3, 48)), ("betas", slice(48, 58))))
        x = arena.place((B, V, 3), skew, name="verts", out=True)
        jac = arena.place((B, 3 * V, 58), skew, name="jac", out=True)
        ns.scat_mano_verts_jac(*mp, rots.data_ptr(), poses.data_ptr(), betas.data_ptr(), x.data_ptr(), jac.data_ptr(), B, V,
                               m.parents_packed, stream)
        assert L.scat_last_kernel() == b"mano_verts_jac_v37"
        tg = arena.place(Tv, skew, name="targets")
        wd = arena.place(w, skew, name="weights")
        outs = []
        for init in (1, 0):
            p = arena.place((B, 62), skew, name="p", out=True) if init else arena.place(P0[:B].float(), skew, name="p0", out=True)
            cost = arena.place((B,), skew, name="cost", out=True)
            acc = arena.place((B,), skew, dtype=torch.int32, name="accepted", out=True)
            ns.scat_mano_fit_verts(*mp, tg.data_ptr(), wd.data_ptr(), p.data_ptr(), cost.data_ptr(), acc.data_ptr(), B, V,
                                   m.parents_packed, 4, init, 1e-3, 1e-6, 1e-6, (1 << 62) - 1, stream)
            assert L.scat_last_kernel() == b"mano_fit_verts_v37_i4"
            outs += [p, cost, acc]
        torch.cuda.synchronize()
        arena.check()
        assert bool((outs[2] >= 0).all()) and bool((outs[2] <= 4).all())
        for got, want in zip([x, jac] + outs, plain):
            assert got.cpu().numpy().tobytes() == want.tobytes(), skew


def test_layer_output_to_fit_to_mesh_to_evaluator():
    """ManoLayer's [B,21+V,3] -> fit_mesh_outputs -> mesh -> MeshEvaluator: the raw mean vertex error is within the
    recovery gate (a mean of distances is at most their RMS), and the result is a FitResult like any other"""
    from scat_amd.mano import ManoLayer
    from scat_amd.mesh_evaluator import MeshEvaluator

    V = 778
    m = model(V)
    P, Tv, _, _, want, _ = layer_case(V)
    Pd = P.float().to(DEV)
    with torch.no_grad():
        out = ManoLayer(m)(Pd[:, :3].contiguous(), Pd[:, 3:48].contiguous(), Pd[:, 48:58].contiguous())
    assert out.shape == (NB, 21 + V, 3)
    assert np.abs(out[:, 21:].cpu().numpy() - Tv.numpy()).max() < 1e-6      # the targets the oracle fitted, to fp32 rounding
    f = fitter(V)
    r = f.fit_mesh_outputs(out)
    assert r.rots.shape == (NB, 3) and r.poses.shape == (NB, 45) and r.betas.shape == (NB, 10) and r.trans.shape == (NB, 3)
    assert r.scale.shape == (NB,) and r.cost.shape == (NB,) and r.accepted.dtype == torch.int32 and r.p.shape == (NB, 62)
    verts, joints = f.mesh(r), f.joints(r)
    assert verts.shape == (NB, V, 3) and verts.is_cuda and joints.shape == (NB, 21, 3)
    ev = MeshEvaluator()
    ev.update(verts, out[:, 21:].contiguous())
    res = ev.result()
    gate_mm = 1e3 * (2 * want + 1e-5)
    per_hand = 1e3 * (verts - out[:, 21:]).double().pow(2).sum(2).sqrt().mean(1).cpu().numpy()
    print(f"MPVPE {res['mpvpe_mm']:.5f} mm; per hand {per_hand} mm, gates {gate_mm} mm")
    assert res["frames_kept"] == NB and (per_hand <= gate_mm).all()
    assert res["mpvpe_mm"] <= gate_mm.mean() and abs(res["mpvpe_mm"] - per_hand.mean()) < 1e-4
