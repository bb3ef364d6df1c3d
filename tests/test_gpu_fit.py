"""The MANO fit on a real MI355X (include/scat_mano_fit.h, scat_amd/fit.py) against the fp64 oracle of
tests/_fit_oracle.py and inside guard bands.  Inputs and models come from scat_amd.synth.

Every gate that compares fp32 with fp64 is 4 x the error of the oracle itself run in fp32 on the CPU against its fp64 run
on the same inputs (E32 below, printed by tools/fit_gates.py), normalised max |a - b| / max |b|: the project's rule for
the MANO gates.  The factor covers the kernel's different order of sums (forward mode, folded regressor) and device
sin / cos / exp being a unit or two in the last place off libm."""
import os
import sys

import numpy as np
import pytest
import torch

from scat_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_oracle as FO  # noqa: E402
from _fit_cases import JOINT_MAP, T_, case, edge_batch, host_model, recovery_case, step_case  # noqa: E402
from _guard import Arena  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The oracle in fp32 on the CPU against itself in fp64, max |a - b| / max |b|, as tools/fit_gates.py printed them.
#   x, jac   the joints and the Jacobian on the inputs of case(B, V) and of edge_batch()
#   step     the accepted p after one LM step from step_case(V) (lambda 1e-2)
#   cost     the oracle's cost function at its own iterate after k iterations of recovery_case(778)
E32 = {
    ("x", 1, 37): 1.017e-07, ("jac", 1, 37): 1.786e-07, ("x", 3, 37): 1.554e-07, ("jac", 3, 37): 1.520e-07,
    ("x", 65, 37): 2.297e-07, ("jac", 65, 37): 1.878e-07, ("x", 1, 778): 1.213e-07, ("jac", 1, 778): 2.065e-07,
    ("x", 3, 778): 1.592e-07, ("jac", 3, 778): 1.614e-07, ("x", 65, 778): 2.467e-07, ("jac", 65, 778): 1.904e-07,
    ("x", "edge"): 3.802e-07, ("jac", "edge"): 3.355e-07, ("step", 37): 1.507e-06, ("step", 778): 3.936e-06,
    ("cost", 1): 1.149e-07, ("cost", 2): 1.489e-07, ("cost", 5): 1.732e-07, ("cost", 10): 2.225e-07,
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
    from scat_amd.fit import mano_joints_jac

    P = T_(P).to(DEV)
    x, jac = mano_joints_jac(m, P[:, :3], P[:, 3:48], P[:, 48:58])
    return x.cpu().numpy(), jac.cpu().numpy()


def held(tag, key, got, want):
    e = FO.rel(got, want)
    print(f"{tag}: {key[0]} {e:.3e} (gate {GATE[key]:.3e} = 4 x {E32[key]:.3e})")
    assert np.isfinite(got).all(), (tag, key)
    assert e <= GATE[key], (tag, key, e, GATE[key])


# V = 37: less than one wavefront and odd; V = 778: MANO.  B = 65: more workgroups than one wave of them is wide.
@pytest.mark.parametrize("V", [37, 778])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_jacobian_matches_the_oracle(B, V):
    P, x, jac = case(B, V)
    gx, gj = run_jac(model(V), P)
    assert gx.shape == (B, 21, 3) and gj.shape == (B, 63, 58)
    held(f"B {B} V {V}", ("x", B, V), gx, x)
    held(f"B {B} V {V}", ("jac", B, V), gj, jac)
    assert np.abs(gx[:, 1]).max() == 0.0 and np.abs(gj[:, 3:6]).max() == 0.0      # joint 1 is the origin


def test_jacobian_edge_batch():
    P, x, jac = edge_batch()
    gx, gj = run_jac(model("edge"), P)
    held("edge", ("x", "edge"), gx, x)
    held("edge", ("jac", "edge"), gj, jac)
    for b in range(8):      # sample by sample as well, so that no large sample carries a small one
        e = FO.rel(gj[b], jac[b])
        print(f"  sample {b}: jac {e:.3e}")
        assert e <= GATE[("jac", "edge")], (b, e)


@pytest.mark.parametrize("V", [37, 778])
def test_jacobian_agrees_with_the_backward_kernel(V):
    """row 3 j + c of the Jacobian is scat_mano_bwd's gradient for the one-hot cotangent on joint j, component c: 63
    cotangents per sample in one launch of 63 B; the two kernels agree to the sum of their gates"""
    from scat_amd.mano import mano_bwd

    B = 3
    P, _, _ = case(B, V)
    m = model(V)
    _, gj = run_jac(m, P)
    Pr = T_(P).to(DEV).repeat_interleave(63, dim=0).contiguous()
    dout = torch.zeros(B * 63, 21 + V, 3, device=DEV)
    dout.view(B, 63, -1)[:, torch.arange(63), torch.arange(63)] = 1.0
    dr, dp, db = mano_bwd(m, Pr[:, :3].contiguous(), Pr[:, 3:48].contiguous(), Pr[:, 48:58].contiguous(), dout)
    rows = torch.cat([dr, dp, db], dim=1).reshape(B, 63, 58).cpu().numpy()
    for name, sl in (("drots", slice(0, 3)), ("dposes", slice(3, 48)), ("dbetas", slice(48, 58))):
        e, gate = FO.rel(gj[:, :, sl], rows[:, :, sl]), GATE[("jac", B, V)] + GATE_BWD[name]
        print(f"V {V} {name}: jac vs bwd {e:.3e} (gate {gate:.3e})")
        assert e <= gate, (name, e, gate)


def fitter(V, **kw):
    from scat_amd.fit import ManoFitter

    return ManoFitter(model(V), joint_map=JOINT_MAP, **kw)


@pytest.mark.parametrize("V", [37, 778])
def test_one_step_matches_the_oracle(V):
    T, P1, Ps, c = step_case(V)
    r = fitter(V, lambda0=1e-2).fit(T.to(DEV), init=P1.float().to(DEV), iters=1)
    assert r.accepted.tolist() == [1] * 6
    e = FO.rel(r.p.cpu().numpy(), Ps.numpy())
    print(f"V {V}: one step {e:.3e} (gate {GATE[('step', V)]:.3e} = 4 x {E32[('step', V)]:.3e})")
    assert e <= GATE[("step", V)]


@pytest.mark.parametrize("V", [37, 778])
def test_recovers_seeded_hands(V):
    """the gate is on the joints, never on the parameters: twist about a bone is not observable from joints.  Per sample
    RMS <= 2 x the fp64 oracle's final RMS + 1e-5 m (the factor: another accept / reject history in fp32; the floor: fp32
    rounding at a 0.1 - 0.3 m hand)"""
    m = model(V)
    P, T, P0, Pf, want, _ = recovery_case(V)
    f = fitter(V, w_pose=1e-6, w_beta=1e-6, iters=20)
    r = f.fit(T.to(DEV))
    got = FO.rms(m, r.p.cpu(), T, JOINT_MAP).numpy()
    start = FO.rms(m, P0, T, JOINT_MAP).numpy()
    for b in range(6):
        print(f"V {V} sample {b}: start {1e3 * start[b]:.3f} mm, oracle {1e3 * want[b]:.4f} mm, kernel {1e3 * got[b]:.4f} mm "
              f"(gate {1e3 * (2 * want[b] + 1e-5):.4f} mm), accepted {int(r.accepted[b])}")
    assert np.isfinite(r.p.cpu().numpy()).all()
    assert (got <= 2 * want + 1e-5).all(), (got, want)
    # ManoFitter.joints is the oracle's model_joints at the returned p, to fp32 rounding of a 0.1 - 0.3 m hand
    assert np.abs(f.joints(r).cpu().numpy() - FO.model_joints(m, r.p.cpu().double(), JOINT_MAP).numpy()).max() < 1e-6


def test_cost_is_monotone_and_is_the_oracles():
    V = 778
    m = model(V)
    P, T, P0, _, _, _ = recovery_case(V)
    f = fitter(V)
    Td, costs = T.to(DEV), []
    for k in (1, 2, 5, 10):
        r = f.fit(Td, iters=k)
        assert bool((r.accepted <= k).all()) and bool((r.accepted >= 0).all())
        c = r.cost.cpu().double()
        costs.append(c)
        # the oracle's cost function at the returned p, in the metric of every gate here
        p64 = r.p.cpu().double()
        with torch.no_grad():
            want = FO.cost(m, p64, T.double(), torch.ones(6, 21, dtype=torch.float64), JOINT_MAP, f.w_pose, f.w_beta)
        e = FO.rel(c.numpy(), want.numpy())
        print(f"iters {k}: cost {c.numpy()}, against the oracle's at p {e:.3e} (gate {GATE[('cost', k)]:.3e} = 4 x "
              f"{E32[('cost', k)]:.3e}; the Jacobian's gate {GATE[('jac', 3, V)]:.3e})")
        assert e <= GATE[("cost", k)] and e <= GATE[("jac", 3, V)], (k, e)
    for a, b in zip(costs, costs[1:]):
        assert bool((b <= a).all())
    assert bool((costs[-1] < costs[0]).all())


def test_frozen_unknowns_keep_their_bits():
    from scat_amd.fit import free_mask

    V = 37
    T, P1, _, _ = step_case(V)
    f = fitter(V)
    p0 = P1.float().to(DEV)
    r1 = f.fit(T.to(DEV), init=p0, iters=1, free=free_mask(betas=False, log_scale=False))
    r = f.fit(T.to(DEV), init=p0, iters=8, free=free_mask(betas=False, log_scale=False))
    assert torch.equal(r.betas, p0[:, 48:58]) and torch.equal(r.p[:, 61], p0[:, 61])
    assert not torch.equal(r.poses, p0[:, 3:48]) and bool((r.accepted > 0).all())
    c0 = FO.cost(model(V), P1, T.double(), torch.ones(6, 21, dtype=torch.float64), JOINT_MAP, f.w_pose, f.w_beta)
    assert bool((r.cost.cpu().double() < c0).all()) and bool((r.cost <= r1.cost).all())


def test_zero_weight_joints_do_not_count():
    V = 37
    _, T, _, _, _, _ = recovery_case(V)
    f = fitter(V)
    w = torch.ones(6, 21)
    w[:, 4], w[2, 9] = 0.0, 0.0
    far = T.clone()
    far[:, 4], far[2, 9] = 1e6, -1e6
    a, b = f.fit(T.to(DEV), w.to(DEV)), f.fit(far.to(DEV), w.to(DEV))
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert bool((a.accepted > 0).all())


@pytest.mark.parametrize("with_init", [False, True])
def test_non_finite_targets_are_not_fitted(with_init):
    V = 37
    _, T, P0, _, _, _ = recovery_case(V)
    f = fitter(V, iters=6)
    T4 = T[:4].clone()
    T4[1, 7, 2], T4[3, 0, 0] = float("nan"), float("inf")
    good = [0, 2]
    init = P0[:4].float().to(DEV) if with_init else None
    r = f.fit(T4.to(DEV), init=init)
    ref = f.fit(T[good].to(DEV), init=None if init is None else init[good])
    assert torch.isfinite(r.p).all()
    for b in (1, 3):
        assert float(r.cost[b]) == float("inf") and int(r.accepted[b]) == 0
        assert torch.equal(r.p[b], init[b] if with_init else torch.zeros(62, device=DEV))
    for x, y in zip(r, ref):
        assert x[good].cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_same_call_same_bits():
    P, _, _ = case(65, 778)
    a, b = run_jac(model(778), P), run_jac(model(778), P)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    _, T, _, _, _, _ = recovery_case(778)
    f = fitter(778)
    a, b = f.fit(T.to(DEV)), f.fit(T.to(DEV))
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_both_kernels_inside_guard_bands(fill):
    """every operand of both entry points between poisoned bands at pointer skews 0, 1 and 3 floats: bands intact, every
    output element written, results bit for bit those of the skew-0 run and of the plain run outside the arena"""
    from scat_amd._lib import lib
    from scat_amd.fit import mano_joints_jac

    L, V, B = lib(), 37, 3
    m = model(V)
    P, _, _ = case(B, V)
    _, T, P0, _, _, _ = recovery_case(V)
    T, w = T[:B], torch.full((B, 21), 0.75)
    stream = torch.cuda.current_stream().cuda_stream
    Pd = T_(P).to(DEV)
    plain = [t.cpu().numpy() for t in mano_joints_jac(m, Pd[:, :3], Pd[:, 3:48], Pd[:, 48:58])]
    r = fitter(V, iters=4).fit(T.to(DEV), w.to(DEV))
    plain += [r.p.cpu().numpy(), r.cost.cpu().numpy(), r.accepted.cpu().numpy()]
    r = fitter(V, iters=4).fit(T.to(DEV), w.to(DEV), init=P0[:B].float().to(DEV))
    plain += [r.p.cpu().numpy(), r.cost.cpu().numpy(), r.accepted.cpu().numpy()]
    arena = Arena(DEV, fill, nbytes=16 << 20)
    for skew in (0, 1, 3):
        arena.reset()
        mod = [arena.place(t.cpu(), skew, name=n) for n, t in (("blend", m.blend), ("joint_t", m.joint_t), ("joint_s", m.joint_s),
                                                               ("weights_t", m.weights_t), ("hands_mean", m.hands_mean_d))]
        mp = [t.data_ptr() for t in mod]
        rots, poses, betas = (arena.place(T_(P[:, s]), skew, name=n) for n, s in
                              (("rots", slice(0, 3)), ("poses", slice(3, 48)), ("betas", slice(48, 58))))
        x = arena.place((B, 21, 3), skew, name="joints", out=True)
        jac = arena.place((B, 63, 58), skew, name="jac", out=True)
        L.scat_mano_joints_jac(*mp, rots.data_ptr(), poses.data_ptr(), betas.data_ptr(), x.data_ptr(), jac.data_ptr(), B, V,
                               m.parents_packed, *m.tips, stream)
        assert L.scat_last_kernel() == b"mano_joints_jac_v37"
        tg = arena.place(T, skew, name="targets")
        wd = arena.place(w, skew, name="weights")
        jm = arena.place(torch.tensor(JOINT_MAP, dtype=torch.int32), skew, name="joint_map")
        outs = []
        for init in (1, 0):
            p = arena.place((B, 62), skew, name="p", out=True) if init else arena.place(P0[:B].float(), skew, name="p0", out=True)
            cost = arena.place((B,), skew, name="cost", out=True)
            acc = arena.place((B,), skew, dtype=torch.int32, name="accepted", out=True)
            L.scat_mano_fit(*mp, tg.data_ptr(), wd.data_ptr(), jm.data_ptr(), p.data_ptr(), cost.data_ptr(), acc.data_ptr(), B, V,
                            m.parents_packed, *m.tips, 4, init, 1e-3, 1e-6, 1e-6, (1 << 62) - 1, stream)
            assert L.scat_last_kernel() == b"mano_fit_v37_i4"
            outs += [p, cost, acc]
        torch.cuda.synchronize()
        arena.check()
        assert bool((outs[2] >= 0).all()) and bool((outs[2] <= 4).all())
        for got, want in zip([x, jac] + outs, plain):
            assert got.cpu().numpy().tobytes() == want.tobytes(), skew


def test_fit_outputs_to_mesh_to_renderer():
    """the network's [B,66] -> fit -> mesh -> MeshRenderer with the predicted camera: shapes, and the fitted joints
    project to within the joint-RMS gate (scaled to pixels by the camera) of the input joints"""
    from scat_amd.render import MeshRenderer, project_outputs

    V, B = 778, 6
    m = model(V)
    _, T, _, _, want, _ = recovery_case(V)
    T = T - T[:, :1]      # root-relative, as the networks predict
    cam = T_(np.stack([synth.uniform(5, "cam.s", (B,), 3.0, 5.0), synth.uniform(5, "cam.tx", (B,), -0.05, 0.05),
                       synth.uniform(5, "cam.ty", (B,), -0.05, 0.05)], axis=1).astype(np.float32))
    out66 = torch.cat([cam, T.reshape(B, 63)], dim=1).to(DEV)
    f = fitter(V)
    r = f.fit_outputs(out66)
    assert r.rots.shape == (B, 3) and r.poses.shape == (B, 45) and r.betas.shape == (B, 10) and r.trans.shape == (B, 3)
    assert r.scale.shape == (B,) and r.cost.shape == (B,) and r.accepted.shape == (B,) and r.accepted.dtype == torch.int32
    verts, joints = f.mesh(r), f.joints(r)
    assert verts.shape == (B, V, 3) and verts.is_cuda and joints.shape == (B, 21, 3)
    assert torch.equal(fitter(V).mesh(r), verts)      # a fitter that has not fitted yet poses a result as well
    # the tips are vertices of that mesh
    tips_at = [JOINT_MAP.index(16 + j) for j in range(5)]
    assert torch.equal(joints[:, tips_at], verts[:, list(m.tips)])
    faces = np.load(os.path.join(ROOT, "tests", "golden", "hand_mesh.npz"))["f"]
    out = MeshRenderer(faces, V, size=(64, 64), device=DEV).render(verts, out66[:, :3].contiguous())
    assert out["rgb"].shape == (B, 64, 64, 3) and out["mask"].shape == (B, 64, 64) and bool(out["mask"].any())
    a = project_outputs(torch.cat([out66[:, :3], joints.reshape(B, 63)], dim=1), 64, 64).cpu().double()
    b = project_outputs(out66, 64, 64).cpu().double()
    rms_px = ((a - b) ** 2).sum(2).mean(1).sqrt().numpy()
    gate_px = (2 * want + 1e-5) * cam[:, 0].double().numpy() * 32.0
    print("projected joint RMS, pixels:", rms_px, "gate", gate_px)
    assert (rms_px <= gate_px).all()
