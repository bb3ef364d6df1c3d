"""The MANO fit to keypoints on a real MI355X (include/scat_mano_fit_kp.h, scat_amd/fit.py) against the fp64 oracle of
tests/_fit_kp_oracle.py and inside guard bands.  Inputs come from tests/_fit_kp_cases.py.

Every gate that compares fp32 with fp64 is 4 x the error of the oracle itself run in fp32 on the CPU against its fp64 run
on the same inputs (E32 below, printed by tools/fit_kp_gates.py), max |a - b| / max |b|: the project's rule for the MANO
gates.  The recovery gates are on joints and reprojections, never on parameters: twist about
a bone, and depth from 2-D alone, are not observable."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_kp_cases as C  # noqa: E402
import _fit_kp_oracle as KO  # noqa: E402
import _fit_oracle as FO  # noqa: E402
from _fit_cases import JOINT_MAP, host_model, recovery_case, step_case  # noqa: E402
from _guard import Arena  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL, HALF = (1 << 62) - 1, C.HALF
STARTS = [("3d", 37, 1), ("3d", 778, 3), ("3d", 37, 65), ("2d", 37, 3), ("2d", 778, 6), ("mirror", 37, 4)]
STEPS = [("both", 37, 6), ("2d", 37, 6), ("gm", 37, 6), ("limits_wide", 37, 6), ("both", 778, 3), ("gm", 37, 65)]
RECOVERY = [("2d", 37), ("both", 37), ("both", 778), ("gm", 37)]
# The oracle in fp32 on the CPU against itself in fp64, max |a - b| / max |b|, as tools/fit_kp_gates.py printed them.
#   start    p of the closed-form start of _fit_kp_cases.start_case(kind, V, B)
#   step     the accepted p after one LM step from near_start on problem(name, V, B) (lambda 1e-2)
#   cost     the oracle's cost function at its own iterate after k iterations of the gm_limits problem, V = 37
#   limits2  p after two iterations of the limits problem (condition (b)'s box), V = 37
E32 = {
    ("start", "3d", 37, 1): 1.898e-08, ("start", "3d", 778, 3): 1.476e-08, ("start", "3d", 37, 65): 7.398e-08,
    ("start", "2d", 37, 3): 3.397e-08, ("start", "2d", 778, 6): 2.872e-08, ("start", "mirror", 37, 4): 5.057e-08,
    ("step", "both", 37, 6): 1.084e-06, ("step", "2d", 37, 6): 2.222e-06, ("step", "gm", 37, 6): 1.252e-06,
    ("step", "limits_wide", 37, 6): 1.183e-06, ("step", "both", 778, 3): 1.223e-06, ("step", "gm", 37, 65): 1.710e-06,
    ("cost", 1): 6.152e-08, ("cost", 2): 2.118e-08, ("cost", 5): 1.078e-07,
    ("cost", 10): 2.141e-07, ("limits2",): 4.174e-07,
}
# scat_mano_fit's own gates (tests/test_gpu_fit.py: 4 x the 3-D oracle's fp32 error), for the agreement test
GATE_FIT = {("step", 37): 4 * 1.507e-06, ("step", 778): 4 * 3.936e-06, ("cost", 1): 4 * 1.149e-07, ("cost", 2): 4 * 1.489e-07,
            ("cost", 5): 4 * 1.732e-07, ("cost", 10): 4 * 2.225e-07}


def model(V):
    m = host_model(V)
    return m if m.device is not None else m.to(DEV)


@pytest.fixture(scope="module", autouse=True)
def device():
    from scat_amd._lib import lib

    lib().scat_check_device()


def kfit(V, pr, free, fc, iters, P0=None, lambda0=1e-2):
    """the entry point as declared, on a Problem of the oracle -> p [B,65], cost [B], accepted [B] on the host"""
    from scat_amd.fit import mano_fit_kp

    d = lambda t: None if t is None else t.float().contiguous().to(DEV)
    B = (pr.T3 if pr.T3 is not None else pr.T2).shape[0]
    p = torch.empty(B, 65, device=DEV) if P0 is None else P0.float().contiguous().to(DEV)
    jm = torch.tensor(pr.joint_map, dtype=torch.int32, device=DEV)
    cost, acc = mano_fit_kp(model(V), d(pr.T3), d(pr.w3), d(pr.T2), d(pr.w2), jm, d(pr.lo), d(pr.hi), p, iters, 0 if P0 is not None else 1,
                            lambda0, pr.w_pose, pr.w_beta, pr.w_limit, pr.sigma3, pr.sigma2, pr.half[0], pr.half[1], free, fc)
    return p.cpu(), cost.cpu(), acc.cpu()


def held(tag, got, want, e32):
    e = KO.rel(got.numpy(), want.numpy())
    print(f"{tag}: {e:.3e} (gate {4 * e32:.3e} = 4 x {e32:.3e})")
    assert torch.isfinite(got).all(), tag
    assert e <= 4 * e32, (tag, e, 4 * e32)


# V = 37: less than one wavefront and odd; V = 778: MANO.  B = 65: more workgroups than one wave of them is wide.
@pytest.mark.parametrize("kind,V,B", STARTS)
def test_start_matches_the_oracle(kind, V, B):
    """init = 1 with everything frozen returns the closed-form start: both branches, the mirrored and the rotated hands"""
    pr, want, _ = C.start_case(kind, V, B)
    p, cost, acc = kfit(V, pr, 0, 0, 1)
    assert acc.tolist() == [0] * B and bool(torch.isfinite(cost).all())
    held(f"start {kind} V {V} B {B}", p, want, E32[("start", kind, V, B)])
    if kind == "mirror":      # samples 2 and 3 took the second candidate: a turn of pi about an axis in the image plane
        ang = p[:, :3].norm(dim=1)
        assert bool((ang[2:] - np.pi).abs().max() < 1e-5) and bool((p[2:, 2].abs() < 1e-5).all())
        assert abs(float(p[1, 2]) - 2.5) < 1e-4 and abs(float(p[0, 2]) - 0.4) < 1e-4


@pytest.mark.parametrize("name,V,B", STEPS)
def test_one_step_matches_the_oracle(name, V, B):
    pr, free, fc = C.problem(name, V, B)
    want, _, acc64 = C.run(name, V, 1, B)
    assert acc64.tolist() == [1] * B
    p, cost, acc = kfit(V, pr, free, fc, 1, C.near_start(V, B))
    assert acc.tolist() == [1] * B
    held(f"one step {name} V {V} B {B}", p, want, E32[("step", name, V, B)])


def test_cost_is_monotone_and_is_the_oracles():
    V, name = 37, "gm_limits"
    pr, free, fc = C.problem(name, V)
    costs = []
    for k in (1, 2, 5, 10):
        p, c, acc = kfit(V, pr, free, fc, k, C.near_start(V))
        assert bool((acc <= k).all()) and bool((acc >= 0).all())
        costs.append(c.double())
        with torch.no_grad():
            want = KO.cost(host_model(V), p.double(), pr)
        held(f"cost after {k} iterations {c.numpy()}", c.double(), want, E32[("cost", k)])
    for a, b in zip(costs, costs[1:]):
        assert bool((b <= a).all())
    assert bool((costs[-1] < costs[0]).all())


def figures(tag, name, V, p, want64):
    """the recovery gates, per sample, no sample left out: 3-D joint RMS <= 2 x the fp64 oracle's + 1e-5 m, reprojection RMS
    <= 2 x the oracle's + 1e-5 m in pixels"""
    g3, g2 = C.recovery_figures(name, V, p)
    w3, w2 = C.recovery_figures(name, V, want64)
    floor = C.px_floor(V)
    for b in range(p.shape[0]):
        s3 = "" if g3 is None else f"3-D {1e3 * g3[b]:.4f} mm (oracle {1e3 * w3[b]:.4f}, gate {1e3 * (2 * w3[b] + 1e-5):.4f}), "
        print(f"{tag} sample {b}: {s3}2-D {g2[b]:.5f} px (oracle {w2[b]:.5f}, gate {2 * w2[b] + floor[b]:.5f})")
    assert torch.isfinite(p).all()
    if g3 is not None:
        assert (g3 <= 2 * w3 + 1e-5).all(), (g3, w3)
    assert (g2 <= 2 * w2 + floor).all(), (g2, w2)
    return g3, g2


@pytest.mark.parametrize("name,V", RECOVERY)
def test_recovers_from_the_near_start(name, V):
    pr, free, fc = C.problem(name, V)
    want = C.run(name, V, 20)[0]
    p, cost, acc = kfit(V, pr, free, fc, 20, C.near_start(V))
    assert bool((acc > 0).all())
    g3, _ = figures(f"{name} V {V}", name, V, p, want)
    if name == "gm":      # condition (a) on the kernel: GM against the kernel's own quadratic fit of the same outliers
        prq, _, _ = C.problem("quad_outliers", V)
        q3, _ = C.recovery_figures("quad_outliers", V, kfit(V, prq, free, fc, 20, C.near_start(V))[0])
        print(f"inlier RMS, mm: GM {1e3 * g3}, quadratic {1e3 * q3}")
        assert (g3 < 0.5 * q3).all()


def test_two_d_only_from_the_closed_form_start():
    """condition (c) on the kernel: 40 iterations halve the start's reprojection RMS on every sample, and more"""
    V = 37
    pr, start, end64 = C.condition_c(V)
    p, cost, acc = kfit(V, pr, C.FREE_2D, 7, 40, lambda0=1e-3)
    got = KO.rms2(host_model(V), p, pr.T2, JOINT_MAP, HALF).numpy()
    print(f"reprojection RMS, px: start {start}, fp64 oracle {end64}, kernel {got}, accepted {acc.tolist()}")
    assert torch.isfinite(p).all() and (got <= 0.5 * start).all()
    assert torch.equal(p[:, 58:62], torch.zeros(6, 4))      # trans and log_scale stayed the gauge they are


def test_limits_hold_the_angles():
    """condition (b) on the kernel, and p after two iterations with limits against the oracle"""
    V = 37
    viol = {}
    for name in ("both", "limits"):
        pr, free, fc = C.problem(name, V)
        p, _, _ = kfit(V, pr, free, fc, 20, C.near_start(V))
        viol[name] = (p[:, 3:48].abs() - C.BOX).clamp_min(0).max(1).values.numpy()
    print(f"largest violation of +-{C.BOX}, rad: with limits {viol['limits']}, without {viol['both']}")
    assert (viol["limits"] < viol["both"]).all()
    pr, free, fc = C.problem("limits", V)
    p, _, acc = kfit(V, pr, free, fc, 2, C.near_start(V))
    want, _, acc64 = C.run("limits", V, 2)
    assert acc.tolist() == acc64.tolist()
    held("two iterations with limits", p, want, E32[("limits2",)])


@pytest.mark.parametrize("V", [37, 778])
def test_agrees_with_the_quadratic_fit(V):
    """no 2-D term, sigma = 0, no limits, free_cam = 0: scat_mano_fit's problem, held to _fit_oracle.lm at scat_mano_fit's
    own gates; the difference to scat_mano_fit's output is printed, not gated (another kernel may contract differently)"""
    from scat_amd.fit import ManoFitter

    cam = torch.tensor([1.0, 0.0, 0.0]).repeat(6, 1)
    T, P1, Ps, c = step_case(V)
    pr = KO.Problem(JOINT_MAP, T3=T, half=HALF)
    p, cost, acc = kfit(V, pr, ALL, 0, 1, torch.cat([P1.float(), cam], 1))
    assert acc.tolist() == [1] * 6 and torch.equal(p[:, 62:], cam)
    e, ec = FO.rel(p[:, :62].numpy(), Ps.numpy()), FO.rel(cost.double().numpy(), c.numpy())
    ref = ManoFitter(model(V), joint_map=JOINT_MAP, lambda0=1e-2).fit(T.to(DEV), init=P1.float().to(DEV), iters=1)
    print(f"V {V}: one step {e:.3e} (gate {GATE_FIT[('step', V)]:.3e}), cost {ec:.3e}; against scat_mano_fit: p "
          f"{FO.rel(p[:, :62].numpy(), ref.p.cpu().numpy()):.3e}, cost {FO.rel(cost.numpy(), ref.cost.cpu().numpy()):.3e}")
    assert e <= GATE_FIT[("step", V)] and ec <= GATE_FIT[("step", V)]
    if V != 778:
        return
    _, T, P0, _, _, _ = recovery_case(V)
    pr = KO.Problem(JOINT_MAP, T3=T, half=HALF)
    f = ManoFitter(model(V), joint_map=JOINT_MAP)
    for k in (1, 2, 5, 10):
        p, cost, acc = kfit(V, pr, ALL, 0, k, lambda0=1e-3)
        with torch.no_grad():
            want = FO.cost(host_model(V), p[:, :62].double(), T.double(), torch.ones(6, 21, dtype=torch.float64), JOINT_MAP, 1e-6, 1e-6)
        e = FO.rel(cost.double().numpy(), want.numpy())
        ref = f.fit(T.to(DEV), iters=k)
        print(f"iters {k}: cost against the oracle's at p {e:.3e} (gate {GATE_FIT[('cost', k)]:.3e}), accepted {acc.tolist()}; against "
              f"scat_mano_fit: p {FO.rel(p[:, :62].numpy(), ref.p.cpu().numpy()):.3e}, accepted {ref.accepted.tolist()}")
        assert e <= GATE_FIT[("cost", k)] and bool((acc <= k).all())
    # its 20 iterations recover the hands as scat_mano_fit's do
    _, _, _, _, want, _ = recovery_case(V)
    p, _, _ = kfit(V, pr, ALL, 0, 20, lambda0=1e-3)
    got = FO.rms(host_model(V), p[:, :62], T, JOINT_MAP).numpy()
    print(f"joint RMS after 20 iterations, mm: {1e3 * got}, oracle {1e3 * want}")
    assert (got <= 2 * want + 1e-5).all()


def test_frozen_unknowns_keep_their_bits():
    from scat_amd.fit import free_mask

    V = 37
    pr, _, _ = C.problem("both", V)
    p0 = C.near_start(V).float()
    free = free_mask(betas=False, log_scale=False)
    p, cost, acc = kfit(V, pr, free, 0b010, 8, p0)      # of the camera only ctx moves
    assert torch.equal(p[:, 48:58], p0[:, 48:58]) and torch.equal(p[:, 61], p0[:, 61])
    assert torch.equal(p[:, 62], p0[:, 62]) and torch.equal(p[:, 64], p0[:, 64])
    assert not torch.equal(p[:, 3:48], p0[:, 3:48]) and not torch.equal(p[:, 63], p0[:, 63]) and bool((acc > 0).all())
    p, _, _ = kfit(V, pr, 0, 0, 8, p0)
    assert torch.equal(p, p0)


def test_zero_weight_joints_do_not_count():
    V = 37
    pr, free, fc = C.problem("gm", V)
    w3, w2 = torch.ones(6, 21), pr.w2.clone()
    w3[:, 4], w3[2, 9], w2[:, 7], w2[1, 0] = 0.0, 0.0, 0.0, 0.0
    far3, far2 = pr.T3.clone(), pr.T2.clone()
    far3[:, 4], far3[2, 9], far2[:, 7], far2[1, 0] = 1e6, -1e6, -1e6, 1e6
    a = kfit(V, pr._replace(w3=w3, w2=w2), free, fc, 6, C.near_start(V))
    b = kfit(V, pr._replace(w3=w3, w2=w2, T3=far3, T2=far2), free, fc, 6, C.near_start(V))
    for x, y in zip(a, b):
        assert x.numpy().tobytes() == y.numpy().tobytes()
    assert bool((a[2] > 0).all())
    a, b = kfit(V, pr._replace(w3=w3, w2=w2), free, fc, 2), kfit(V, pr._replace(w3=w3, w2=w2, T3=far3, T2=far2), free, fc, 2)
    for x, y in zip(a, b):      # the closed-form start as well
        assert x.numpy().tobytes() == y.numpy().tobytes()


@pytest.mark.parametrize("with_init", [False, True])
def test_non_finite_targets_are_not_fitted(with_init):
    V = 37
    pr, free, fc = C.problem("both", V)
    T3, T2 = pr.T3[:4].clone(), pr.T2[:4].clone()
    T2[1, 7, 1], T3[3, 0, 0] = float("nan"), float("inf")
    good = [0, 2]
    P0 = C.near_start(V)[:4].float() if with_init else None
    sub = lambda q, idx: q._replace(T3=q.T3[idx], T2=q.T2[idx], w2=q.w2[idx])
    r = kfit(V, sub(pr, slice(0, 4))._replace(T3=T3, T2=T2), free, fc, 6, P0)
    ref = kfit(V, sub(pr, good), free, fc, 6, None if P0 is None else P0[good])
    assert torch.isfinite(r[0]).all()
    untouched = torch.zeros(65)
    untouched[62] = 1.0
    for b in (1, 3):
        assert float(r[1][b]) == float("inf") and int(r[2][b]) == 0
        assert torch.equal(r[0][b], P0[b] if with_init else untouched)
    for x, y in zip(r, ref):
        assert x[good].numpy().tobytes() == y.numpy().tobytes()


def test_same_call_same_bits():
    V = 778
    pr, free, fc = C.problem("gm_limits", V)
    a, b = kfit(V, pr, free, fc, 12), kfit(V, pr, free, fc, 12)
    for x, y in zip(a, b):
        assert x.numpy().tobytes() == y.numpy().tobytes()
    assert bool((a[2] > 0).all())


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_inside_guard_bands(fill):
    """every operand between poisoned bands at pointer skews 0, 1 and 3 floats, with and without the optional pointers:
    bands intact, every output element written, results bit for bit those of the plain run outside the arena"""
    from scat_amd._lib import lib

    L, V, B = lib(), 37, 3
    m = model(V)
    full, free, fc = C.problem("gm_limits", V, B)
    bare = KO.Problem(JOINT_MAP, T2=full.T2, half=HALF, w_pose=1e-3, w_beta=1e-3)      # no 3-D term, no weights, no limits
    P0 = C.near_start(V, B).float()
    stream = torch.cuda.current_stream().cuda_stream
    plain = []
    for pr, fr in ((full, free), (bare, C.FREE_2D)):
        for init in (1, 0):
            plain += list(kfit(V, pr, fr, 7, 4, None if init else P0, lambda0=1e-3))
    arena = Arena(DEV, fill, nbytes=16 << 20)
    for skew in (0, 1, 3):
        arena.reset()
        mp = [arena.place(t.cpu(), skew, name=n).data_ptr() for n, t in (("blend", m.blend), ("joint_t", m.joint_t), ("joint_s", m.joint_s),
                                                                         ("weights_t", m.weights_t), ("hands_mean", m.hands_mean_d))]
        jm = arena.place(torch.tensor(JOINT_MAP, dtype=torch.int32), skew, name="joint_map")
        outs = []
        for pr, fr in ((full, free), (bare, C.FREE_2D)):
            ptr = lambda t, n: 0 if t is None else arena.place(t.float(), skew, name=n).data_ptr()
            ops = [ptr(pr.T3, "targets3"), ptr(pr.w3, "weights3"), ptr(pr.T2, "targets2"), ptr(pr.w2, "weights2"), jm.data_ptr(),
                   ptr(pr.lo, "pose_lo"), ptr(pr.hi, "pose_hi")]
            for init in (1, 0):
                p = arena.place((B, 65), skew, name="p", out=True) if init else arena.place(P0, skew, name="p0", out=True)
                cost = arena.place((B,), skew, name="cost", out=True)
                acc = arena.place((B,), skew, dtype=torch.int32, name="accepted", out=True)
                L.scat_mano_fit_kp(*mp, *ops, p.data_ptr(), cost.data_ptr(), acc.data_ptr(), B, V, m.parents_packed, *m.tips, 4, init,
                                   1e-3, pr.w_pose, pr.w_beta, pr.w_limit, pr.sigma3, pr.sigma2, HALF[0], HALF[1], fr, 7, stream)
                assert L.scat_last_kernel() == b"mano_fit_kp_v37_i4"
                outs += [p, cost, acc]
        torch.cuda.synchronize()
        arena.check()
        for got, want in zip(outs, plain):
            assert got.cpu().numpy().tobytes() == want.numpy().tobytes(), skew


def test_fit_keypoints_to_projection_to_renderer():
    """the public API: fit_keypoints -> project is project_outputs on (res.cam, joints(res)), lands on the keypoints, and
    mesh(res) renders with res.cam; shape, dtype and device errors are ScatErrors"""
    from scat_amd._lib import ScatError
    from scat_amd.fit import KeypointFitResult, ManoFitter
    from scat_amd.render import MeshRenderer, project_outputs

    V, B = 778, 6
    m = model(V)
    _, T3, T2 = C.truth(V)
    f = ManoFitter(m, joint_map=JOINT_MAP, iters=20)
    r = f.fit_keypoints(joints2d=T2.to(DEV), sigma2=10.0)
    assert isinstance(r, KeypointFitResult) and r.p.shape == (B, 65) and r.cam.shape == (B, 3) and r.scale.shape == (B,)
    assert torch.equal(r.trans, torch.zeros(B, 3, device=DEV)) and torch.equal(r.scale, torch.ones(B, device=DEV))
    uv = f.project(r)
    assert uv.shape == (B, 21, 2)
    assert torch.equal(uv, project_outputs(torch.cat([r.cam, f.joints(r).reshape(B, 63)], 1), 224, 224))
    want = KO.reproject(host_model(V), r.p.cpu().double(), JOINT_MAP, HALF)
    assert float((uv.cpu().double() - want).abs().max()) < 1e-3      # pixels of a 224 frame in fp32
    r0 = f.fit_keypoints(joints2d=T2.to(DEV), free=0, free_cam=0, iters=1)      # everything frozen: the closed-form start
    px = lambda q: ((f.project(q).cpu() - T2) ** 2).sum(2).mean(1).sqrt()
    print("reprojection RMS, px: the closed-form start", px(r0).numpy(), "after 20 iterations", px(r).numpy())
    assert bool((px(r) < px(r0)).all())
    both = f.fit_keypoints(T3.to(DEV), T2.to(DEV), w2=torch.full((B, 21), 1e-6, device=DEV), init=r)
    assert bool((both.accepted > 0).all()) and bool(torch.isfinite(both.p).all())
    only3 = f.fit_keypoints(T3.to(DEV))
    assert torch.equal(only3.cam, torch.tensor([1.0, 0.0, 0.0], device=DEV).repeat(B, 1))      # no 2-D term: the camera stays
    verts = f.mesh(r)
    assert verts.shape == (B, V, 3) and verts.is_cuda
    faces = np.load(os.path.join(ROOT, "tests", "golden", "hand_mesh.npz"))["f"]
    out = MeshRenderer(faces, V, size=(224, 224), device=DEV).render(verts, r.cam.contiguous())
    assert out["rgb"].shape == (B, 224, 224, 3) and bool(out["mask"].any())
    for bad, pat in ((dict(joints2d=T2.to(DEV).double()), "fp32"), (dict(joints2d=T2[:, :20].to(DEV)), "joints2d"),
                     (dict(joints2d=T2.to(DEV), w2=torch.ones(B, 20, device=DEV)), "w2"), (dict(), "joints3d, joints2d or both"),
                     (dict(joints2d=T2.to(DEV), limits=(torch.zeros(44), torch.zeros(45))), "limits"),
                     (dict(joints2d=T2.to(DEV), init=torch.zeros(B, 62, device=DEV)), "start"),
                     (dict(joints2d=T2.to(DEV), iters=65), "iterations"), (dict(joints2d=T2.to(DEV), free_cam=8), "free_cam")):
        with pytest.raises(ScatError, match=pat):
            f.fit_keypoints(**bad)
