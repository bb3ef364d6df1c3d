"""The MANO fit to a track of keypoints in calibrated views on a real MI355X (include_ext/scat_mano_fit_seq_views.h,
scat_amd/fit.py) against the fp64 oracle of tests/_fit_seq_views_oracle.py and inside guard bands.  Inputs come from
tests/_fit_seq_views_cases.py.

Every gate that compares fp32 with fp64 is 4 x the error of the oracle itself run in fp32 on the CPU against its fp64 run
on the same inputs (E32 below, printed by tools/fit_seq_views_gates.py), max |a - b| / max |b|: the project's rule for the
MANO gates.  The recovery gates are on joints and reprojections, never on parameters, and are 4 x what the fp32 oracle
reaches on the same case, per sequence."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_seq_views_cases as C  # noqa: E402
import _fit_seq_views_oracle as QO  # noqa: E402
from _fit_cases import JOINT_MAP, host_model  # noqa: E402
from _guard import Arena  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ALL = C.ALL
# V = 37: less than one wavefront and odd; V = 778: MANO.  S = 65: more workgroups than one wave of them is wide.  T = 1 has
# no neighbour, T = 2 one, T = 3 and 5 a frame with both.  (V, S, T, C, a rig per sequence)
SCAN_START = (37, 3, 5, 2, True)      # a single-view frame, an unseen first frame and a rotation through pi
STARTS = [(37, 1, 1, 2, False), (778, 3, 3, 3, True), (37, 65, 2, 8, False), SCAN_START]
# (problem, V, S, T, C, a rig per sequence); C = 1 has no closed-form start and is entered with init = 0, as every step is
STEPS = [("quad", 37, 3, 2, 2, False), ("gm", 37, 3, 3, 3, True), ("limits", 37, 3, 5, 8, False), ("quad", 37, 1, 1, 1, False),
         ("quad", 778, 3, 3, 3, False), ("gm", 37, 65, 2, 3, True)]
COST = ("gm_limits", 37, 3, 3, 3)
# The oracle in fp32 on the CPU against itself in fp64, max |a - b| / max |b|, as tools/fit_seq_views_gates.py printed them.
#   start    p of the scanned closed-form start of _fit_seq_views_cases.start_case(V, S, T, C, per)
#   step     the accepted p after one LM step from near_start on problem(name, V, S, T, C, per) (lambda 1e-2)
#   cost     the oracle's cost function at its own iterate after k iterations of the gm_limits problem, V = 37, S = T = C = 3
E32 = {
    ("start", 37, 1, 1, 2, False): 6.181e-08, ("start", 778, 3, 3, 3, True): 2.061e-08,
    ("start", 37, 65, 2, 8, False): 4.056e-08, ("start", 37, 3, 5, 2, True): 7.448e-08,
    ("step", "quad", 37, 3, 2, 2, False): 1.397e-06, ("step", "gm", 37, 3, 3, 3, True): 1.805e-06,
    ("step", "limits", 37, 3, 5, 8, False): 2.143e-06, ("step", "quad", 37, 1, 1, 1, False): 3.416e-06,
    ("step", "quad", 778, 3, 3, 3, False): 2.908e-06, ("step", "gm", 37, 65, 2, 3, True): 3.510e-06,
    ("cost", 1): 1.161e-07, ("cost", 2): 4.950e-08, ("cost", 5): 1.056e-07, ("cost", 10): 1.031e-07,
}


def e32_keys():
    return [("start",) + s for s in STARTS] + [("step",) + s for s in STEPS] + [("cost", k) for k in (1, 2, 5, 10)]


def model(V):
    m = host_model(V)
    return m if m.device is not None else m.to(DEV)


@pytest.fixture(scope="module", autouse=True)
def device():
    from scat_amd._lib import lib

    lib().scat_check_device()


d_ = lambda t: None if t is None else t.float().contiguous().to(DEV)


def qfit(V, pr, free, iters, P0=None, lambda0=1e-2):
    """the entry point as declared, on a Problem of the oracle -> p [S,T,62], cost [S], accepted [S] on the host"""
    from scat_amd.fit import mano_fit_seq_views

    S, T = pr.T2.shape[:2]
    p = torch.empty(S, T, 62, device=DEV) if P0 is None else P0.float().contiguous().to(DEV)
    jm = torch.tensor(pr.joint_map, dtype=torch.int32, device=DEV)
    cost, acc = mano_fit_seq_views(model(V), d_(pr.cams), d_(pr.T2), d_(pr.w2), jm, d_(pr.lo), d_(pr.hi), p, iters,
                                   0 if P0 is not None else 1, lambda0, pr.w_pose, pr.w_beta, pr.w_limit, pr.sigma2, pr.z_near,
                                   pr.smooth, free)
    return p.cpu(), cost.cpu(), acc.cpu()


def held(tag, got, want, e32):
    e = QO.rel(got.numpy(), want.numpy())
    print(f"{tag}: {e:.3e} (gate {4 * e32:.3e} = 4 x {e32:.3e})")
    assert torch.isfinite(got).all(), tag
    assert e <= 4 * e32, (tag, e, 4 * e32)


def test_e32_covers_the_cases():
    assert sorted(map(repr, E32)) == sorted(map(repr, e32_keys())) and all(v > 0 for v in E32.values())


@pytest.mark.parametrize("V,S,T,Cn,per", STARTS)
def test_start_matches_the_oracle(V, S, T, Cn, per):
    """init = 1 with everything frozen returns the scanned closed-form start; both forms of cam_batch; in SCAN_START a frame
    that one camera sees and a first frame that none sees take their neighbours', and a rotation through pi is unwrapped"""
    pr, P64, has, _ = C.start_case(V, S, T, Cn, per)
    assert pr.cams.shape[0] == (S if per else 1) and ((V, S, T, Cn, per) != SCAN_START or int((~has).sum()) == 2)
    p, cost, acc = qfit(V, pr, 0, 1)
    assert acc.tolist() == [0] * S and bool(torch.isfinite(cost).all())
    held(f"start V {V} S {S} T {T} C {Cn}", p.double(), P64, E32[("start", V, S, T, Cn, per)])
    with torch.no_grad():      # the start's cost is the oracle's at the returned p
        want = QO.cost(host_model(V), p.double(), pr)
    assert QO.rel(cost.double().numpy(), want.numpy()) < 1e-4


@pytest.mark.parametrize("name,V,S,T,Cn,per", STEPS)
def test_one_step_matches_the_oracle(name, V, S, T, Cn, per):
    pr = C.problem(name, V, S, T, Cn, per)
    want, _, acc64 = C.run(name, V, S, T, Cn, per, 1)
    assert acc64.tolist() == [1] * S
    p, cost, acc = qfit(V, pr, ALL, 1, C.near_start(V, S, T, Cn, per))
    assert acc.tolist() == [1] * S
    held(f"one step {name} V {V} S {S} T {T} C {Cn}", p.double(), want, E32[("step", name, V, S, T, Cn, per)])


def test_cost_is_monotone_and_is_the_oracles():
    name, V, S, T, Cn = COST
    pr = C.problem(name, V, S, T, Cn)
    costs = []
    for k in (1, 2, 5, 10):
        p, c, acc = qfit(V, pr, ALL, k, C.near_start(V, S, T, Cn))
        assert bool((acc <= k).all()) and bool((acc >= 0).all())
        costs.append(c.double())
        with torch.no_grad():
            want = QO.cost(host_model(V), p.double(), pr)
        held(f"cost after {k} iterations {c.numpy()}", c.double(), want, E32[("cost", k)])
    for a, b in zip(costs, costs[1:]):
        assert bool((b <= a).all())
    assert bool((costs[-1] < costs[0]).all())


@pytest.mark.parametrize("name", C.RECOVERY_CASES)
def test_recovers(name):
    """20 iterations on S = 3 tracks of T = 5 frames in C = 3 views: noise-free, pixel noise, one view of outliers under the
    robust loss, a frame that one camera sees and a frame that none sees; joints, reprojections and the gap frame's joints
    within 4 x what the fp32 oracle reaches, per sequence"""
    pr = C.recovery_problem(name)[0]
    P0 = C.recovery_near() if name == "outliers" else None
    p, cost, acc = qfit(C.RECOVERY["V"], pr, ALL, C.RECOVERY["iters"], P0, C.RECOVERY["lambda0"])
    assert bool((acc > 0).all()) and torch.isfinite(p).all()
    g3, g2, gg = C.figures(p, name)
    _, o3, o2, og, _ = C.recovery(name, torch.float32)
    for s in range(p.shape[0]):
        print(f"{name} sequence {s}: joints {1e3 * g3[s]:.6f} mm (fp32 oracle {1e3 * o3[s]:.6f}), pixels {g2[s]:.6f} (fp32 oracle "
              f"{o2[s]:.6f}), frame {C.GAP_FRAME} joints {1e3 * gg[s]:.6f} mm (fp32 oracle {1e3 * og[s]:.6f}); gates 4 x")
    assert (g3 <= 4 * o3).all() and (g2 <= 4 * o2).all() and (gg <= 4 * og).all()


RULES = dict(V=37, S=4, T=3, Cn=3, iters=6)


def rules_problem():
    V, S, T, Cn = (RULES[k] for k in ("V", "S", "T", "Cn"))
    return C.problem("gm", V, S, T, Cn)._replace(w2=torch.ones(S, T, Cn, 21)), C.near_start(V, S, T, Cn).float()


def one_of(pr, s):
    return pr._replace(T2=pr.T2[s:s + 1], w2=pr.w2[s:s + 1], cams=pr.cams if pr.cams.shape[0] == 1 else pr.cams[s:s + 1])


@functools.lru_cache(maxsize=None)
def alone(s, with_init):
    """sequence s of rules_problem() fitted alone"""
    pr, P0 = rules_problem()
    return qfit(RULES["V"], one_of(pr, s), ALL, RULES["iters"], P0[s:s + 1] if with_init else None)


def same_bits(a, b):
    return all(x.numpy().tobytes() == y.numpy().tobytes() for x, y in zip(a, b))


def others_are_as_alone(r, skipped, with_init):
    for s in range(RULES["S"]):
        if s != skipped:
            assert same_bits([x[s:s + 1] for x in r], alone(s, with_init)), s


def not_fitted(r, s, start):
    assert float(r[1][s]) == float("inf") and int(r[2][s]) == 0 and r[0][s].numpy().tobytes() == start.numpy().tobytes()


def test_bits_do_not_depend_on_the_batch_or_the_index():
    pr, P0 = rules_problem()
    for with_init in (True, False):
        r = qfit(RULES["V"], pr, ALL, RULES["iters"], P0 if with_init else None)
        others_are_as_alone(r, -1, with_init)
        assert bool((r[2] > 0).all())
        rev = qfit(RULES["V"], pr._replace(T2=pr.T2.flip(0), w2=pr.w2.flip(0)), ALL, RULES["iters"], P0.flip(0) if with_init else None)
        assert same_bits([x.flip(0) for x in rev], r)
    assert same_bits(qfit(RULES["V"], pr, ALL, RULES["iters"]), qfit(RULES["V"], pr, ALL, RULES["iters"]))


@pytest.mark.parametrize("with_init", [False, True])
def test_a_frame_behind_a_camera_at_the_start_is_not_fitted(with_init):
    """with the caller's start: p untouched; with the closed-form start: the sequence alone is not fitted either and returns
    the same scanned start"""
    pr, P0 = rules_problem()
    V = RULES["V"]
    if with_init:
        P0 = P0.clone()
        cam0 = pr.cams[0, 0]
        P0[1, 2, 58:61] = -1.2 * (cam0[:9].reshape(3, 3).T @ cam0[9:12])      # frame 2's hand 0.1 m behind camera 0's centre
        with torch.no_grad():
            assert float(QO.cost(host_model(V), P0.double(), pr)[1]) == float("inf")
        r = qfit(V, pr, ALL, RULES["iters"], P0)
        not_fitted(r, 1, P0[1])
    else:      # z_near beyond the hand: every start is behind
        far = pr._replace(z_near=5.0)
        r = qfit(V, far, ALL, RULES["iters"])
        for s in range(RULES["S"]):      # triangulation refuses every joint under that z_near: no start, zeros
            not_fitted(r, s, torch.zeros(RULES["T"], 62))
        # the start in front of the cameras, one frame of sequence 1 with one camera that has the hand behind it
        cams = pr.cams.expand(RULES["S"], -1, -1).clone()
        R1 = cams[1, 2, :9].reshape(3, 3)
        centre = -(R1.T @ cams[1, 2, 9:12])
        cams[1, 2, 9:12] = -(R1 @ (-0.2 * centre))      # camera 2 of sequence 1 stands 0.1 m past the hand, looking away
        w2 = pr.w2.clone()
        w2[1, :, 2] = 0.0
        w2[1, 1, 2] = 1.0      # and only frame 1 counts it: the other two views triangulate every frame's start
        turned = pr._replace(cams=cams, w2=w2)
        r = qfit(V, turned, ALL, RULES["iters"])
        P64, _, fitted = QO.start(host_model(V), turned)
        with torch.no_grad():
            assert bool(fitted.all()) and float(QO.cost(host_model(V), P64, turned)[1]) == float("inf")
        assert float(r[1][1]) == float("inf") and int(r[2][1]) == 0 and QO.rel(r[0][1].double().numpy(), P64[1].numpy()) < 1e-5
        assert same_bits([x[1:2] for x in r], qfit(V, one_of(turned, 1), ALL, RULES["iters"]))
        assert bool((r[2][[0, 2, 3]] > 0).all()) and bool(torch.isfinite(r[1][[0, 2, 3]]).all())
        return
    others_are_as_alone(r, 1, True)
    assert bool((r[2][[0, 2, 3]] > 0).all())


@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("what", ["nan_keypoint", "negative_weight", "inf_camera"])
def test_unusable_sequences_are_not_fitted(what, with_init):
    pr, P0 = rules_problem()
    T2, w2, cams = pr.T2.clone(), pr.w2.clone(), pr.cams
    if what == "nan_keypoint":
        T2[1, 2, 2, 7, 1] = float("nan")
    elif what == "negative_weight":
        w2[1, 0, 0, 3] = -1.0
    else:      # a rig per sequence, so that only sequence 1 has the bad camera
        cams = cams.expand(RULES["S"], -1, -1).clone()
        cams[1, 1, 12] = float("inf")
    r = qfit(RULES["V"], pr._replace(T2=T2, w2=w2, cams=cams), ALL, RULES["iters"], P0 if with_init else None)
    not_fitted(r, 1, P0[1] if with_init else torch.zeros(RULES["T"], 62))
    others_are_as_alone(r, 1, with_init)
    assert torch.isfinite(r[0]).all()


def test_a_sequence_without_any_start_is_not_fitted_and_gaps_are_bridged():
    pr, _ = rules_problem()
    w2 = pr.w2.clone()
    w2[2, :, 1:] = 0.0      # sequence 2 is seen by one camera in every frame: nothing is triangulated anywhere
    w2[3, 1] = 0.0          # sequence 3's middle frame is seen by no camera
    w2[0, 0, 1:] = 0.0      # sequence 0's first frame by one
    r = qfit(RULES["V"], pr._replace(w2=w2), ALL, RULES["iters"])
    not_fitted(r, 2, torch.zeros(RULES["T"], 62))
    assert bool((r[2][[0, 1, 3]] > 0).all()) and bool(torch.isfinite(r[1][[0, 1, 3]]).all()) and torch.isfinite(r[0]).all()
    assert same_bits([x[1:2] for x in r], alone(1, False))
    # what no camera sees does not reach the result
    far = pr.T2.clone()
    far[3, 1], far[0, 0, 1:], far[2, :, 1:] = 1e6, -1e6, 3e4
    assert same_bits(r, qfit(RULES["V"], pr._replace(w2=w2, T2=far), ALL, RULES["iters"]))


def test_frozen_unknowns_keep_their_bits():
    from scat_amd.fit import free_mask

    pr, P0 = rules_problem()
    p, cost, acc = qfit(RULES["V"], pr, free_mask(betas=False, log_scale=False), 8, P0)
    assert torch.equal(p[..., 48:58], P0[..., 48:58]) and torch.equal(p[..., 61], P0[..., 61])
    assert not torch.equal(p[..., 3:48], P0[..., 3:48]) and not torch.equal(p[..., 58:61], P0[..., 58:61]) and bool((acc > 0).all())
    p, c0, acc = qfit(RULES["V"], pr, 0, 8, P0)
    assert torch.equal(p, P0) and acc.tolist() == [0] * RULES["S"]
    with torch.no_grad():
        assert QO.rel(c0.double().numpy(), QO.cost(host_model(RULES["V"]), P0.double(), pr).numpy()) < 1e-4


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_inside_guard_bands_and_at_the_exact_workspace(fill):
    """every pointer operand between poisoned bands at pointer skews 0, 1 and 3 floats, the workspace at exactly the queried
    size, with and without the optional pointers, a rig per sequence and one for all: bands intact, every output word
    written, results bit for bit those of the plain run outside the arena"""
    from scat_amd._lib import lib
    from scat_amd.fit import FIT_SEQ_VIEWS_HEADER

    L, V, S, T, Cn = lib(), 37, 3, 3, 3
    ns = L.bind(FIT_SEQ_VIEWS_HEADER)
    m = model(V)
    w2 = torch.ones(S, T, Cn, 21)
    w2[0, 1, 1:], w2[1, 0, 0, 2], w2[2, 0] = 0.0, 0.5, 0.0
    full = C.problem("gm_limits", V, S, T, Cn, True)._replace(w2=w2)
    bare = C.problem("quad", V, S, T, Cn, False)
    P0 = C.near_start(V, S, T, Cn).float()
    stream = torch.cuda.current_stream().cuda_stream
    need = ns.scat_mano_fit_seq_views_ws(S, T)
    plain = []
    for pr in (full, bare):
        for init in (1, 0):
            plain += list(qfit(V, pr, ALL, 4, None if init else P0, lambda0=1e-3))
    arena = Arena(DEV, fill, nbytes=16 << 20)
    for skew in (0, 1, 3):
        arena.reset()
        mp = [arena.place(t.cpu(), skew, name=n).data_ptr() for n, t in (("blend", m.blend), ("joint_t", m.joint_t), ("joint_s", m.joint_s),
                                                                         ("weights_t", m.weights_t), ("hands_mean", m.hands_mean_d))]
        jm = arena.place(torch.tensor(JOINT_MAP, dtype=torch.int32), skew, name="joint_map")
        outs = []
        for pr in (full, bare):
            ptr = lambda t, n: 0 if t is None else arena.place(t.float(), skew, name=n).data_ptr()
            cams, T2, wp = ptr(pr.cams, "cams"), ptr(pr.T2, "targets2"), ptr(pr.w2, "weights2")
            lo, hi = ptr(pr.lo, "pose_lo"), ptr(pr.hi, "pose_hi")
            for init in (1, 0):
                p = arena.place((S, T, 62), skew, name="p", out=True) if init else arena.place(P0, skew, name="p0", out=True)
                cost = arena.place((S,), skew, name="cost", out=True)
                acc = arena.place((S,), skew, dtype=torch.int32, name="accepted", out=True)
                ws = arena.place((need // 4,), 0, name="ws", out=True, finite=False)      # 16-byte aligned, exactly the queried size
                assert ws.data_ptr() % 16 == 0
                ns.scat_mano_fit_seq_views(*mp, cams, pr.cams.shape[0], T2, wp, jm.data_ptr(), lo, hi, p.data_ptr(), cost.data_ptr(),
                                           acc.data_ptr(), ws.data_ptr(), need, S, T, Cn, V, m.parents_packed, *m.tips, 4, init, 1e-3,
                                           pr.w_pose, pr.w_beta, pr.w_limit, pr.sigma2, pr.z_near, *pr.smooth, ALL, stream)
                assert L.scat_last_kernel() == b"mano_fit_seq_views_t3_c3_i4"
                outs += [p, cost, acc]
        torch.cuda.synchronize()
        arena.check()
        for got, want in zip(outs, plain):
            assert got.cpu().numpy().tobytes() == want.numpy().tobytes(), skew


def test_fit_keypoints_views_sequence_end_to_end():
    """the public API: fit_keypoints_views_sequence -> SequenceFitResult that joints(), mesh(), project_views() and
    fit_sequence's init take; triangulate takes the clip"""
    from scat_amd._lib import ScatError
    from scat_amd.fit import Cameras, ManoFitter, SequenceFitResult

    V, S, T, Cn = 778, 3, 5, 3
    m = model(V)
    _, X3, T2, cams = C.truth(V, S, T, Cn, pose_sd=0.5)
    cams = cams.to(DEV)
    cameras = Cameras(cams[:, :, :9].reshape(1, Cn, 3, 3), cams[:, :, 9:12], cams[:, :, 12:16])
    f = ManoFitter(m, joint_map=JOINT_MAP, iters=20, w_pose=1e-2, w_beta=1e-2)
    kp = T2.to(DEV)
    smooth = dict(zip(("rots", "poses", "betas", "trans", "scale"), C.SMOOTH))
    w2 = torch.ones(S, T, Cn, 21, device=DEV)
    w2[:, 2, 1:] = 0.0      # the middle frame is seen by one camera
    r = f.fit_keypoints_views_sequence(kp, cameras, w2=w2, smooth=smooth, sigma2=10.0)
    assert isinstance(r, SequenceFitResult) and r.p.shape == (S, T, 62) and bool((r.accepted > 0).all()) and bool(torch.isfinite(r.cost).all())
    uv = f.project_views(r, cameras)
    px = ((uv - kp) ** 2).sum(4).flatten(1).mean(1).sqrt()
    mm = 1e3 * ((f.joints(r).cpu().double() - X3) ** 2).sum(3).flatten(1).mean(1).sqrt()
    print(f"after 20 iterations: pixel RMS {px.cpu().numpy()}, joint RMS mm {mm.numpy()}")
    assert uv.shape == (S, T, Cn, 21, 2) and bool((px < 0.5).all()) and bool((mm < 0.5).all())
    per = Cameras(*(a.expand(S, *a.shape[1:]).contiguous() for a in cameras))      # a rig per track gives the same pixels
    assert torch.equal(f.project_views(r, per), uv)
    assert f.mesh(r).shape == (S, T, V, 3)
    pts, valid = f.triangulate(kp, cameras)
    assert pts.shape == (S, T, 21, 3) and valid.shape == (S, T, 21) and valid.dtype == torch.bool and bool(valid.all())
    assert float((pts.cpu().double() - X3).abs().max()) < 1e-5
    p4, v4 = f.triangulate(kp[:, 1].contiguous(), cameras)      # the 4-D form is unchanged
    assert torch.equal(p4, pts[:, 1]) and torch.equal(v4, valid[:, 1])
    pw, vw = f.triangulate(kp, per, w2=w2)
    assert not bool(vw[:, 2].any()) and bool(vw[:, [0, 1, 3, 4]].all()) and torch.equal(pw[:, 0], pts[:, 0])
    again = f.fit_keypoints_views_sequence(kp, cameras, smooth=smooth, init=r, iters=2)
    assert bool(torch.isfinite(again.p).all()) and bool((f.fit_sequence(pts, init=r, iters=1).accepted >= 0).all())
    one = Cameras(cameras.R[:, :1], cameras.t[:, :1], cameras.K[:, :1])
    single = f.fit_keypoints_views_sequence(kp[:, :, :1].contiguous(), one, smooth=smooth, init=r, iters=2)
    assert bool(torch.isfinite(single.cost).all())
    for bad, pat in ((dict(joints2d=kp.double()), "fp32"), (dict(joints2d=kp[:, :, :2].contiguous()), "joints2d"),
                     (dict(joints2d=kp[:, 0].contiguous()), "joints2d"), (dict(w2=torch.ones(S, T, Cn, 20, device=DEV)), "weights"),
                     (dict(limits=(torch.zeros(44), torch.zeros(45))), "limits"), (dict(init=torch.zeros(S, T, 65, device=DEV)), "start"),
                     (dict(iters=65), "iterations"), (dict(z_near=0.0), "z_near"), (dict(sigma2=-1.0), "sigma2"),
                     (dict(joints2d=kp[:, :, :1].contiguous(), cameras=one), "one view needs a start"),
                     (dict(cameras=Cameras(cameras.R.expand(2, -1, -1, -1), cameras.t.expand(2, -1, -1), cameras.K.expand(2, -1, -1))),
                      "2 rigs for 3 sequences")):
        with pytest.raises(ScatError, match=pat):
            f.fit_keypoints_views_sequence(**dict(dict(joints2d=kp, cameras=cameras), **bad))
