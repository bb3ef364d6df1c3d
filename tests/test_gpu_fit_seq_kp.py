"""The MANO fit to a track of keypoints on a real MI355X (include/scat_mano_fit_seq_kp.h,
ManoFitter.fit_keypoints_sequence) against the fp64 oracle of tests/_fit_seq_kp_oracle.py, against the two kernels it
composes, and inside guard bands.  V = 37, S <= 3 and T in {1, 2, 3, 5} unless stated: no neighbour, ends only, one interior
frame, several.

Every gate that compares fp32 with fp64 is 4 x the error of the oracle itself run in fp32 on the CPU against its fp64 run
on the same inputs (E32 below, printed by tools/fit_seq_kp_gates.py), normalised max |a - b| / max |b|: the rule of
tests/test_gpu_fit.py.  None of the figures comes from the kernel."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_kp_oracle as KO  # noqa: E402
import _fit_seq_cases as SC  # noqa: E402
import _fit_seq_kp_cases as G  # noqa: E402
import _fit_seq_kp_oracle as QO  # noqa: E402
from _fit_cases import JOINT_MAP, host_model  # noqa: E402
from _guard import Arena  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
# The oracle in fp32 on the CPU against itself in fp64, max |a - b| / max |b|, as tools/fit_seq_kp_gates.py printed them.
#   step      the accepted p after one LM step from step_case(name, V, 2, T) (lambda 1e-2, SMOOTH), key (name, V, T);
#             "3d" is _fit_seq_cases.step_case's problem through this oracle (the first 62 unknowns)
#   cost      the oracle's cost function at its own iterate after k iterations from its start, cost_e32()
#   start     the oracle's start from zero-pose joints in fp32 against fp64, start_case(kind)
E32 = {
    ("step", "both", 37, 1): 1.153e-06, ("step", "both", 37, 2): 6.576e-07, ("step", "both", 37, 3): 5.476e-07,
    ("step", "both", 37, 5): 7.809e-07, ("step", "2d", 37, 1): 1.523e-06, ("step", "2d", 37, 2): 4.364e-06,
    ("step", "2d", 37, 3): 9.290e-06, ("step", "2d", 37, 5): 5.042e-06, ("step", "robust", 37, 1): 1.437e-06,
    ("step", "robust", 37, 2): 5.730e-07, ("step", "robust", 37, 3): 1.034e-06, ("step", "robust", 37, 5): 5.419e-07,
    ("step", "both", 778, 3): 4.946e-07, ("step", "3d", 37, 3): 1.188e-06,
    ("cost", 1): 2.220e-07, ("cost", 2): 3.094e-07, ("cost", 5): 1.191e-06, ("cost", 10): 1.111e-07,
    ("start", "pi"): 3.256e-08, ("start", "gap0"): 1.329e-07, ("start", "gap_mid"): 4.184e-08,
}
GATE = {k: 4.0 * v for k, v in E32.items()}
GATE_KP_STEP_37 = 4.0 * 1.084e-06       # tests/test_gpu_fit_kp.py's ("step", "both", 37, 6): fit_keypoints' own step gate
GATE_SEQ_STEP_37_3 = 4.0 * 9.605e-07    # tests/test_gpu_fit_seq.py's ("step", 37, 3): fit_sequence's own step gate


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


def d(t):
    return None if t is None else t.float().to(DEV)


def run(f, pr, free, fc, **kw):
    """fit_keypoints_sequence on a Problem of the cases"""
    lim = None if pr.lo is None else (pr.lo, pr.hi)
    return f.fit_keypoints_sequence(d(pr.T3), d(pr.T2), d(pr.w3), d(pr.w2), sigma3=pr.sigma3, sigma2=pr.sigma2, limits=lim,
                                    w_limit=pr.w_limit, free=free, free_cam=fc, **kw)


def held(tag, key, got, want):
    e = QO.rel(got, want)
    print(f"{tag}: {e:.3e} (gate {GATE[key]:.3e} = 4 x {E32[key]:.3e})")
    assert np.isfinite(got).all(), (tag, key)
    assert e <= GATE[key], (tag, key, e, GATE[key])


def same_bits(a, b):
    return all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))


STEPS = [(n, 37, T) for n in ("both", "2d", "robust") for T in (1, 2, 3, 5)] + [("both", 778, 3)]


@pytest.mark.parametrize("name,V,T", STEPS)
def test_one_step_matches_the_oracle(name, V, T):
    pr, free, fc, P1, Ps, c, acc = G.step_case(name, V, 2, T)
    r = run(fitter(V, lambda0=1e-2), pr, free, fc, smooth=G.SMOOTH, init=d(P1), iters=1)
    assert r.accepted.tolist() == [1, 1] == acc.tolist()
    assert r.p.shape == (2, T, 65) and r.rots.shape == (2, T, 3) and r.scale.shape == (2, T) and r.cam.shape == (2, T, 3)
    assert r.cost.shape == (2,)
    held(f"{name} V {V} T {T}: one step", ("step", name, V, T), r.p.cpu().numpy(), Ps.numpy())


def test_cost_is_monotone_and_is_the_oracles():
    m = host_model(37)
    pr, free, fc = G.problem("both", G.COST_SEED, G.COST_S, G.COST_T, 37)
    f = fitter(37)
    costs = []
    for k in G.COST_KS:
        r = run(f, pr, free, fc, smooth=G.SMOOTH, iters=k)
        assert bool((r.accepted <= k).all()) and bool((r.accepted >= 0).all())
        c = r.cost.cpu().double()
        costs.append(c)
        with torch.no_grad():
            want = QO.cost(m, r.p.cpu().double(), pr, QO.sm(G.SMOOTH))
        held(f"iters {k}: cost {c.numpy()} against the oracle's at p", ("cost", k), c.numpy(), want.numpy())
    for a, b in zip(costs, costs[1:]):
        assert bool((b <= a).all())
    assert bool((costs[-1] < costs[0]).all())


@pytest.mark.parametrize("kind", ["pi", "gap0", "gap_mid"])
def test_start_matches_the_oracle(kind):
    """with every unknown and the camera frozen no step can be taken, and init = 1 returns the start itself"""
    pr, S, T, P0, _ = G.start_case(kind)
    f = fitter(37)
    r0 = run(f, pr, 0, 0, smooth=G.SMOOTH, iters=1)
    assert r0.accepted.tolist() == [0] * S
    got = r0.p.cpu().numpy()
    held(kind, ("start", kind), got, P0.numpy())
    if kind == "pi":      # continuous across pi: a jump would be about 2 pi
        n = np.linalg.norm(got[0, :, :3], axis=1)
        assert n[0] < np.pi < n[-1] and np.linalg.norm(np.diff(got[:, :, :3], axis=1), axis=2).max() < 0.5
    if kind == "gap0":
        assert np.array_equal(got[:, 0], got[:, 1])
    if kind == "gap_mid":
        assert np.array_equal(got[:, 2], got[:, 1])
    free, fc = (G.FREE_2D, 7) if pr.T3 is None else (G.ALL, 7)
    r = run(f, pr, free, fc, smooth=G.SMOOTH, iters=5)
    assert bool((r.cost < r0.cost).all()) and bool((r.accepted > 0).all())


def test_single_frames_without_smoothness_agree_with_fit_keypoints():
    """T = 1 and s_* = 0: this kernel on one-frame sequences and fit_keypoints on the same frames, one step from the same
    start; their p agree to the sum of the two kernels' step gates"""
    pr, free, fc, P1, _, _, _ = G.step_case("both", 37, 2, 1)
    f = fitter(37, lambda0=1e-2)
    a = run(f, pr, free, fc, init=d(P1), iters=1)
    b = f.fit_keypoints(d(pr.T3[:, 0]), d(pr.T2[:, 0]), None, d(pr.w2[:, 0]), init=d(P1[:, 0]), iters=1)
    assert a.accepted.tolist() == [1, 1] and b.accepted.tolist() == [1, 1]
    assert f.joints(a).shape == (2, 1, 21, 3) and f.mesh(a).shape == (2, 1, 37, 3) and f.project(a).shape == (2, 1, 21, 2)
    e, gate = QO.rel(a.p[:, 0].cpu().numpy(), b.p.cpu().numpy()), GATE[("step", "both", 37, 1)] + GATE_KP_STEP_37
    ec = QO.rel(a.cost.cpu().numpy(), b.cost.cpu().numpy())
    print(f"T = 1 against fit_keypoints: p {e:.3e}, cost {ec:.3e} (gate {gate:.3e})")
    assert e <= gate and ec <= gate
    assert torch.equal(f.project(a)[:, 0], f.project(KO_result(a)))


def KO_result(a):
    """the frames of a one-frame KeypointSequenceFitResult as a KeypointFitResult"""
    from scat_amd.fit import KeypointFitResult

    return KeypointFitResult(*(t[:, 0] for t in a[:6]), a.cost, a.accepted, a.p[:, 0].contiguous())


def test_3d_only_with_a_frozen_camera_agrees_with_fit_sequence():
    """no 2-D term, sigma = 0, no limits, free_cam = 0: scat_mano_fit_seq's problem; one step from the same start agrees with
    fit_sequence to the sum of the two kernels' step gates"""
    S, T = 2, 3
    X, P1, _, _ = SC.step_case(37, S, T)
    P65 = torch.cat([P1, torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64).expand(S, T, 3)], dim=2)
    f = fitter(37, lambda0=1e-2)
    a = f.fit_keypoints_sequence(joints3d=X.to(DEV), smooth=SC.SMOOTH, init=d(P65), free_cam=0, iters=1)
    b = f.fit_sequence(X.to(DEV), smooth=SC.SMOOTH, init=d(P1), iters=1)
    assert a.accepted.tolist() == [1, 1] == b.accepted.tolist() and torch.equal(a.cam, d(P65)[..., 62:])
    e, gate = QO.rel(a.p[..., :62].cpu().numpy(), b.p.cpu().numpy()), GATE[("step", "3d", 37, 3)] + GATE_SEQ_STEP_37_3
    ec = QO.rel(a.cost.cpu().numpy(), b.cost.cpu().numpy())
    print(f"3-D only against fit_sequence: p {e:.3e}, cost {ec:.3e} (gate {gate:.3e})")
    assert e <= gate and ec <= gate


def test_smoothing_noisy_2d_tracks_lowers_the_acceleration_error():
    """the kernel's accel_error against the truth is <= 2 x the fp64 oracle's + 1e-5 m, and below that of the kernel's own
    per-frame fit_keypoints"""
    m = host_model(37)
    X, T2n, out = G.noisy_case()
    S, T = T2n.shape[:2]
    f = fitter(37, iters=G.NOISE_ITERS)
    r = f.fit_keypoints_sequence(joints2d=T2n.to(DEV), smooth=G.SMOOTH_NOISY)
    pf = f.fit_keypoints(joints2d=T2n.reshape(S * T, 21, 2).to(DEV))
    seq = QO.accel(m, r.p.cpu(), JOINT_MAP, X).numpy()
    frame = QO.accel(m, pf.p.cpu().reshape(S, T, 65), JOINT_MAP, X).numpy()
    print(f"accel_error in mm: kernel sequence {1e3 * seq}, fp64 oracle {1e3 * out['seq', 'fp64']}, kernel per frame {1e3 * frame}")
    assert np.isfinite(r.p.cpu().numpy()).all() and bool((r.accepted > 0).all())
    assert (seq <= 2 * out["seq", "fp64"] + 1e-5).all()
    assert (seq < frame).all()


def test_a_frame_without_weight_is_bridged():
    X, pr, r0, rf = G.gap_case()
    f = fitter(37, iters=G.GAP_ITERS)
    res = []
    for fill3, fill2 in ((1e6, -1e6), (-3.25, 977.0)):
        T3, T2 = pr.T3.clone(), pr.T2.clone()
        T3[0, G.GAP_AT], T2[0, G.GAP_AT] = fill3, fill2
        res.append(run(f, pr._replace(T3=T3, T2=T2), G.ALL, 7, smooth=G.SMOOTH))
    assert same_bits(res[0], res[1])      # the frame's targets do not reach the result
    J = f.joints(res[0]).cpu().double()
    rms = float(((J[0, G.GAP_AT] - X[0, G.GAP_AT].double()) ** 2).sum(1).mean().sqrt())
    print(f"bridged frame: {1e3 * rms:.4f} mm from the truth, oracle {1e3 * rf:.4f} mm, start {1e3 * r0:.3f} mm")
    assert bool((res[0].accepted > 0).all()) and rms <= 2 * rf + 1e-5


def test_outliers_are_down_weighted():
    """the robust tracks: reprojection RMS over the inliers, against the clean targets, <= 2 x the oracle's + 1e-5 m in
    pixels in every frame; without sigma2 the outlier frame is worse"""
    m = host_model(37)
    pr, pq, P1, inl, want = G.robust_case()
    S, T = G.ROBUST_S, G.ROBUST_T
    clean = G.truth(G.STEP_SEED, S, T, 37)[2]
    f = fitter(37, lambda0=1e-2, iters=G.ROBUST_ITERS)
    got = {}
    for name, q in (("gm", pr), ("quad", pq)):
        r = run(f, q, G.ALL, 7, smooth=G.SMOOTH, init=d(P1))
        assert bool((r.accepted > 0).all())
        got[name] = QO.rms2(m, r.p.cpu(), clean, JOINT_MAP, G.HALF, inl).numpy()
    at = G.outlier_frame(T)
    print(f"inlier reprojection RMS in px: kernel {got['gm']}, oracle {want['gm']}; sigma2 = 0 on frame {at}: {got['quad'][:, at]}")
    assert (got["gm"] <= 2 * want["gm"] + G.px_floor(S)[:, None]).all()
    assert (got["quad"][:, at] > got["gm"][:, at]).all()


def test_frozen_unknowns_and_a_frozen_camera_keep_their_bits_in_every_frame():
    from scat_amd.fit import free_mask

    pr, _, _, P1, _, _, _ = G.step_case("both", 37, 2, 3)
    f = fitter(37)
    p0 = d(P1)
    r = run(f, pr, free_mask(betas=False, log_scale=False), 2, smooth=G.SMOOTH, init=p0, iters=8)
    assert torch.equal(r.betas, p0[:, :, 48:58]) and torch.equal(r.p[:, :, 61], p0[:, :, 61])
    assert torch.equal(r.cam[..., 0], p0[..., 62]) and torch.equal(r.cam[..., 2], p0[..., 64])
    assert not torch.equal(r.cam[..., 1], p0[..., 63]) and not torch.equal(r.poses, p0[:, :, 3:48])
    assert bool((r.accepted > 0).all())
    r = run(f, pr, G.ALL, 0, smooth=G.SMOOTH, init=p0, iters=4)
    assert torch.equal(r.cam, p0[..., 62:]) and bool((r.accepted > 0).all())


@pytest.mark.parametrize("with_init", [False, True])
@pytest.mark.parametrize("what", ["nan3", "nan2", "negative"])
def test_a_bad_sequence_is_not_fitted_and_leaves_the_others_alone(what, with_init):
    pr, free, fc, P1, _, _, _ = G.step_case("both", 37, 2, 3)
    cat = lambda t: torch.cat([t, t[:1]], 0)
    ok = pr._replace(T3=cat(pr.T3), T2=cat(pr.T2), w2=cat(pr.w2))
    T3, T2, w2 = ok.T3.clone(), ok.T2.clone(), ok.w2.clone()
    if what == "nan3":
        T3[1, 2, 7, 1] = float("nan")
    elif what == "nan2":
        T2[1, 0, 20, 1] = float("inf")
    else:
        w2[1, 1, 3] = -1e-6
    bad = ok._replace(T3=T3, T2=T2, w2=w2)
    init = d(cat(P1)) if with_init else None
    f = fitter(37, iters=4)
    r = run(f, bad, free, fc, smooth=G.SMOOTH, init=init)
    ref = run(f, ok, free, fc, smooth=G.SMOOTH, init=init)
    assert float(r.cost[1]) == float("inf") and int(r.accepted[1]) == 0
    start = torch.zeros(3, 65, device=DEV)
    start[:, 62] = 1.0
    assert torch.equal(r.p[1], init[1] if with_init else start)
    assert same_bits([t[[0, 2]] for t in r], [t[[0, 2]] for t in ref]) and bool((ref.accepted > 0).all())


def test_same_call_same_bits_and_no_dependence_on_S():
    pr, free, fc = G.problem("robust", G.COST_SEED, 3, 5, 37)
    f = fitter(37, iters=5)
    a, b = run(f, pr, free, fc, smooth=G.SMOOTH), run(f, pr, free, fc, smooth=G.SMOOTH)
    assert same_bits(a, b) and bool((a.accepted > 0).all())
    for s in range(3):
        one = pr._replace(T3=pr.T3[s:s + 1], T2=pr.T2[s:s + 1], w2=pr.w2[s:s + 1])
        assert same_bits(run(f, one, free, fc, smooth=G.SMOOTH), [t[s:s + 1] for t in a]), s


def test_without_an_accepted_step_p_is_untouched():
    """init = 0 and a lambda0 so large that the step cannot lower the fp32 cost: nothing is accepted, p keeps its bits"""
    pr, free, fc, P1, _, _, _ = G.step_case("both", 37, 2, 3)
    P = G.truth(G.STEP_SEED, 2, 3, 37)[0]
    f = fitter(37, lambda0=1e12)
    p0 = d(P)
    keep = p0.clone()
    r = run(f, pr, free, fc, smooth=G.SMOOTH, init=p0, iters=3)
    assert r.accepted.tolist() == [0, 0] and torch.equal(r.p, keep) and torch.equal(p0, keep)
    assert bool(torch.isfinite(r.cost).all())


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_inside_guard_bands(fill):
    """every operand, the workspace at exactly the queried size included, between poisoned bands at pointer skews 0, 1 and
    3 floats (the workspace stays 16-byte aligned), with every optional operand present and with the 2-D term alone: bands
    intact, every output element written, results bit for bit those of the plain run"""
    from scat_amd._lib import lib
    from scat_amd.fit import FIT_SEQ_KP_HEADER

    L, V, S, T = lib(), 37, 3, 3
    ns = L.bind(FIT_SEQ_KP_HEADER)
    m = model(V)
    pr, free, fc, P1, _, _, _ = G.step_case("robust", V, 2, T)
    cat = lambda t: torch.cat([t, t[:1]], 0).float()
    T3, T2, P1 = cat(pr.T3), cat(pr.T2), cat(P1)
    w3, w2 = torch.full((S, T, 21), 0.75), torch.full((S, T, 21), 0.75 * G.W2)
    w3[2, 1], w2[2, 1] = 0.0, 0.0
    full = KO.Problem(JOINT_MAP, T3=T3, w3=w3, T2=T2, w2=w2, lo=pr.lo, hi=pr.hi, w_limit=pr.w_limit, sigma2=pr.sigma2, half=G.HALF)
    only2 = KO.Problem(JOINT_MAP, T2=T2, half=G.HALF)
    s7 = QO.sm(G.SMOOTH)
    stream = torch.cuda.current_stream().cuda_stream
    f = fitter(V, iters=3)
    need = int(ns.scat_mano_fit_seq_kp_ws(S, T))
    assert need > 0
    arena = Arena(DEV, fill, nbytes=16 << 20)
    for q, fr, fcam in ((full, G.ALL, 7), (only2, G.FREE_2D, 7)):
        plain = {}
        for init in (1, 0):
            r = run(f, q, fr, fcam, smooth=G.SMOOTH, init=None if init else P1.to(DEV))
            plain[init] = [r.p.cpu().numpy(), r.cost.cpu().numpy(), r.accepted.cpu().numpy()]
        for skew in (0, 1, 3):
            arena.reset()
            mp = [arena.place(t.cpu(), skew, name=n).data_ptr() for n, t in (
                ("blend", m.blend), ("joint_t", m.joint_t), ("joint_s", m.joint_s), ("weights_t", m.weights_t),
                ("hands_mean", m.hands_mean_d))]
            opt = [0 if t is None else arena.place(t.float(), skew, name=n).data_ptr() for n, t in (
                ("targets3", q.T3), ("weights3", q.w3), ("targets2", q.T2), ("weights2", q.w2))]
            jm = arena.place(torch.tensor(JOINT_MAP, dtype=torch.int32), skew, name="joint_map")
            lim = [0 if t is None else arena.place(t.float(), skew, name=n).data_ptr() for n, t in (("lo", q.lo), ("hi", q.hi))]
            for init in (1, 0):
                p = arena.place((S, T, 65), skew, name="p", out=True) if init else arena.place(P1, skew, name="p0", out=True)
                cost = arena.place((S,), skew, name="cost", out=True)
                acc = arena.place((S,), skew, dtype=torch.int32, name="accepted", out=True)
                ws = arena.place((need,), 0, dtype=torch.uint8, name="ws", out=True, finite=False)
                ns.scat_mano_fit_seq_kp(*mp, *opt, jm.data_ptr(), *lim, p.data_ptr(), cost.data_ptr(), acc.data_ptr(),
                                        ws.data_ptr(), need, S, T, V, m.parents_packed, *m.tips, 3, init, 1e-3, 1e-6, 1e-6,
                                        q.w_limit, q.sigma3, q.sigma2, *G.HALF, *s7, fr, fcam, stream)
                assert L.scat_last_kernel() == b"mano_fit_seq_kp_t3_i3"
                torch.cuda.synchronize()
                arena.check()
                for got, want in zip((p, cost, acc), plain[init]):
                    assert got.cpu().numpy().tobytes() == want.tobytes(), (skew, q.T3 is None, init)
