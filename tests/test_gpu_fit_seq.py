"""The MANO fit to a track of frames on a real MI355X (include/scat_mano_fit_seq.h, ManoFitter.fit_sequence) against the
fp64 oracle of tests/_fit_seq_oracle.py and inside guard bands.  V = 37, S <= 3 and T in {1, 2, 3, 5} unless stated: no
neighbour, ends only, one interior frame, several.

Every gate that compares fp32 with fp64 is 4 x the error of the oracle itself run in fp32 on the CPU against its fp64 run
on the same inputs (E32 below, printed by tools/fit_seq_gates.py), normalised max |a - b| / max |b|: the rule of
tests/test_gpu_fit.py.  None of the figures comes from the kernel."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fit_oracle as FO  # noqa: E402
import _fit_seq_cases as G  # noqa: E402
import _fit_seq_oracle as SO  # noqa: E402
from _fit_cases import JOINT_MAP, host_model  # noqa: E402
from _guard import Arena  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
# The oracle in fp32 on the CPU against itself in fp64, max |a - b| / max |b|, as tools/fit_seq_gates.py printed them.
#   step      the accepted p after one LM step from step_case(V, 2, T) (lambda 1e-2, SMOOTH), key (V, T)
#   cost      the oracle's cost function at its own iterate after k iterations of start_case()
#   start     the oracle's start from zero-pose joints in fp32 against fp64, on start_case() and on pi_case()
E32 = {
    ("step", 37, 1): 1.352e-06, ("step", 37, 2): 2.282e-06, ("step", 37, 3): 9.605e-07, ("step", 37, 5): 7.597e-07,
    ("step", 778, 3): 1.188e-06,
    ("cost", 1): 5.546e-08, ("cost", 2): 6.128e-08, ("cost", 5): 2.078e-07, ("cost", 10): 2.660e-07,
    ("start",): 4.022e-08, ("start_pi",): 6.582e-08,
}
GATE = {k: 4.0 * v for k, v in E32.items()}
GATE_FIT_STEP_37 = 4.0 * 1.507e-06      # tests/test_gpu_fit.py's ("step", 37): ManoFitter.fit's own step gate


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


def held(tag, key, got, want):
    e = FO.rel(got, want)
    print(f"{tag}: {e:.3e} (gate {GATE[key]:.3e} = 4 x {E32[key]:.3e})")
    assert np.isfinite(got).all(), (tag, key)
    assert e <= GATE[key], (tag, key, e, GATE[key])


def same_bits(a, b):
    return all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("V,T", [(37, 1), (37, 2), (37, 3), (37, 5), (778, 3)])
def test_one_step_matches_the_oracle(V, T):
    X, P1, Ps, c = G.step_case(V, 2, T)
    r = fitter(V, lambda0=1e-2).fit_sequence(X.to(DEV), smooth=G.SMOOTH, init=P1.float().to(DEV), iters=1)
    assert r.accepted.tolist() == [1, 1]
    assert r.p.shape == (2, T, 62) and r.rots.shape == (2, T, 3) and r.scale.shape == (2, T) and r.cost.shape == (2,)
    held(f"V {V} T {T}: one step", ("step", V, T), r.p.cpu().numpy(), Ps.numpy())


def test_cost_is_monotone_and_is_the_oracles():
    m = model(37)
    P, X, P0 = G.start_case()
    f = fitter(37)
    costs = []
    for k in (1, 2, 5, 10):
        r = f.fit_sequence(X.to(DEV), smooth=G.SMOOTH, iters=k)
        assert bool((r.accepted <= k).all()) and bool((r.accepted >= 0).all())
        c = r.cost.cpu().double()
        costs.append(c)
        with torch.no_grad():
            want = SO.cost(m, r.p.cpu().double(), X.double(), G.ones(2, 5), JOINT_MAP, f.w_pose, f.w_beta, G.sm(G.SMOOTH))
        held(f"iters {k}: cost {c.numpy()} against the oracle's at p", ("cost", k), c.numpy(), want.numpy())
    for a, b in zip(costs, costs[1:]):
        assert bool((b <= a).all())
    assert bool((costs[-1] < costs[0]).all())


@pytest.mark.parametrize("name", ["start", "start_pi"])
def test_start_matches_the_oracle(name):
    """with every unknown frozen no step can be taken, and init = 1 returns the start itself and its cost"""
    P, X, P0 = G.start_case() if name == "start" else G.pi_case()
    S, T = X.shape[:2]
    f = fitter(37)
    r0 = f.fit_sequence(X.to(DEV), smooth=G.SMOOTH, free=0, iters=1)
    assert r0.accepted.tolist() == [0] * S
    got = r0.p.cpu().numpy()
    held(name, (name,), got, P0.numpy())
    # consecutive rots stay within the oracle's distance (a jump across pi would be about 2 pi), and the fit goes down
    step = lambda Q: np.linalg.norm(np.diff(Q[:, :, :3], axis=1), axis=2)
    assert (step(got.astype(np.float64)) <= step(P0.numpy()) + GATE[(name,)] * np.abs(P0.numpy()).max()).all()
    if name == "start_pi":
        n = np.linalg.norm(got[0, :, :3], axis=1)
        assert n[0] < np.pi < n[-1] and step(got).max() < 0.5
    r = f.fit_sequence(X.to(DEV), smooth=G.SMOOTH, iters=5)
    assert bool((r.cost < r0.cost).all()) and bool((r.accepted > 0).all())


def test_single_frames_without_smoothness_agree_with_the_frame_fit():
    """T = 1 and s_* = 0: the sequence kernel on one-frame sequences and ManoFitter.fit on the same frames, one step
    from the same start; their joints agree to the sum of the two kernels' step gates"""
    X, P1, _, _ = G.step_case(37, 2, 1)
    f = fitter(37, lambda0=1e-2)
    p0 = P1.float().to(DEV)
    a = f.fit_sequence(X.to(DEV), init=p0, iters=1)
    b = f.fit(X[:, 0].to(DEV), init=p0[:, 0], iters=1)
    assert a.accepted.tolist() == [1, 1] and b.accepted.tolist() == [1, 1]
    ja, jb = f.joints(a), f.joints(b)
    assert ja.shape == (2, 1, 21, 3) and f.mesh(a).shape == (2, 1, 37, 3)
    e, gate = FO.rel(ja[:, 0].cpu().numpy(), jb.cpu().numpy()), GATE[("step", 37, 1)] + GATE_FIT_STEP_37
    print(f"T = 1 against the frame fit: joints {e:.3e} (gate {gate:.3e})")
    assert e <= gate


def test_smoothing_lowers_the_acceleration_error():
    """condition (a)'s inputs: the kernel's accel_error against the truth is <= 2 x the fp64 oracle's + 1e-5 m, and below
    that of the kernel's own per-frame fits"""
    m = model(37)
    X, Xn, out = G.noisy_case()
    S, T = Xn.shape[:2]
    f = fitter(37, iters=G.NOISE_ITERS)
    r = f.fit_sequence(Xn.to(DEV), smooth=G.SMOOTH_NOISY)
    pf = f.fit(Xn.reshape(S * T, 21, 3).to(DEV))
    seq = SO.accel(m, r.p.cpu(), JOINT_MAP, X).numpy()
    frame = SO.accel(m, pf.p.cpu().reshape(S, T, 62), JOINT_MAP, X).numpy()
    print(f"accel_error in mm: kernel sequence {1e3 * seq}, fp64 oracle {1e3 * out['seq', 'fp64']}, kernel per frame {1e3 * frame}")
    assert np.isfinite(r.p.cpu().numpy()).all() and bool((r.accepted > 0).all())
    assert (seq <= 2 * out["seq", "fp64"] + 1e-5).all()
    assert (seq < frame).all()


def test_a_frame_without_weight_is_bridged():
    m = model(37)
    X, w, r0, rf = G.gap_case()
    f = fitter(37, iters=G.GAP_ITERS)
    res = []
    for fill in (1e6, -3.25):
        Xg = X.clone()
        Xg[0, G.GAP_AT] = fill
        res.append(f.fit_sequence(Xg.to(DEV), w.to(DEV), smooth=G.SMOOTH))
    assert same_bits(res[0], res[1])      # the frame's targets do not reach the result
    J = f.joints(res[0]).cpu().double()
    rms = float(((J[0, G.GAP_AT] - X[0, G.GAP_AT].double()) ** 2).sum(1).mean().sqrt())
    print(f"bridged frame: {1e3 * rms:.4f} mm from the truth, oracle {1e3 * rf:.4f} mm, start {1e3 * r0:.3f} mm")
    assert rms <= 2 * rf + 1e-5


def test_frozen_unknowns_keep_their_bits_in_every_frame():
    from scat_amd.fit import free_mask

    X, P1, _, _ = G.step_case(37, 2, 3)
    f = fitter(37)
    p0 = P1.float().to(DEV)
    r = f.fit_sequence(X.to(DEV), smooth=G.SMOOTH, init=p0, iters=8, free=free_mask(betas=False, log_scale=False))
    assert torch.equal(r.betas, p0[:, :, 48:58]) and torch.equal(r.p[:, :, 61], p0[:, :, 61])
    assert not torch.equal(r.poses, p0[:, :, 3:48]) and bool((r.accepted > 0).all())


@pytest.mark.parametrize("with_init", [False, True])
def test_a_bad_sequence_is_not_fitted_and_leaves_the_others_alone(with_init):
    X, P1, _, _ = G.step_case(37, 2, 3)
    X3 = torch.cat([X, X[:1]], 0)
    bad = X3.clone()
    bad[1, 2, 7, 1] = float("nan")
    init = torch.cat([P1, P1[:1]], 0).float().to(DEV) if with_init else None
    f = fitter(37, iters=4)
    r = f.fit_sequence(bad.to(DEV), smooth=G.SMOOTH, init=init)
    ref = f.fit_sequence(X3.to(DEV), smooth=G.SMOOTH, init=init)
    assert float(r.cost[1]) == float("inf") and int(r.accepted[1]) == 0
    assert torch.equal(r.p[1], init[1] if with_init else torch.zeros(3, 62, device=DEV))
    assert same_bits([t[[0, 2]] for t in r], [t[[0, 2]] for t in ref]) and bool((ref.accepted > 0).all())


def test_same_call_same_bits_and_no_dependence_on_S():
    P, X, P0 = G.start_case()
    X3 = torch.cat([X, X[:1] + 0.01], 0)
    f = fitter(37, iters=5)
    a, b = f.fit_sequence(X3.to(DEV), smooth=G.SMOOTH), f.fit_sequence(X3.to(DEV), smooth=G.SMOOTH)
    assert same_bits(a, b)
    for s in range(3):
        one = f.fit_sequence(X3[s:s + 1].to(DEV), smooth=G.SMOOTH)
        assert same_bits(one, [t[s:s + 1] for t in a]), s


def test_without_an_accepted_step_p_is_untouched():
    """init = 0 from the truth with every unknown frozen: no step can lower the cost"""
    P, X, P0 = G.start_case()
    f = fitter(37)
    p0 = P.float().to(DEV)
    keep = p0.clone()
    r = f.fit_sequence(X.to(DEV), smooth=G.SMOOTH, init=p0, free=0, iters=3)
    assert r.accepted.tolist() == [0, 0] and torch.equal(r.p, keep) and torch.equal(p0, keep)
    assert bool(torch.isfinite(r.cost).all())


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_inside_guard_bands(fill):
    """every operand, the workspace at exactly the queried size included, between poisoned bands at pointer skews 0, 1
    and 3 floats (the workspace stays 16-byte aligned), with and without weights: bands intact, every output element
    written, results bit for bit those of the plain run"""
    from scat_amd._lib import lib

    L, V, S, T = lib(), 37, 3, 3
    m = model(V)
    X, P1, _, _ = G.step_case(V, 2, T)
    X = torch.cat([X, X[:1]], 0)
    P1 = torch.cat([P1, P1[:1]], 0).float()
    w = torch.full((S, T, 21), 0.75)
    w[2, 1] = 0.0
    s5 = G.sm(G.SMOOTH)
    stream = torch.cuda.current_stream().cuda_stream
    f = fitter(V, iters=3)
    plain = {}
    for ww in (None, w):
        for init in (1, 0):
            r = f.fit_sequence(X.to(DEV), None if ww is None else ww.to(DEV), smooth=G.SMOOTH, init=None if init else P1.to(DEV))
            plain[ww is None, init] = [r.p.cpu().numpy(), r.cost.cpu().numpy(), r.accepted.cpu().numpy()]
    need = int(L.scat_mano_fit_seq_ws(S, T))
    assert need > 0
    arena = Arena(DEV, fill, nbytes=16 << 20)
    for skew in (0, 1, 3):
        for ww in (None, w):
            arena.reset()
            mp = [arena.place(t.cpu(), skew, name=n).data_ptr() for n, t in (
                ("blend", m.blend), ("joint_t", m.joint_t), ("joint_s", m.joint_s), ("weights_t", m.weights_t),
                ("hands_mean", m.hands_mean_d))]
            tg = arena.place(X, skew, name="targets")
            wd = 0 if ww is None else arena.place(ww, skew, name="weights").data_ptr()
            jm = arena.place(torch.tensor(JOINT_MAP, dtype=torch.int32), skew, name="joint_map")
            for init in (1, 0):
                p = arena.place((S, T, 62), skew, name="p", out=True) if init else arena.place(P1, skew, name="p0", out=True)
                cost = arena.place((S,), skew, name="cost", out=True)
                acc = arena.place((S,), skew, dtype=torch.int32, name="accepted", out=True)
                ws = arena.place((need,), 0, dtype=torch.uint8, name="ws", out=True, finite=False)
                L.scat_mano_fit_seq(*mp, tg.data_ptr(), wd, jm.data_ptr(), p.data_ptr(), cost.data_ptr(), acc.data_ptr(),
                                    ws.data_ptr(), need, S, T, V, m.parents_packed, *m.tips, 3, init, 1e-3, 1e-6, 1e-6, *s5,
                                    (1 << 62) - 1, stream)
                assert L.scat_last_kernel() == b"mano_fit_seq_v37_t3_i3"
                torch.cuda.synchronize()
                arena.check()
                for got, want in zip((p, cost, acc), plain[ww is None, init]):
                    assert got.cpu().numpy().tobytes() == want.tobytes(), (skew, ww is None, init)
