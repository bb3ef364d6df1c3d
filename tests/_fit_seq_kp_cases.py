"""The fixed inputs of the keypoint-track fit's tests and what the oracle (tests/_fit_seq_kp_oracle.py) makes of them,
computed once per process and read-only: shared by tests/test_fit_seq_kp.py (no GPU), tests/test_gpu_fit_seq_kp.py and
tools/fit_seq_kp_gates.py.  Needs no GPU.  Tracks are _fit_seq_cases.track's, seen by the cameras of _fit_kp_cases.truth (one
camera per sequence, at rest); 2-D targets are _fit_kp_oracle.reproject at HALF, weighted W2 beside a 3-D term."""
import functools

import torch

from scat_amd import synth

import _fit_kp_cases as KC
import _fit_kp_oracle as KO
import _fit_seq_cases as SC
import _fit_seq_kp_oracle as QO
from _fit_cases import JOINT_MAP, T_, host_model

HALF, W2, FREE_2D, ALL = KC.HALF, KC.W2, KC.FREE_2D, (1 << 62) - 1
# the smoothness the step, cost, start and gap cases run with; units in the header.  cam_scale is on a number of 3..5
# whose 2-D rows weigh about 5e-3 (42 rows x W2 x (11 px per unit)^2), cam_trans is in metres like trans
SMOOTH = dict(SC.SMOOTH, cam_scale=1e-3, cam_trans=1e-1)
SIGMA2 = 10.0           # pixels
WIDE_BOX = KC.WIDE_BOX  # the limits of the robust problem: active on a few angles at the step's start, and the step is accepted
W_LIMIT = 1e-2
OUTLIER_PX = 40.0


def frozen(t):
    """tensors of a cached case are shared: nobody writes to them"""
    if isinstance(t, torch.Tensor):
        t = t.detach()
        t.requires_grad_(False)
    return t


@functools.lru_cache(maxsize=None)
def truth(seed, S, T, V):
    """-> P [S,T,65] fp64 (exactly representable in fp32), T3 [S,T,21,3] fp32, T2 [S,T,21,2] fp32 pixels"""
    m = host_model(V)
    P62, X = SC.track(seed, S, T, V)
    cam = KC.truth(V, S)[0][:, 62:65]
    P = torch.cat([P62, cam[:, None, :].expand(S, T, 3)], dim=2).contiguous()
    with torch.no_grad():
        T2 = KO.reproject(m, P.reshape(S * T, 65), JOINT_MAP, HALF).float().reshape(S, T, 21, 2)
    return P, X, T2


def outlier_frame(T):
    return T // 2


@functools.lru_cache(maxsize=None)
def outliers(seed, S, T, V):
    """-> T2 with three keypoints of frame T // 2 of every sequence moved by 40 px in a seeded direction, inl [S,T,21] bool"""
    T2 = truth(seed, S, T, V)[2].clone()
    inl = torch.ones(S, T, 21, dtype=torch.bool)
    d = T_(synth.normal_like(17, "seqkp.out2", (S, KC.OUTLIERS, 2), 1.0)).float()
    for s in range(S):
        for k in range(KC.OUTLIERS):
            j = (4 + 7 * k + 3 * s) % 21
            T2[s, outlier_frame(T), j] += OUTLIER_PX * d[s, k] / d[s, k].norm()
            inl[s, outlier_frame(T), j] = False
    return T2, inl


@functools.lru_cache(maxsize=None)
def problem(name, seed, S, T, V, sigma2=SIGMA2):
    """-> (Problem, free, free_cam): "both", "2d" (2-D only, trans and log_scale frozen), "robust" (both terms, sigma2,
    limits of +-WIDE_BOX with W_LIMIT, three outlier keypoints in frame T // 2), "3d" (scat_mano_fit_seq's problem)"""
    _, T3, T2 = truth(seed, S, T, V)
    w2 = torch.full((S, T, 21), W2)
    if name == "both":
        return KO.Problem(JOINT_MAP, T3=T3, T2=T2, w2=w2, half=HALF), ALL, 7
    if name == "2d":
        return KO.Problem(JOINT_MAP, T2=T2, half=HALF), FREE_2D, 7
    if name == "3d":
        return KO.Problem(JOINT_MAP, T3=T3, half=HALF), ALL, 0
    if name == "robust":
        wide = torch.full((45,), WIDE_BOX)
        return KO.Problem(JOINT_MAP, T3=T3, T2=outliers(seed, S, T, V)[0], w2=w2, sigma2=sigma2, lo=-wide, hi=wide, w_limit=W_LIMIT,
                          half=HALF), ALL, 7
    raise KeyError(name)


STEP_SEED = 21


@functools.lru_cache(maxsize=None)
def near_start(seed, S, T, V):
    """the truth moved by 0.05 x N(0, 1) in the 58 model unknowns of every frame, fp32-exact"""
    P1 = truth(seed, S, T, V)[0].clone()
    P1[:, :, :58] += 0.05 * T_(synth.normal_like(23, "seq.off", (S, T, 58), 1.0)).double()
    return P1.float().double()


@functools.lru_cache(maxsize=None)
def step_case(name, V, S, T, dtype=torch.float64):
    """the oracle's one step in dtype from near_start with lambda = 1e-2 and SMOOTH -> Problem, free, free_cam, the start,
    the step, its cost, accepted"""
    pr, free, fc = problem(name, STEP_SEED, S, T, V)
    P1 = near_start(STEP_SEED, S, T, V)
    Ps, c, acc = QO.lm(host_model(V), pr, P1.to(dtype), 1, QO.sm(SMOOTH), 1e-2, free, fc)
    return pr, free, fc, P1, frozen(Ps), frozen(c), acc


COST_SEED, COST_S, COST_T, COST_KS = 25, 2, 5, (1, 2, 5, 10)


@functools.lru_cache(maxsize=None)
def cost_e32():
    """{k: the oracle's cost function in fp32 against fp64 at its own fp64 iterate after k iterations from its start}, on
    "both" at V = 37, COST_S tracks of COST_T frames"""
    m = host_model(37)
    pr, free, fc = problem("both", COST_SEED, COST_S, COST_T, 37)
    P0 = QO.start(m, pr, COST_S, COST_T)
    trace = QO.lm(m, pr, P0, max(COST_KS), QO.sm(SMOOTH), 1e-3, free, fc, history=True)[4]
    out = {}
    with torch.no_grad():
        for k in COST_KS:
            Pk = trace[k - 1].float()
            out[k] = QO.rel(QO.cost(m, Pk, pr, QO.sm(SMOOTH)).numpy(), QO.cost(m, Pk.double(), pr, QO.sm(SMOOTH)).numpy())
    return out


@functools.lru_cache(maxsize=None)
def start_case(kind):
    """init = 1 at V = 37 -> (Problem, S, T, P64, E32).  "pi": _fit_seq_cases.pi_case's hands (the global rotation crosses the
    angle pi) under a camera, both terms; "gap0": the cost case's tracks from 2-D alone with frame 0 of every sequence at
    weight zero; "gap_mid": the same tracks with both terms and frame 2 at weight zero in both"""
    m = host_model(37)
    if kind == "pi":
        P62, X, _ = SC.pi_case()
        S, T = 1, 5
        P = torch.cat([P62, KC.truth(37, 1)[0][:, None, 62:65].expand(1, 5, 3)], dim=2)
        with torch.no_grad():
            T2 = KO.reproject(m, P.reshape(5, 65), JOINT_MAP, HALF).float().reshape(1, 5, 21, 2)
        pr = KO.Problem(JOINT_MAP, T3=X, T2=T2, w2=torch.full((1, 5, 21), W2), half=HALF)
    else:
        S, T = COST_S, COST_T
        _, T3, T2 = truth(COST_SEED, S, T, 37)
        if kind == "gap0":
            w2 = torch.ones(S, T, 21)
            w2[:, 0] = 0.0
            pr = KO.Problem(JOINT_MAP, T2=T2, w2=w2, half=HALF)
        else:
            w3, w2 = torch.ones(S, T, 21), torch.full((S, T, 21), W2)
            w3[:, 2], w2[:, 2] = 0.0, 0.0
            pr = KO.Problem(JOINT_MAP, T3=T3, w3=w3, T2=T2, w2=w2, half=HALF)
    P64, P32 = QO.start(m, pr, S, T), QO.start(m, pr, S, T, torch.float32)
    return pr, S, T, frozen(P64), QO.rel(P32.numpy(), P64.numpy())


# The noisy 2-D-only tracks: N(0, NOISE_PX) pixels on every keypoint coordinate.  From 2-D alone the rotation out of the
# image plane and the depth-like unknowns are loose in every frame, and the per-frame fits flicker there; the smoothness
# is chosen to outweigh the 2-D data in exactly those.  tests/test_fit_seq_kp.py holds the condition; recorded there.
NOISE_PX, NOISE_T, NOISE_S, NOISE_ITERS, NOISE_SEED = 1.0, 8, 2, 8, 29
SMOOTH_NOISY = dict(rots=6e3, poses=2e3, betas=2e4, cam_scale=1e3, cam_trans=4e5)


def per_frame(m, pr, S, T, iters, dt, free, fc):
    """the frames fitted one by one from their own closed-form start, as ManoFitter.fit_keypoints would: [S,T,65]"""
    fp = QO.flat(pr)
    P0 = KO.start(m, fp, S * T, dt)
    return KO.lm(m, fp, P0, iters, 1e-3, free, fc)[0].reshape(S, T, 65)


@functools.lru_cache(maxsize=None)
def noisy_case():
    """V = 37 -> the true joints [S,T,21,3], the noisy 2-D targets, and the accel_error against the truth of the oracle's
    sequence fit and of its per-frame fits, each in fp64 and in fp32.  Asserts that the sequence fit wins on every track."""
    m, S, T = host_model(37), NOISE_S, NOISE_T
    _, X, T2 = truth(NOISE_SEED, S, T, 37)
    T2n = (T2.double() + NOISE_PX * T_(synth.normal_like(31, "seqkp.noise", (S, T, 21, 2), 1.0)).double()).float()
    pr = KO.Problem(JOINT_MAP, T2=T2n, half=HALF)
    out = {}
    for name, dt in (("fp64", torch.float64), ("fp32", torch.float32)):
        P0 = QO.start(m, pr, S, T, dt)
        Pq = QO.lm(m, pr, P0, NOISE_ITERS, QO.sm(SMOOTH_NOISY), 1e-3, FREE_2D, 7)[0]
        out["seq", name] = QO.accel(m, Pq, JOINT_MAP, X).numpy()
        out["frame", name] = QO.accel(m, per_frame(m, pr, S, T, NOISE_ITERS, dt, FREE_2D, 7), JOINT_MAP, X).numpy()
    assert (out["seq", "fp64"] < out["frame", "fp64"]).all(), out
    return X, frozen(T2n), out


GAP_T, GAP_AT, GAP_ITERS, GAP_SEED = 5, 2, 8, 33


@functools.lru_cache(maxsize=None)
def gap_case():
    """V = 37, S = 1, T = 5, both terms, frame 2 without weight in either -> the true joints, (Problem with its w3, w2), and
    the distance (RMS over the joints) of frame 2 from the truth at the oracle's start and after GAP_ITERS iterations"""
    m = host_model(37)
    _, X, T2 = truth(GAP_SEED, 1, GAP_T, 37)
    w3, w2 = torch.ones(1, GAP_T, 21), torch.full((1, GAP_T, 21), W2)
    w3[0, GAP_AT], w2[0, GAP_AT] = 0.0, 0.0
    pr = KO.Problem(JOINT_MAP, T3=X, w3=w3, T2=T2, w2=w2, half=HALF)
    P0 = QO.start(m, pr, 1, GAP_T)
    Pf = QO.lm(m, pr, P0, GAP_ITERS, QO.sm(SMOOTH), 1e-3, ALL, 7)[0]
    rms = lambda Q: float(((QO.frame_joints(m, Q, JOINT_MAP)[0, GAP_AT] - X[0, GAP_AT].double()) ** 2).sum(1).mean().sqrt())
    return X, pr, rms(P0), rms(Pf)


ROBUST_S, ROBUST_T, ROBUST_ITERS = 2, 5, 10


@functools.lru_cache(maxsize=None)
def robust_case():
    """V = 37, the "robust" tracks of the step case from near_start -> (Problem with sigma2, the same with sigma2 = 0, the
    start, inliers [S,T,21], the reprojection RMS over the inliers against the clean targets [S,T] in pixels of the oracle
    with sigma2 and without).  Asserts that without sigma2 the outlier frame is worse on every track."""
    m, S, T = host_model(37), ROBUST_S, ROBUST_T
    pr, free, fc = problem("robust", STEP_SEED, S, T, 37)
    pq = problem("robust", STEP_SEED, S, T, 37, 0.0)[0]
    P1 = near_start(STEP_SEED, S, T, 37)
    inl = outliers(STEP_SEED, S, T, 37)[1]
    clean = truth(STEP_SEED, S, T, 37)[2]
    r = {}
    for name, q in (("gm", pr), ("quad", pq)):
        Pf = QO.lm(m, q, P1, ROBUST_ITERS, QO.sm(SMOOTH), 1e-2, free, fc)[0]
        r[name] = QO.rms2(m, Pf, clean, JOINT_MAP, HALF, inl).numpy()
    at = outlier_frame(T)
    assert (r["quad"][:, at] > r["gm"][:, at]).all(), r
    return pr, pq, P1, inl, r


def px_floor(S):
    """_fit_kp_cases.px_floor for the S cameras of truth(): 1e-5 m in pixels, per sequence"""
    return KC.px_floor(37, S)
