"""Self-tests of the exact-sum data (tests/_exact_split.py) that tests/test_gpu_exact_split.py holds the split kernels to:
the pieces each design puts into the six terms, exactness of fp32 accumulation in any order, which design catches
which missing term, and what the 2e-5 gate of the per-kernel tests sees of a missing term.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact_split as E  # noqa: E402

from oracle.util import rel_err  # noqa: E402
from scat_amd import synth  # noqa: E402

M, N = 48, 40


def _matmul_abs(l, r):
    return l.double().abs() @ r.double().abs()


def _pair(which, K, seed=7):
    """design ``which`` as a [M, K] x [K, N] product that meets the bound"""
    l, r, s = E.build(which, (M, K), (K, N), seed, K, _matmul_abs)
    assert E.fed_share(s) >= 0.99
    return l.numpy(), r.numpy()


def test_bf16_rn_matches_torch():
    x = np.concatenate([synth.normal_like(1, "x", (4096,)), np.float32([1 + 2 ** -8, 1 + 3 * 2.0 ** -8, 0.0, -0.0, 2.0 ** -130]),
                        E.DENSE3 * np.float32([1, -2]), E.DENSE2 * np.float32([1, -1])]).astype(np.float32)
    assert np.array_equal(E.bf16_rn(x), torch.from_numpy(x).bfloat16().float().numpy())
    hi, mid, lo = E.split3(x)
    assert np.array_equal((lo.astype(np.float64) + mid) + hi, x.astype(np.float64))     # 3 x 8 bits hold N(0,1) data


def test_pieces_of_each_design():
    """A: hi, mid and lo non-zero on every non-zero element of the dense operand, the other operand is hi only;
    B: A swapped; C: hi and mid non-zero, lo zero on both.  Hence mid.lo, lo.mid and lo.lo vanish everywhere."""
    for which in E.DESIGNS:
        l, r = _pair(which, 288)
        (lh, lm, ll), (rh, rm, rl) = E.split3(l), E.split3(r)
        assert np.array_equal((ll.astype(np.float64) + lm) + lh, l) and np.array_equal((rl.astype(np.float64) + rm) + rh, r)
        nzl, nzr = l != 0, r != 0
        if which == "A":
            assert nzl.all() and (lh != 0).all() and (lm != 0).all() and (ll != 0).all()
            assert (rm == 0).all() and (rl == 0).all() and 0 < nzr.mean() < 1
        elif which == "B":
            assert nzr.all() and (rh != 0).all() and (rm != 0).all() and (rl != 0).all()
            assert (lm == 0).all() and (ll == 0).all() and 0 < nzl.mean() < 1
        else:
            assert (ll == 0).all() and (rl == 0).all()
            assert ((lm != 0) == nzl).all() and ((rm != 0) == nzr).all() and ((lh != 0) == nzl).all()
        for a, b in ((lm, rl), (ll, rm), (ll, rl)):                                      # the terms split.h drops
            assert not (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)).any()
        prod = l.astype(np.float64)[:, :, None] * r.astype(np.float64)[None, :, :]
        assert np.array_equal(prod / E.Q, np.round(prod / E.Q))                          # every product a multiple of Q


def _fp32_sum(l, r, order, cuts):
    """fp32 accumulation of l @ r: k visited in ``order``, in chunks ending at ``cuts``, chunk sums added in fp32"""
    total = np.zeros((l.shape[0], r.shape[1]), dtype=np.float32)
    lo = 0
    for hi in cuts:
        acc = np.zeros_like(total)
        for k in order[lo:hi]:
            acc = acc + l[:, k, None] * r[None, k, :]
            assert acc.dtype == np.float32
        total = total + acc
        lo = hi
    return total


@pytest.mark.parametrize("which", E.DESIGNS)
def test_any_order_of_fp32_accumulation_is_exact(which):
    """at the longest reduction a GPU case uses: forward order, a permutation of k, and random split-K-like chunks"""
    K = E.MAX_K
    l, r = _pair(which, K)
    ref = l.astype(np.float64) @ r.astype(np.float64)
    rng = np.random.default_rng(3)
    perm = rng.permutation(K)
    cuts = sorted(set(rng.integers(1, K, size=11).tolist())) + [K]
    for order, c in ((np.arange(K), [K]), (perm, [K]), (perm, cuts), (np.arange(K), cuts)):
        assert np.array_equal(_fp32_sum(l, r, order, c).astype(np.float64), ref)
    assert np.array_equal(E.six_term(l, r), ref)                                         # and the six terms are all of it


# which design changes when one term is left out (recorded from six_term on a 48 x 288 x 40 product)
CATCHES = {"hi.hi": "ABC", "hi.mid": "BC", "mid.hi": "AC", "hi.lo": "B", "mid.mid": "C", "lo.hi": "A"}


@pytest.mark.parametrize("n", range(6))
def test_every_term_is_caught_by_some_design(n):
    """The comparison of the GPU cases (E.is_exact: torch.equal against fp64) fed the emulation with one term missing in
    place of a kernel's result: it passes with all six terms and fails in exactly the designs of CATCHES, there on
    nearly every output."""
    caught = ""
    for which in E.DESIGNS:
        l, r = _pair(which, 288)
        ref = torch.from_numpy(l.astype(np.float64) @ r.astype(np.float64))
        assert E.is_exact(torch.from_numpy(E.six_term(l, r).astype(np.float32)), ref)
        got = torch.from_numpy(E.six_term(l, r, drop=n).astype(np.float32))
        if not E.is_exact(got, ref):
            caught += which
            assert float((got.double() != ref).double().mean()) > 0.85
    assert caught == CATCHES[E.TERMS[n]], (E.TERMS[n], caught)


def test_the_2e5_gate_does_not_see_a_missing_small_term():
    """Why the exact cases exist.  The data of test_conv1x1_pointwise at (5, 256, 128, 14, 14) (N(0,1) activations,
    He-scaled weights) as the matmul w[128, 256] @ x[256, 980], through the six-term emulation with one term left out,
    against fp64, in the metric of the per-kernel gate (max|got - ref| / max|ref| < 2e-5):

        all six 4.3e-08 (the rounding of the result to fp32) | without hi.hi 1.0e+00 | hi.mid 1.8e-03 | mid.hi 1.9e-03
        | hi.lo 2.5e-06 | mid.mid 3.4e-06 | lo.hi 2.9e-06

    A kernel that loses hi.lo, mid.mid or lo.hi — 60 to 80 times the error of a correct one — passes the gate with a
    factor of six to spare."""
    B, cin, cout, H = 5, 256, 128, 14
    x = synth.normal_like(70, "x", (B, cin, H, H))
    w = synth.normal_like(71, "w", (cout, cin, 1, 1), std=(2.0 / cin) ** 0.5).reshape(cout, cin)
    xm = np.ascontiguousarray(x.reshape(B, cin, H * H).transpose(1, 0, 2).reshape(cin, B * H * H))
    ref = w.astype(np.float64) @ xm.astype(np.float64)
    errs = {"all": rel_err(E.six_term(w, xm).astype(np.float32), ref)}
    for n, name in enumerate(E.TERMS):
        errs[name] = rel_err(E.six_term(w, xm, drop=n).astype(np.float32), ref)
    print(" | ".join("%s %.1e" % kv for kv in errs.items()))
    assert errs["all"] < 1e-7
    for name in ("hi.hi", "hi.mid", "mid.hi"):
        assert errs[name] > 2e-5, errs               # the gate sees these
    for name in ("hi.lo", "mid.mid", "lo.hi"):
        assert 20 * errs["all"] < errs[name] < 2e-5, errs    # ... and is blind to these
