"""Exact-sum data for the bf16x3 split kernels (csrc/split.h), and a numpy emulation of the split for the self-tests.

If every product a_i*b_i of a dot product is an integer multiple of a power of two q and sum|a_i*b_i| <= 2^24 q, every
partial sum, in any order and any grouping (inside an MFMA, across split-K slices, with a bias or an accumulate base that
is itself a multiple of q and counted in the bound), is an fp32 number: the fp32 result IS the fp64 one.  Three designs
make each of the six terms hi.hi, hi.mid, mid.hi, hi.lo, mid.mid, lo.hi carry part of that answer:

  A   left  +-(1 + 2^-9 + 2^-17) 2^e, e in {0, 1}  (hi, mid and lo all non-zero)
      right +-2^e', e' in {-1, 0, 1}, sparse       (hi only)                          -> hi.hi, mid.hi, lo.hi
  B   A with the operands swapped                                                      -> hi.hi, hi.mid, hi.lo
  C   both  +-(1 + 2^-9), sparse                    (hi and mid)                       -> hi.hi, hi.mid, mid.hi, mid.mid

The terms a correct kernel drops (mid.lo, lo.mid, lo.lo) are identically zero in all three, and every product is a
multiple of Q = 2^-18.  No GPU here: the GPU cases are tests/test_gpu_exact_split.py, the self-tests test_exact_split.py.
"""
import numpy as np
import torch

from scat_amd import synth

Q = 2.0 ** -18                 # every product of the three designs is a multiple of this
MAX_K = 2016                   # longest reduction of a GPU case (the any-order self-test runs at this length)
TERMS = ("hi.hi", "hi.mid", "mid.hi", "hi.lo", "mid.mid", "lo.hi")
DESIGNS = ("A", "B", "C")
_PIECES = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))        # TERMS as (piece of a, piece of b)
DENSE3 = np.float32(1.0 + 2.0 ** -9 + 2.0 ** -17)
DENSE2 = np.float32(1.0 + 2.0 ** -9)
# non-zero products a builder starts from in the longest dot product of a case: the mean of |product| is 1.75 in A and B
# (1 in C), so 36 (64) of them sum to the 64 the bound allows on average; the thinning loop takes it down from there to
# the densest data that meets the bound in every output, which is what feeds the most outputs
_START = {"A": 36.0, "B": 36.0, "C": 64.0}


# ---------------------------------------------------------------- split.h in numpy

def bf16_rn(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32: pk_bf16 of split.h"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def split3(a):
    """a -> (hi, mid, lo): hi = bf16(a), mid = bf16(a - hi), lo = bf16(a - hi - mid), fp32 subtractions"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    hi = bf16_rn(a)
    r = a - hi
    mid = bf16_rn(r)
    lo = bf16_rn(r - mid)
    return hi, mid, lo


def six_term(a, b, drop=None):
    """a[M, K] @ b[K, N] as the six bf16 terms of mfma_split, each accumulated in fp64 (so exact wherever the bound
    holds); drop = index into TERMS of one term to leave out.  Returns fp64."""
    pa, pb = split3(a), split3(b)
    out = np.zeros((a.shape[0], b.shape[1]), dtype=np.float64)
    for n, (i, j) in enumerate(_PIECES):
        if n != drop:
            out += pa[i].astype(np.float64) @ pb[j].astype(np.float64)
    return out


# ---------------------------------------------------------------- the three designs

def _u(seed, name, shape):
    return synth.uniform(seed, name, shape, 0.0, 1.0)


def _sign(seed, name, shape):
    return np.where(_u(seed, name + ".sign", shape) < 0.5, np.float32(-1.0), np.float32(1.0))


def _dense3(seed, name, shape):
    e = np.where(_u(seed, name + ".e", shape) < 0.5, np.float32(1.0), np.float32(2.0))
    return _sign(seed, name, shape) * DENSE3 * e


def _pow2(seed, name, shape, density):
    e = np.exp2(np.floor(_u(seed, name + ".e", shape) * 3.0) - 1.0).astype(np.float32)
    return np.where(_u(seed, name + ".keep", shape) < density, _sign(seed, name, shape) * e, np.float32(0.0))


def _dense2(seed, name, shape, density):
    return np.where(_u(seed, name + ".keep", shape) < density, _sign(seed, name, shape) * DENSE2, np.float32(0.0))


def design(which, left_shape, right_shape, seed, density, right_weight=None):
    """(left, right) of design A, B or C as fp32 tensors; ``density`` = share of non-zero products (the sparse operand's
    density in A and B, the product of the two in C).  right_weight (broadcast to right_shape): relative density of the
    elements of the right operand where it is a sparse one, for reductions whose length depends on the element (the
    parity classes of a stride-2 data gradient take one, two or four taps of the filter).  The uniform draws do not
    depend on the density, so a lower density keeps a subset of the non-zero elements of a higher one."""
    density = min(1.0, density)
    rw = 1.0 if right_weight is None else np.broadcast_to(np.asarray(right_weight, dtype=np.float64), right_shape)
    if which == "A":
        l, r = _dense3(seed, "l", left_shape), _pow2(seed, "r", right_shape, density * rw)
    elif which == "B":
        l, r = _pow2(seed, "l", left_shape, density), _dense3(seed, "r", right_shape)
    else:
        assert which == "C", which
        l, r = _dense2(seed, "l", left_shape, density ** 0.5), _dense2(seed, "r", right_shape, density ** 0.5 * rw)
    return torch.from_numpy(l.astype(np.float32)), torch.from_numpy(r.astype(np.float32))


def exact_sum_ok(abs_products_sum, q=Q):
    return float(torch.as_tensor(abs_products_sum).max()) <= 2.0 ** 24 * q


def assert_exact_sum(abs_products_sum, q=Q):
    """abs_products_sum: sum|a||b| (+ |bias|, + |base|) of every output, from the same torch op in fp64"""
    m = float(torch.as_tensor(abs_products_sum).max())
    assert m <= 2.0 ** 24 * q, "sum|a b| = %g exceeds 2^24 q = %g: fp32 accumulation is not exact" % (m, 2.0 ** 24 * q)


def fed_share(abs_products_sum, reachable=None):
    """share of the outputs that receive at least one non-zero product; reachable: the outputs the operation can feed at
    all (default: every one) — the stride-2 data gradient of a 1x1 convolution leaves three pixels of four untouched"""
    fed = torch.as_tensor(abs_products_sum) > 0
    if reachable is None:
        return float(fed.double().mean())
    reachable = torch.as_tensor(reachable).bool()
    assert not bool((fed & ~reachable).any())
    return float(fed[reachable].double().mean())


def build(which, left_shape, right_shape, seed, terms, abs_sum, extra=0.0, q=Q, right_weight=None):
    """Design ``which`` for one case.  terms: products in the longest dot product of the case (halved by the caller
    where a ReLU removes half of an operand); abs_sum(left, right) -> fp64 sum|a||b| of every output; extra: max |bias| +
    max |base| added to the result; right_weight: see design().  Starts at the density that gives _START non-zero products and thins by 0.9 until
    the bound holds.  Returns (left, right, abs_products_sum)."""
    assert terms <= MAX_K, (terms, MAX_K)
    density = min(1.0, _START[which] / terms)
    for _ in range(60):
        l, r = design(which, left_shape, right_shape, seed, density, right_weight)
        s = abs_sum(l, r)
        if exact_sum_ok(s + extra, q):
            assert_exact_sum(s + extra, q)
            return l, r, s
        density *= 0.9
    raise AssertionError("design %s does not meet the exact-sum bound at any density" % which)


def small_ints(seed, name, shape, top=2):
    """+-{1..top}: a bias or an accumulate base (multiples of q; the caller counts ``top`` in the bound)"""
    v = np.floor(_u(seed, name + ".v", shape) * top) + 1.0
    return torch.from_numpy((_sign(seed, name, shape) * v).astype(np.float32))


def pow2_scale(seed, name, n):
    """per-channel {1/2, 1, 2}: scaling by these is exact"""
    return torch.from_numpy(np.exp2(np.floor(_u(seed, name, (n,)) * 3.0) - 1.0).astype(np.float32))


def bnb_coef(seed, name, n):
    """[ca | cb | cc] with ca in {+-1, +-2}, cb = cc = 0: the folded BatchNorm backward's operand ca*g + cb*z + cc = ca*g"""
    ca = _sign(seed, name, (n,)) * np.where(_u(seed, name + ".m", (n,)) < 0.5, np.float32(1.0), np.float32(2.0))
    return torch.from_numpy(np.stack([ca, np.zeros_like(ca), np.zeros_like(ca)]).astype(np.float32))


def is_exact(got, ref64):
    """the comparison of every exact-sum case: bit-for-bit the fp64 answer, no tolerance"""
    got = torch.as_tensor(got).detach().cpu().double()
    ref64 = torch.as_tensor(ref64)
    assert ref64.dtype == torch.float64 and got.shape == ref64.shape, (ref64.dtype, got.shape, ref64.shape)
    return torch.equal(got, ref64)
