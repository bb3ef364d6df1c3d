"""The guard arena (tests/_guard.py) proves itself on CPU memory: the mistakes are planted by Python code, nothing on a
GPU is made to misbehave.  Plus the completeness test: every pointer-taking entry point of include/scat_hip.h is either
exercised by a case of tests/test_gpu_guard.py or exempted by name with a reason."""
import re

import pytest
import torch

import _guard
from _guard import Arena, GuardError, TorchProxy

SMALL = dict(nbytes=4 << 20)   # 1 MiB at each end + room for a few tensors with 64 KiB between them


def _nan_bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("fill", ["nan", "big"])
def test_skew_gives_the_promised_pointer_residues(fill):
    a = Arena("cpu", fill, **SMALL)
    for dtype in (torch.float32, torch.uint8, torch.int8, torch.int32):
        for skew in range(4):
            v = a.place((3, 5), skew=skew, dtype=dtype)
            assert v.data_ptr() % 16 == 4 * skew and v.is_contiguous() and v.dtype == dtype and tuple(v.shape) == (3, 5)
    src = torch.arange(7, dtype=torch.float32)
    v = a.place(src, skew=3)
    assert v.data_ptr() % 16 == 12 and torch.equal(v, src)
    with pytest.raises(ValueError):
        a.place((4,), skew=4)
    a.check()


def test_layout_keeps_the_promised_guard_bands():
    a = Arena("cpu", "nan", **SMALL)
    a.place((1000,), skew=1)
    a.place((17,), dtype=torch.uint8, skew=2)
    a.place((3, 3), skew=0, out=True)
    bands = a.bands()
    assert bands[0][1] - bands[0][0] >= 1 << 20 and bands[-1][1] - bands[-1][0] >= 1 << 20
    assert all(b - s >= 64 << 10 for s, b, _, _ in bands[1:-1])
    base = a.buf.data_ptr()
    for s in a.slots:       # every view lies inside the one allocation, in order, not overlapping
        assert base + s.off == s.view.data_ptr()
    with pytest.raises(AssertionError):
        Arena("cpu", "nan", nbytes=4 << 20, min_gap=512)      # the bands can not be configured away


def test_guard_pattern_is_a_quiet_nan_with_a_payload():
    a = Arena("cpu", "nan", **SMALL)
    f = a.buf.view(torch.float32)
    assert bool(torch.isnan(f).all())
    assert int(a.buf.view(torch.int32)[12345]) == 0x7FC5CA7E and (0x7FC5CA7E >> 22) & 0x1FF == 0x1FF
    b = Arena("cpu", "big", **SMALL)
    assert float(b.buf.view(torch.float32)[777]) == pytest.approx(1e30, rel=1e-6)
    y = b.place((8,), out=True)
    assert bool(torch.isnan(y).all()), "output bodies hold the NaN under either fill"


@pytest.mark.parametrize("fill", ["nan", "big"])
@pytest.mark.parametrize("skew", [0, 1, 3])
def test_a_clean_kernel_passes(fill, skew):
    a = Arena("cpu", fill, **SMALL)
    x = a.place(torch.randn(5, 33), skew=skew, name="x")
    y = a.place((5, 33), skew=skew, name="y", out=True)
    acc = a.place(torch.ones(5, 33), skew=skew, name="acc", out=True)
    m = a.place((41,), dtype=torch.uint8, skew=skew, name="mask", out=True)
    torch.mul(x, 2.0, out=y)
    acc += x
    m.copy_((torch.arange(41) % 2).to(torch.uint8))
    a.check()
    assert torch.equal(y, x * 2)


@pytest.mark.parametrize("where,expect", [("before", "guard BEFORE 'y' damaged: 4 bytes, first at -4 and last at -1 bytes"),
                                          ("after", "guard AFTER 'y' damaged: 4 bytes, first at +0 and last at +3 bytes"),
                                          # the last float of the band behind y is nearer to z: named by z
                                          ("far", "guard BEFORE 'z' damaged: 4 bytes, first at -4 and last at -1 bytes")])
@pytest.mark.parametrize("skew", [0, 1])
def test_one_element_outside_the_body_is_named(where, expect, skew):
    a = Arena("cpu", "nan", **SMALL)
    a.place(torch.randn(64), skew=skew, name="x")
    y = a.place((6, 10), skew=skew, name="y", out=True)
    a.place(torch.randn(64), skew=skew, name="z")
    y.fill_(1.0)
    a.check()
    slot = a.slots[1]
    pos = {"before": slot.off - 4, "after": slot.off + slot.nbytes, "far": a.slots[2].off - 4}[where]
    a.buf[pos:pos + 4].view(torch.float32)[0] = 3.0
    with pytest.raises(GuardError) as e:
        a.check()
    assert expect in str(e.value), str(e.value)
    # a single damaged BYTE is enough (the comparison is bit for bit, not a float compare)
    a2 = Arena("cpu", "nan", **SMALL)
    y2 = a2.place((4,), name="y", out=True)
    y2.zero_()
    a2.buf[a2.slots[0].off + 16] ^= 1
    with pytest.raises(GuardError, match=r"AFTER 'y' damaged: 1 bytes, first at \+0 and last at \+0"):
        a2.check()


def test_damage_at_both_ends_of_the_arena_is_seen():
    a = Arena("cpu", "nan", **SMALL)
    y = a.place((4,), name="y", out=True)
    y.zero_()
    a.buf[0] = 0
    with pytest.raises(GuardError, match="BEFORE 'y'"):
        a.check()
    a.reset()
    y = a.place((4,), name="y", out=True)
    y.zero_()
    a.buf[a.nbytes - 1] = 0
    with pytest.raises(GuardError, match="AFTER 'y'"):
        a.check()


def test_replacing_a_guard_nan_by_another_nan_is_damage():
    """a float compare would call NaN != NaN everywhere, or an isnan() test would accept any NaN: the bits decide"""
    a = Arena("cpu", "nan", **SMALL)
    y = a.place((4,), name="y", out=True)
    y.zero_()
    pos = a.slots[0].off + 16
    a.buf[pos:pos + 4].view(torch.float32)[0] = float("nan")
    with pytest.raises(GuardError, match="AFTER 'y'"):
        a.check()


def test_an_unwritten_output_element_is_reported():
    a = Arena("cpu", "nan", **SMALL)
    x = a.place(torch.randn(4, 9), name="x")
    y = a.place((4, 9), name="y", out=True)
    y.view(-1)[:35].copy_(x.view(-1)[:35])          # the "kernel" forgets the last element
    with pytest.raises(GuardError, match=r"output 'y': 1 of 36 elements not finite, first at flat index 35 \(1 still hold"):
        a.check()


def test_a_guard_nan_that_bleeds_into_an_output_is_reported():
    """a "kernel" that loads one element past its input and masks by multiplying with zero instead of selecting"""
    for fill in ("nan", "big"):
        a = Arena("cpu", fill, **SMALL)
        x = a.place(torch.randn(8), name="x")
        y = a.place((8,), name="y", out=True)
        over = a.buf[a.slots[0].off: a.slots[0].off + 36].view(torch.float32)      # 9 floats: one past the end
        if fill == "nan":
            torch.add(x, over[1:9] * 0.0, out=y)
            with pytest.raises(GuardError, match=r"output 'y': 1 of 8 elements not finite, first at flat index 7"):
                a.check()
        else:
            # relu(v * scale + shift) of the poisoned lane: fmaxf would swallow a NaN, +1e30 survives and overflows the sum
            torch.add(x, torch.relu(over[1:9] * 1e9), out=y)
            with pytest.raises(GuardError, match=r"output 'y': 1 of 8 elements not finite.*1 other NaN/Inf"):
                a.check()


def test_scratch_bodies_are_not_asked_to_be_finite_but_are_guarded():
    a = Arena("cpu", "nan", **SMALL)
    ws = a.place((256,), dtype=torch.uint8, name="ws", out=True)
    a.check()
    a.buf[a.slots[0].off - 1] = 7
    with pytest.raises(GuardError, match="BEFORE 'ws'"):
        a.check()


def test_torch_proxy_carves_allocations_out_of_the_arena():
    a = Arena("cpu", "nan", **SMALL)
    p = TorchProxy(a, skew=1)
    lo, hi = a.buf.data_ptr(), a.buf.data_ptr() + a.nbytes
    e = p.empty((3, 4), dtype=torch.float32, device="cpu")
    l = p.empty_like(torch.zeros(5, dtype=torch.int8))
    z = p.zeros((7,), dtype=torch.float32, device="cpu")
    f = p.full((2, 2), 3.0, dtype=torch.float32, device="cpu")
    v = p.empty(6, dtype=torch.uint8, device="cpu")
    for t in (e, l, z, f, v):
        assert lo <= t.data_ptr() < hi and t.data_ptr() % 16 == 4
    assert l.dtype == torch.int8 and bool((z == 0).all()) and bool((f == 3).all()) and bool(torch.isnan(e).all())
    with p.scratch():
        w = p.empty(1 << 12, dtype=torch.uint8, device="cpu")
    assert w.data_ptr() % 16 == 0 and lo <= w.data_ptr() < hi
    assert p.float32 is torch.float32 and p.cuda is torch.cuda        # everything else is torch's own
    with pytest.raises(GuardError, match="output 'empty0'"):         # e was never written
        a.check()


# ------------------------------------------------------------------ completeness of tests/test_gpu_guard.py

EXEMPT_KINDS = ("returns a string", "host-side state only", "diagnostic build only")


def test_every_pointer_taking_entry_point_is_exercised_or_exempted():
    import test_gpu_guard as G

    protos = _guard.header_pointer_entry_points()
    assert len(protos) > 60, "the header parse lost its prototypes"
    covered = {}
    for case in G.CASES:
        assert case.syms, f"case {case.name} names no entry point"
        for s in case.syms:
            covered.setdefault(s, []).append(case.name)
    unknown = sorted((set(covered) | set(G.EXEMPT)) - set(protos))
    assert not unknown, f"not pointer-taking entry points of include/scat_hip.h: {unknown}"
    both = sorted(set(covered) & set(G.EXEMPT))
    assert not both, f"both exercised and exempted: {both}"
    missing = sorted(set(protos) - set(covered) - set(G.EXEMPT))
    assert not missing, f"pointer-taking entry points neither exercised nor exempted: {missing}"
    for name, reason in G.EXEMPT.items():
        assert isinstance(reason, str) and "\n" not in reason and any(k in reason for k in EXEMPT_KINDS), (name, reason)
    assert len(G.EXEMPT) <= 0.15 * len(protos), f"{len(G.EXEMPT)} exemptions of {len(protos)} entry points: more than 15 %"


def test_every_case_fixes_its_skew_outcome_and_gate_beforehand():
    import test_gpu_guard as G

    names = [c.name for c in G.CASES]
    assert len(names) == len(set(names))
    for c in G.CASES:
        assert c.gate in (2e-5, 1e-5, 1e-6, 0.0), (c.name, c.gate)           # the gates of tests/test_gpu_ops.py, or bit-exact
        assert set(c.expect) == {"A", "S", "O"} and c.expect["A"] == "compute", c.name
        for pl, e in c.expect.items():
            assert e == "compute" or re.fullmatch(r"SCAT_E_(SHAPE|ARG|WORKSPACE)", e), (c.name, pl, e)
        if not c.direct:
            assert all(e == "compute" for e in c.expect.values()), f"{c.name}: a dispatching wrapper must compute"
