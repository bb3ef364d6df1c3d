"""The guard arena (tests/_guard.py) proves itself on CPU memory: the mistakes are planted by Python code, nothing on a
GPU is made to misbehave.  Plus the completeness tests: every pointer-taking entry point of include/scat_hip.h is either
exercised by a case of tests/test_gpu_guard.py or exempted by name with a reason, and every entry point that takes a
workspace has its row in that module's WS table, with shapes at which its query returns the bytes written there."""
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


# ------------------------------------------------------------------ the exact-size workspace stand-in

def _overshoot(ws, at):
    """one byte written through ws's own storage at offset ``at`` of it: what a kernel that trusts a larger size does"""
    torch.as_strided(ws, (at + 1,), (1,))[at] = 0


@pytest.mark.parametrize("fill", ["nan", "big"])
@pytest.mark.parametrize("n", [1, 13, 4608, 61936, 592703])
def test_a_workspace_request_gets_exactly_its_bytes_and_one_byte_more_is_seen(n, fill):
    a = Arena("cpu", fill, **SMALL)
    workspace = _guard.exact_workspace(TorchProxy(a, skew=1))
    ws = workspace(n, "cpu", "slot")
    slot = a.slots[-1]
    assert ws.dtype == torch.uint8 and ws.numel() == n == slot.nbytes and slot.view.data_ptr() == ws.data_ptr()
    assert ws.data_ptr() % 16 == 0 and slot.name.startswith("scratch") and slot.out and not slot.finite
    assert a.buf.data_ptr() + slot.off == ws.data_ptr()
    assert torch.equal(ws, a._pattern(slot.off, n, _guard.GUARD_NAN_BITS)), "a workspace starts as the guard NaN"
    a.check()
    _overshoot(ws, n - 1)                    # the last byte it asked for is its own
    a.check()
    _overshoot(ws, n)                        # the first byte it did not ask for is not
    with pytest.raises(GuardError, match=r"guard AFTER 'scratch\d+' damaged: 1 bytes, first at \+0 and last at \+0"):
        a.check()


def test_workspace_requests_are_never_rounded_up_or_shared():
    a = Arena("cpu", "nan", **SMALL)
    workspace = _guard.exact_workspace(TorchProxy(a))
    big, small, again, zero = workspace(9216, "cpu"), workspace(6336, "cpu"), workspace(9216, "cpu"), workspace(0, "cpu", "wt")
    assert [t.numel() for t in (big, small, again, zero)] == [9216, 6336, 9216, 16]       # (0 bytes: 16, a non-null pointer)
    assert len({t.data_ptr() for t in (big, small, again, zero)}) == 4 and len(a.slots) == 4
    assert all(s.nbytes == t.numel() for s, t in zip(a.slots, (big, small, again, zero)))
    assert all(b - s >= 64 << 10 for s, b, _, _ in a.bands()[1:-1])
    # a full arena: the same (slot, stream, bytes) is handed out again, nothing else is
    first = workspace(600 << 10, "cpu", "gg")
    second = workspace(600 << 10, "cpu", "gg")
    third = workspace(600 << 10, "cpu", "gg")
    assert second.data_ptr() != first.data_ptr() and third.data_ptr() == second.data_ptr() and third.numel() == 600 << 10
    for other in ((600 << 10) - 1, (600 << 10) + 1):
        with pytest.raises(MemoryError):
            workspace(other, "cpu", "gg")
    with pytest.raises(MemoryError):
        workspace(600 << 10, "cpu", "another slot")
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


# ------------------------------------------------------------------ the workspace table of tests/test_gpu_guard.py

@pytest.fixture(scope="module")
def L():
    from scat_amd import build
    from scat_amd._lib import lib

    build.build(verbose=False)
    return lib()


def _header_protos():
    from scat_amd._lib import HEADERS, parse_header

    protos = {}
    for h in HEADERS:
        protos.update(parse_header(h))
    return protos


def test_every_entry_point_with_a_workspace_has_its_row():
    import test_gpu_guard as G

    protos = _header_protos()
    with_ws = [n for n, (_, args) in protos.items() if any(an == "ws_bytes" for _, an in args)]
    assert len(with_ws) >= 25, "the header parse lost its prototypes"
    assert all(any(an == "ws" for _, an in protos[n][1]) for n in with_ws)
    assert list(G.WS) == with_ws, (sorted(set(with_ws) - set(G.WS)), sorted(set(G.WS) - set(with_ws)))
    cases = {s for c in G.CASES for s in c.syms}
    for name, row in G.WS.items():
        assert row.align in (4, 8, 16) and row.short in ("reject", "single_pass"), name
        assert row.misaligned in ("SCAT_E_WORKSPACE", "SCAT_E_ARG", "single_pass"), name
        assert (row.short == "single_pass") == (row.misaligned == "single_pass") == (name == "scat_gemm"), name
        assert row.math in (None, 1) and row.nbytes > 0 and (row.shape2 is None) == (row.nbytes2 is None), name
        assert (row.shape2 is None) == (row.branch is None), name
        assert row.where in ("tests/test_cabi.py", "tests/test_eval.py"), name
        # the rows of include/scat_hip.h run inside the arena with exact workspaces; scat_eval.h has tests/test_gpu_eval.py
        assert (name in cases) == (row.where == "tests/test_cabi.py"), name


def test_every_workspace_query_sizes_a_row():
    import test_gpu_guard as G

    queries = {n for n in _header_protos() if n.endswith("_ws")}
    assert len(queries) >= 19
    used = {row.query for row in G.WS.values() if row.query}
    used |= {G._wprep_query(dict(kind=k, Cout=1, Cin=1, KH=1, KW=1))[0] for k in range(6)}      # scat_wprep_jobs: by kind
    assert used == queries, (sorted(queries - used), sorted(used - queries))


def _named(G, L, name, shape):
    return dict(zip([an for _, an in L.protos[name][1]], G.ws_call_args(L, name, shape, 0, 0)))


def test_each_rows_shapes_give_the_bytes_written_in_the_table(L):
    """the byte counts were taken from the host code's own arithmetic; a plan that moves shows here, on the CPU"""
    import test_gpu_guard as G

    for name, row in G.WS.items():
        assert G.ws_query(L, name, _named(G, L, name, row.shape)) == row.nbytes > 0, name
        if row.shape2 is not None:
            assert G.ws_query(L, name, _named(G, L, name, row.shape2)) == row.nbytes2 != row.nbytes, name
        if row.unused and set(row.unused) - {"null"}:
            assert G.ws_query(L, name, _named(G, L, name, dict(row.shape, **row.unused))) == 0, name
    # the branches the table names, from the formulas of the host code
    assert G.WS["scat_bn_bwd"].nbytes == 32 * (4 * 32 + 16) and G.WS["scat_bn_bwd"].nbytes2 == 200 * (11 * 32 + 16)
    assert G.WS["scat_gemm"].nbytes == 3 * 84 * 588 * 4 and G.WS["scat_gemm_group"].nbytes == 2 * (70 * 33 + 3 * 147) * 4
    assert G.WS["scat_colsum_sliced"].nbytes == 79 * 196 * 4
    assert G.WS["scat_layernorm_bwd"].nbytes == (40 + 2) * 196 * 4 and G.WS["scat_layernorm_bwd"].nbytes2 == (21400 + 2 * 79) * 196 * 4
    assert G.WS["scat_conv7x7_s2_wgrad_split"].nbytes == 6 * 64 * 147 * 4            # 22 rows, 4 per workgroup
    assert G.WS["scat_conv7x7_s2_wgrad_split"].nbytes2 == 618 * 64 * 147 * 4         # 3088 rows, 5 per workgroup


class _NoLaunch:
    """the library's queries, and entry points that do nothing: what the recorder notes is looked at without a launch"""

    def __init__(self, real):
        self._real, self.protos = real, real.protos

    def __getattr__(self, name):
        return getattr(self._real, name) if name.endswith("_ws") else (lambda *a: 0)


def test_the_recorder_notes_the_workspace_of_every_row(L):
    import test_gpu_guard as G

    rec = G._Recorder(_NoLaunch(L))
    for name, row in G.WS.items():
        for shape, nbytes in ((row.shape, row.nbytes), (row.shape2, row.nbytes2)):
            if shape is not None:
                getattr(rec, name)(*G.ws_call_args(L, name, shape, 0x7000000, nbytes + 5))
    assert rec.called == set(G.WS)
    for name, row in G.WS.items():
        want = [(row.nbytes + 5, row.nbytes)] + ([(row.nbytes2 + 5, row.nbytes2)] if row.shape2 is not None else [])
        assert rec.ws[name] == want, (name, rec.ws[name], want)
    rec.scat_relu_fwd(16, 32, 4, 0)                                    # (an entry point without a row: only its name)
    assert "scat_relu_fwd" in rec.called and "scat_relu_fwd" not in rec.ws
