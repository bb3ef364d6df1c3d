"""A poisoned arena for kernel tests: operands sit between guard bands of a fixed bit pattern, so that a store outside
an output lands in memory the test owns and is seen, a load outside an input meets NaN (or +1e30) instead of finite
stale data, and an output element the kernel skipped is still NaN afterwards.

    arena = Arena("cuda", fill="nan")
    x = arena.place(x_cpu, skew=1, name="x")                    # input: data_ptr() % 16 == 4
    y = arena.place((B, C, H, W), skew=0, name="y", out=True)   # output: body pre-filled with the guard NaN
    kernel(x, y)
    arena.check()                                               # guards bit for bit, outputs written and finite

TorchProxy stands in for the ``torch`` module global of scat_amd.ops (monkeypatch.setattr(ops, "torch", proxy)): the
outputs the wrappers allocate with empty / empty_like / zeros / full are carved out of the arena too, and
exact_workspace() stands in for ops.workspace with buffers of exactly the requested size.
Plain helper module: no fixtures, no pytest hooks."""
from __future__ import annotations

import contextlib

import numpy as np
import torch

# quiet NaN (exponent all ones, top mantissa bit set) with a payload that is easy to spot in a dump
GUARD_NAN_BITS = 0x7FC5CA7E
BIG = 1e30   # second fill: fmaxf(NaN, 0) = 0 hides an over-read behind a fused ReLU; relu(1e30 * scale + shift) does not
MIN_GAP = 64 << 10     # guard between neighbouring tensors, bytes
END_GAP = 1 << 20      # guard at both ends of the arena, bytes
_ALIGN = 512           # what the caching allocator gives a fresh tensor


def fill_bits(fill) -> int:
    """the int32 bit pattern of a fill value: "nan" (the guard NaN) or "big" (+1e30)"""
    if fill == "nan":
        return GUARD_NAN_BITS
    if fill == "big":
        return int(np.float32(BIG).view(np.int32))
    raise ValueError(f"fill must be 'nan' or 'big', got {fill!r}")


class GuardError(AssertionError):
    pass


class _Slot:
    __slots__ = ("name", "off", "nbytes", "view", "out", "finite")

    def __init__(self, name, off, nbytes, view, out, finite):
        self.name, self.off, self.nbytes, self.view, self.out, self.finite = name, off, nbytes, view, out, finite


class Arena:
    """One allocation; tensors are bump-allocated views with guard bands in front and behind."""

    def __init__(self, device="cpu", fill="nan", nbytes=96 << 20, min_gap=MIN_GAP, end_gap=END_GAP):
        assert nbytes % _ALIGN == 0 and min_gap % _ALIGN == 0 and end_gap % _ALIGN == 0
        assert min_gap >= MIN_GAP and end_gap >= END_GAP, "guard bands may grow, not shrink"
        self.device, self.nbytes, self.min_gap, self.end_gap = torch.device(device), nbytes, min_gap, end_gap
        # _ALIGN spare bytes so that the first usable byte can be rounded up to a 512-byte address
        self._raw = torch.empty(nbytes + _ALIGN, dtype=torch.uint8, device=self.device)
        lead = (-self._raw.data_ptr()) % _ALIGN
        self.buf = self._raw[lead:lead + nbytes]
        assert self.buf.data_ptr() % _ALIGN == 0
        self._quad = {}
        self.reset(fill)

    # ------------------------------------------------------------------ layout
    def reset(self, fill=None):
        """forget every placement and re-poison the whole arena"""
        if fill is not None:
            self.fill = fill
            self.bits = fill_bits(fill)
        self.buf.view(torch.int32).fill_(self.bits)
        self.slots = []
        self._top = self.end_gap

    def place(self, src, skew=0, dtype=torch.float32, name=None, out=False, finite=None):
        """A contiguous view with data_ptr() % 16 == 4 * skew (skew in 0..3 floats), guarded on both sides.
        src: a tensor (copied in; its dtype wins) or a shape.  out: the kernel writes this buffer — a shape is pre-filled
        with the guard NaN (whatever the arena's fill), a tensor keeps its values (accumulated into / updated in place) —
        and check() wants every element of a floating-point ``out`` body finite (finite=False: a scratch whose contents are
        the kernel's business)."""
        if not 0 <= int(skew) <= 3:
            raise ValueError("skew is 0..3 floats")
        if isinstance(src, torch.Tensor):
            dtype, shape = src.dtype, tuple(src.shape)
        else:
            shape = (int(src),) if isinstance(src, int) else tuple(int(s) for s in src)
        esz = torch.empty((), dtype=dtype).element_size()
        n = 1
        for s in shape:
            n *= s
        nbytes = n * esz
        off = (self._top + _ALIGN - 1) // _ALIGN * _ALIGN + 4 * int(skew)
        end = off + nbytes
        if end + self.min_gap + self.end_gap > self.nbytes:
            raise MemoryError(f"arena of {self.nbytes} bytes is full placing {name or shape}")
        view = self.buf[off:end].view(dtype).view(shape) if n else torch.empty(shape, dtype=dtype, device=self.device)
        if isinstance(src, torch.Tensor):
            view.copy_(src)
        elif n and self.bits != GUARD_NAN_BITS:
            self.buf[off:end].copy_(self._pattern(off, nbytes, GUARD_NAN_BITS))
        assert n == 0 or view.data_ptr() % 16 == 4 * int(skew)
        if finite is None:
            finite = bool(out) and dtype.is_floating_point
        self.slots.append(_Slot(name or f"t{len(self.slots)}", off, nbytes, view, bool(out), finite))
        self._top = end + self.min_gap
        return view

    def _pattern(self, off, nbytes, bits):
        """the bytes a region [off, off + nbytes) of the arena holds when filled with the repeating 4-byte pattern"""
        b = self._quad.get(bits)
        if b is None:
            b = self._quad[bits] = torch.tensor([(bits >> (8 * i)) & 0xFF for i in range(4)], dtype=torch.uint8,
                                                device=self.device)
        lo = off - off % 4
        reps = (off + nbytes - lo + 3) // 4
        return b.repeat(reps)[off - lo: off - lo + nbytes]

    # ------------------------------------------------------------------ verdict
    def bands(self):
        """[(start, end, tensor behind, tensor in front)] — the guard bands, in address order"""
        out, pos, prev = [], 0, None
        for s in self.slots:
            out.append((pos, s.off, prev, s))
            pos, prev = s.off + s.nbytes, s
        out.append((pos, self.nbytes, prev, None))
        return out

    def problems(self):
        errs = []
        for a, b, before, after in self.bands():
            if b <= a:
                continue
            bad = self.buf[a:b] != self._pattern(a, b - a, self.bits)
            if not bool(bad.any()):
                continue
            idx = bad.nonzero().flatten()
            first, last, n = int(idx[0]), int(idx[-1]), int(idx.numel())
            # name the damage by the nearer tensor: bytes past the end of `before`, or bytes before the start of `after`
            if before is not None and (after is None or first < (b - a) - 1 - last):
                errs.append(f"guard AFTER '{before.name}' damaged: {n} bytes, first at +{first} and last at +{last} bytes "
                            f"past its end")
            else:
                errs.append(f"guard BEFORE '{after.name}' damaged: {n} bytes, first at -{(b - a) - first} and last at "
                            f"-{(b - a) - last} bytes before its start")
        for s in self.slots:
            if s.finite and s.view.numel():
                fin = torch.isfinite(s.view)
                if not bool(fin.all()):
                    flat = s.view.reshape(-1)
                    idx = (~fin.reshape(-1)).nonzero().flatten()
                    i0 = int(idx[0])
                    unwritten = int((flat[idx].view(torch.int32) == GUARD_NAN_BITS).sum())
                    errs.append(f"output '{s.name}': {idx.numel()} of {flat.numel()} elements not finite, first at flat index "
                                f"{i0} ({unwritten} still hold the guard NaN: never written, or copied from a guard; "
                                f"{idx.numel() - unwritten} other NaN/Inf: computed from poisoned or out-of-bounds data)")
        return errs

    def check(self):
        """every guard band bit for bit (through an integer view), every output body written and finite"""
        errs = self.problems()
        if errs:
            raise GuardError("; ".join(errs))


class TorchProxy:
    """``torch`` as scat_amd.ops sees it, with empty / empty_like / zeros / full carved out of an arena (as outputs, at
    ``skew``); everything else is torch's own.  Buffers allocated inside ``scratch()`` are workspaces: the allocator always
    aligns them and their contents belong to the kernel, so they are placed at skew 0 and not asked to be finite — but
    they sit between guards like everything else."""

    def __init__(self, arena, skew=0):
        self._arena, self.skew, self._scratch = arena, skew, 0

    def __getattr__(self, name):
        return getattr(torch, name)

    @contextlib.contextmanager
    def scratch(self):
        self._scratch += 1
        try:
            yield
        finally:
            self._scratch -= 1

    def _carve(self, shape, dtype, name):
        a = self._arena
        dtype = dtype or torch.float32
        if self._scratch:
            return a.place(shape, 0, dtype, name=f"scratch{len(a.slots)}", out=True, finite=False)
        return a.place(shape, self.skew, dtype, name=f"{name}{len(a.slots)}", out=True)

    @staticmethod
    def _shape(size):
        if len(size) == 1 and not isinstance(size[0], int):
            return tuple(size[0])
        return tuple(size)

    def _dev_ok(self, device):
        return device is None or torch.device(device).type == self._arena.device.type

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._dev_ok(device):
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._carve(self._shape(size), dtype, "empty")

    def empty_like(self, t, **kw):
        return self._carve(tuple(t.shape), t.dtype, "empty_like")

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._dev_ok(device):
            return torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._carve(self._shape(size), dtype, "zeros").zero_()

    def full(self, size, fill_value, dtype=None, device=None, **kw):
        if not self._dev_ok(device):
            return torch.full(size, fill_value, dtype=dtype, device=device, **kw)
        return self._carve(self._shape((size,)), dtype, "full").fill_(fill_value)


def exact_workspace(proxy, stream=lambda: 0):
    """A stand-in for scat_amd.ops.workspace(nbytes, device, slot) that carves EXACTLY nbytes (16 where 0 is asked for, so
    that the pointer is not null) out of the proxy's arena as scratch: skew 0, the guard NaN as contents, a guard band
    right behind the last requested byte.  Every request gets a fresh slot; only when the arena is full is a buffer of the
    same (slot, stream, nbytes) handed out again.  Never a larger one."""
    cache = {}

    def workspace(nbytes, device, slot="default"):
        n = int(nbytes) or 16
        key = (slot, stream(), n)
        try:
            with proxy.scratch():
                buf = proxy.empty(n, dtype=torch.uint8, device=device)
        except MemoryError:
            buf = cache.get(key)
            if buf is None:
                raise
        cache[key] = buf
        assert buf.numel() == n
        return buf
    return workspace


def header_pointer_entry_points():
    """{name: [pointer argument names]} for every prototype of include/scat_hip.h with at least one pointer argument
    other than ``stream``"""
    import ctypes

    from scat_amd._lib import parse_header

    out = {}
    for name, (_, args) in parse_header().items():
        ptrs = [an for ty, an in args if ty is ctypes.c_void_p and an != "stream"]
        if ptrs:
            out[name] = ptrs
    return out
