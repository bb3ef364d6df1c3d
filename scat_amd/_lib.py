"""ctypes binding of libscat_hip.so. Prototypes are parsed from the public headers (HEADERS below): include/scat_hip.h
(the train step), scat_mesh_eval.h (on-device mesh scoring), scat_eval.h (on-device evaluation), scat_mano_fit_kp.h (the MANO fit to 2-D and 3-D keypoints),
scat_mano_fit.h (the MANO fit), scat_render.h (the mesh and skeleton renderer) and scat_mano.h (the MANO layer), so the
headers are the single source of truth for the C ABI. EXTENSION_HEADERS (scat_mano_fit_seq.h, the MANO fit to a track of
frames) are bound the same way beside them, and _Lib.bind(path) binds any further header of the library on first use
(scat_mano_fit_verts.h, the MANO fit to a full mesh, scat_mano_fit_points.h, the MANO fit to a point cloud,
scat_mano_fit_plane.h, the point-to-plane form of the latter, scat_mano_fit_seq_kp.h, the MANO fit to a track of
keypoints, scat_mano_fit_seq_verts.h, the MANO fit to a track of meshes and of point clouds,
include_ext/scat_mano_fit_views.h, the MANO fit to keypoints in calibrated views, and
include_ext/scat_mano_fit_seq_views.h, the MANO fit to a track of such keypoints, from scat_amd/fit.py).
The product path has NO fallback: if the library is missing, importing a kernel raises."""
from __future__ import annotations

import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "scat_hip.h")
EVAL_HEADER = os.path.join(HERE, "..", "include", "scat_eval.h")
MESH_EVAL_HEADER = os.path.join(HERE, "..", "include", "scat_mesh_eval.h")
RENDER_HEADER = os.path.join(HERE, "..", "include", "scat_render.h")
MANO_HEADER = os.path.join(HERE, "..", "include", "scat_mano.h")
FIT_HEADER = os.path.join(HERE, "..", "include", "scat_mano_fit.h")
FIT_KP_HEADER = os.path.join(HERE, "..", "include", "scat_mano_fit_kp.h")
HEADERS = (HEADER, MESH_EVAL_HEADER, EVAL_HEADER, FIT_KP_HEADER, FIT_HEADER, RENDER_HEADER, MANO_HEADER)   # every public header of the one library; parse_header() defaults to the first
# Headers bound beside HEADERS, the same way (parsed prototypes, the checked wrapper, a missing symbol raises), into
# _Lib.by_extension: include/scat_mano_fit_seq.h, the MANO fit to a track of frames
FIT_SEQ_HEADER = os.path.join(HERE, "..", "include", "scat_mano_fit_seq.h")
EXTENSION_HEADERS = (FIT_SEQ_HEADER,)
LIBPATH = os.path.join(HERE, "libscat_hip.so")
if os.environ.get("SCAT_LIBPATH"):
    # measurement tools only (tools/pw_stamp.py, rows_stamp.py): the -DSCAT_DIAG build whose kernels can overwrite their
    # outputs with time stamps.  Said loudly, because results from that library are not the product's.
    import warnings

    LIBPATH = os.path.abspath(os.environ["SCAT_LIBPATH"])
    warnings.warn(f"scat_amd: SCAT_LIBPATH set, loading {LIBPATH} instead of the shipped libscat_hip.so", RuntimeWarning)

_CT = {
    "int": ctypes.c_int,
    "int64_t": ctypes.c_int64,
    "uint64_t": ctypes.c_uint64,
    "float": ctypes.c_float,
}


class HostInOut(ctypes.c_void_p):
    """an argument like ``ScatEpilogue* epi``: a non-const pointer to one of the header's own structs.  It is HOST memory
    that the entry point reads and writes before its first check, so it is null or the address of a real struct, never a
    made-up integer as a device pointer may be in a call that is to stop in the host code.  Its own type, so that code
    which fabricates every ``c_void_p`` argument leaves this one null; it takes what ``c_void_p`` takes."""


def parse_header(path: str = HEADER):
    """-> {name: (restype, [(ctype, argname)])} for every prototype in the header."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    protos = {}
    for m in re.finditer(r"(?m)^\s*(const char\*|int64_t|int)\s+(scat_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        at = []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                if "*" in a:
                    at.append((HostInOut if re.match(r"Scat\w+\s*\*", a) else ctypes.c_void_p, a.split("*")[-1].strip()))
                else:
                    ty, an = a.rsplit(" ", 1)
                    at.append((_CT[ty.replace("const ", "").strip()], an))
        rt = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}[ret]
        protos[name] = (rt, at)
    return protos


class ScatError(RuntimeError):
    pass


class _Lib:
    def __init__(self):
        if not os.path.exists(LIBPATH):
            raise ScatError(
                f"{LIBPATH} not found: build it with `python -m scat_amd.build` (hipcc, gfx950). "
                "There is no CPU fallback on the product path.")
        # torch bundles its own HIP runtime and publishes it RTLD_GLOBAL; let it initialise the device
        # first so this library's hip* symbols resolve to that one runtime (two runtimes racing for
        # /dev/kfd in one process end in "No HIP GPUs are available").
        import torch

        if torch.cuda.is_available():
            torch.cuda.init()
        self.cdll = ctypes.CDLL(LIBPATH)
        # by_header: {header path: its prototypes}, every public header; protos: the train step and evaluation merged, the
        # table the workspace tests index (tests/test_eval.py pins it to those two headers)
        self.by_header = {h: parse_header(h) for h in HEADERS}
        self.protos = {**self.by_header[HEADER], **self.by_header[EVAL_HEADER]}
        self.by_extension = {h: parse_header(h) for h in EXTENSION_HEADERS}
        self.bound = {}      # bind(): {header path: namespace of its entry points}
        for name, proto in ((n, p) for protos in (*self.by_header.values(), *self.by_extension.values())
                            for n, p in protos.items()):
            setattr(self, name, self._resolve(name, proto))

    def _resolve(self, name, proto):
        """the library's symbol `name` with the parsed prototype; an int return goes through the checked wrapper"""
        rt, at = proto
        fn = getattr(self.cdll, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = rt
        fn.argtypes = [t for t, _ in at]
        if rt is ctypes.c_int and name not in ("scat_version", "scat_get_math_mode"):
            return self._checked(fn, name)
        return fn

    def bind(self, header_path):
        """-> a namespace with one callable per entry point that the header declares, bound like those of HEADERS (parsed
        prototypes, the checked wrapper on int returns); a declared symbol that the library lacks raises AttributeError
        naming it.  Cached in self.bound by path; HEADERS, EXTENSION_HEADERS and their tables are not touched."""
        if header_path not in self.bound:
            import types

            fns = {}
            for name, proto in parse_header(header_path).items():
                try:
                    fns[name] = self._resolve(name, proto)
                except AttributeError:
                    raise AttributeError(f"{LIBPATH} lacks {name}, which {header_path} declares") from None
            self.bound[header_path] = types.SimpleNamespace(**fns)
        return self.bound[header_path]

    def _checked(self, fn, name):
        last = self.cdll.scat_last_error
        last.restype = ctypes.c_char_p

        def call(*a):
            rc = fn(*a)
            if rc != 0:
                raise ScatError(f"{name} failed ({rc}): {last().decode(errors='replace')}")
            return rc

        call.__name__ = name
        return call


_lib = None


def lib() -> _Lib:
    global _lib
    if _lib is None:
        _lib = _Lib()
    return _lib
