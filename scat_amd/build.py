"""Build libscat_hip.so (gfx950) in-tree with hipcc. No torch dependency in the library."""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libscat_hip.so")
OBJ = os.path.join(HERE, "csrc", "_obj")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -fno-slp-vectorize: hipcc's SLP vectoriser turns adjacent scalar fp32 adds / multiplies into packed fp32 instructions
# (v_pk_add_f32, v_pk_fma_f32), which cost ~17 issue cycles against 4 beside a busy matrix pipe (MI355X_MICROARCH.md,
# "price of one filler beside MFMAs ... an anti-lever") — every operand split is such a pair.  Measured on the whole
# library: weight gradients 3.95 -> 3.67 ms (tools/conv_bench.py), train step 23.66 -> 23.22 ms, same box.
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-fno-slp-vectorize", "-Wall", "-Wno-unused-function",
         "-Wno-unused-variable"]


def _sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


# The public headers the library ships; build() refuses to build without one of them.  The rebuild trigger below lists
# include/ instead, so a header added later counts before anyone names it here.
PUBLIC_HEADERS = ("scat_hip.h", "scat_mesh_eval.h", "scat_eval.h", "scat_render.h", "scat_mano.h", "scat_mano_fit.h",
                  "scat_mano_fit_kp.h", "scat_mano_fit_seq.h", "scat_mano_fit_verts.h", "scat_mano_fit_points.h",
                  "scat_mano_fit_seq_kp.h", "scat_mano_fit_plane.h", "scat_mano_fit_seq_verts.h")
INCLUDE = os.path.join(HERE, "..", "include")
# Headers added since the suite began to count the files of include/ live beside it in include_ext/: the same library, the
# same conventions, the same refusal to build without one of them, and a rebuild trigger of their own (_ext_headers_mtime)
EXT_HEADERS = ("scat_mano_fit_views.h",)
# the headers that joined include_ext/ after the first: checked by build() exactly as EXT_HEADERS is
EXT_HEADERS_MORE = ("scat_mano_fit_seq_views.h",)
INCLUDE_EXT = os.path.join(HERE, "..", "include_ext")


def _public_headers_mtime():
    return max(os.path.getmtime(os.path.join(INCLUDE, h)) for h in os.listdir(INCLUDE) if h.endswith(".h"))


def _ext_headers_mtime():
    return max((os.path.getmtime(os.path.join(INCLUDE_EXT, h)) for h in os.listdir(INCLUDE_EXT) if h.endswith(".h")), default=0.0)


def _deps_mtime():
    m = 0.0
    for root, _, files in os.walk(CSRC):
        if root.endswith(("_obj", "_obj_diag")):
            continue
        for f in files:
            if f.endswith((".h", ".hip")):
                m = max(m, os.path.getmtime(os.path.join(root, f)))
    return max(m, _public_headers_mtime(), _ext_headers_mtime())


DIAG_OUT = os.path.join(HERE, "..", "tools", "_bin", "libscat_hip_diag.so")


def build(force: bool = False, verbose: bool = True, diag: bool = False) -> str:
    """Compile every .hip for gfx950 and link the shared library. Returns its path.
    diag: the tools build (-DSCAT_DIAG: in-kernel time stamps, ablation and negative-result kernel variants) into
    tools/_bin/libscat_hip_diag.so — never the library the boundary ships; tools select it with SCAT_LIBPATH."""
    global OUT, OBJ
    if diag:
        out, obj, flags = os.path.abspath(DIAG_OUT), os.path.join(CSRC, "_obj_diag"), FLAGS + ["-DSCAT_DIAG"]
        os.makedirs(os.path.dirname(out), exist_ok=True)
        saved = (OUT, OBJ, list(FLAGS))
        OUT, OBJ = out, obj
        FLAGS[:] = flags
        try:
            return build(force, verbose, False)
        finally:
            OUT, OBJ = saved[0], saved[1]
            FLAGS[:] = saved[2]
    missing = [h for h in PUBLIC_HEADERS if not os.path.exists(os.path.join(INCLUDE, h))]
    if missing:
        raise RuntimeError(f"public headers missing from {os.path.abspath(INCLUDE)}: {missing}")
    missing = [h for h in EXT_HEADERS + EXT_HEADERS_MORE if not os.path.exists(os.path.join(INCLUDE_EXT, h))]
    if missing:
        raise RuntimeError(f"public headers missing from {os.path.abspath(INCLUDE_EXT)}: {missing}")
    if not force and os.path.exists(OUT) and os.path.getmtime(OUT) >= _deps_mtime():
        return OUT
    os.makedirs(OBJ, exist_ok=True)
    hdr_m = max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith(".h"))
    hdr_m = max(hdr_m, _public_headers_mtime(), _ext_headers_mtime())

    def one(src):
        o = os.path.join(OBJ, src[:-4] + ".o")
        s = os.path.join(CSRC, src)
        if not force and os.path.exists(o) and os.path.getmtime(o) >= max(os.path.getmtime(s), hdr_m):
            return o
        cmd = [HIPCC, *FLAGS, "-c", s, "-o", o]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
        if verbose and r.stderr.strip():
            print(r.stderr, file=sys.stderr)
        return o

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(one, _sources()))
    cmd = [HIPCC, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", OUT, *objs]
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, diag="--diag" in sys.argv))
