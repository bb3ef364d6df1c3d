"""Writes tests/golden/hand_mesh.npz from the mesh the reference ships as data, extra_data/hand.obj (778 vertices and
1538 faces in MANO order), on the development machine only:

    python tools/gen_render_golden.py /path/to/reference/checkout

Stored: v fp32 [778,3] (the `v` lines) and f int32 [1538,3] (the `f` lines, made 0-based): the real topology for the
renderer's tests (tests/test_render.py, tests/test_gpu_render.py) without the licence-gated pickle.  Every other line of
the file (comments, the material library) is ignored.  No test reads the reference checkout."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse_obj(path):
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            t = line.split()
            if not t:
                continue
            if t[0] == "v":
                v.append([float(x) for x in t[1:4]])
            elif t[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in t[1:4]])
    return np.asarray(v, dtype=np.float32), np.asarray(f, dtype=np.int32)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    v, f = parse_obj(os.path.join(sys.argv[1], "extra_data", "hand.obj"))
    assert v.shape == (778, 3) and f.shape == (1538, 3), (v.shape, f.shape)
    assert f.min() == 0 and f.max() == 777 and len(np.unique(f)) == 778
    out = os.path.join(ROOT, "tests", "golden", "hand_mesh.npz")
    np.savez_compressed(out, v=v, f=f)
    print(f"{out}: v {v.shape} {v.dtype} in [{v.min():.4f}, {v.max():.4f}], f {f.shape} {f.dtype}, "
          f"{os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
