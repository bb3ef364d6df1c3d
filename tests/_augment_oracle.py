"""fp64 numpy restatement of the augmentation operator, the oracle of test_augment.py and
test_gpu_augment.py.  It restates formulas only; each label formula cites the line of the reference's dataset module
(dataset/load_STB.py, dataset/rotation.py of tomguluson92/SCAT) it comes from, so it can be compared by reading."""
import math
import random

import numpy as np

OUT = 224


def draw_sequence(B, rotation, motion_blur):
    """Literal restatement of the reference's per-sample draws (load_STB.py:265-272 with motion_blur's own draws,
    :159 and :180, in between) -> list of (k, choice or None, angle): k = 0 when the blur is not applied."""
    rows = []
    for _ in range(B):
        k, choice, angle = 0, None, 0
        if motion_blur:
            use_blur = random.randint(0, 5)            # load_STB.py:266
            if use_blur == 1:                          # load_STB.py:267
                k = random.randint(1, 10)              # load_STB.py:159  kernel_size
                choice = random.randint(0, 1)          # load_STB.py:180  0 = vertical_mb
        if rotation:
            angle = random.randint(1, 360)             # load_STB.py:271
        rows.append((k, choice, angle))
    return rows


def r101(i, n):
    """cv2.BORDER_REFLECT_101 (filter2D's default border)"""
    i = np.abs(i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def labels_and_plan(j2d, j3d, W, H, flip, angle, norm3d=True):
    """-> labels [105] float64 and the sample's geometry: M (2x3, frame -> canvas), the un-rounded box (l, t, r, b), PIL's
    integer box origin L, T and size nw, nh, the canvas nW, nH and the supersampling grid side n."""
    j2 = np.asarray(j2d, dtype=np.float64).copy()
    j3 = np.asarray(j3d, dtype=np.float64).copy()
    if norm3d:
        l = np.sqrt(((j3[4] - j3[5]) ** 2).sum())      # load_STB.py:99-105
        j3 = j3 * (0.03058954 / l)                     # load_STB.py:106-107
        j3[:, 0] *= -1                                 # load_STB.py:108
        j3 = j3 - j3[1]                                # load_STB.py:109
    if flip:
        j2[:, 0] = W - j2[:, 0]                        # load_STB.py:71-73: [width, 0] + (-x, y)
    M = np.array([[1.0, 0, 0], [0, 1.0, 0]])
    nW, nH = W, H
    if angle:
        rad = math.radians(angle)
        al, be = math.cos(rad), math.sin(rad)          # cv2.getRotationMatrix2D(center, angle, 1.0), rotation.py:17
        cx, cy = W // 2, H // 2                        # rotation.py:12
        M = np.array([[al, be, (1 - al) * cx - be * cy], [-be, al, be * cx + (1 - al) * cy]])
        nW = int(H * abs(be) + W * abs(al))            # rotation.py:22
        nH = int(H * abs(al) + W * abs(be))            # rotation.py:23
        M[0, 2] += nW / 2 - cx                         # rotation.py:26
        M[1, 2] += nH / 2 - cy                         # rotation.py:27
        j2 = (M @ np.hstack([j2, np.ones((21, 1))]).T).T      # rotation.py:33-34
        R = np.eye(3)                                  # rotation.py:39-43 (the 4th row/column only carries the 1)
        R[0, 0], R[0, 1], R[1, 0], R[1, 1] = M[0, 0], M[0, 1], -M[0, 1], M[0, 0]
        j3 = (R @ j3.T).T                              # rotation.py:45
    c = j2[4]                                          # load_STB.py:77
    mn = np.maximum(j2.min(0), 0)                      # load_STB.py:78
    mx = np.minimum(j2.max(0), [nW, nH])               # load_STB.py:79
    s = float(np.max(1.3 * np.maximum(mx - c, c - mn)))       # load_STB.py:80-81
    s = min(max(s, 10), 500)                           # load_STB.py:82
    l, t = c - s                                       # load_STB.py:83
    r, b = c + s                                       # load_STB.py:84
    # Image.crop (load_STB.py:85) rounds its box to integers, half to even; image.size is then (R - L, B - T)
    L, T, Rr, Bb = (int(np.rint(v)) for v in (l, t, r, b))
    nw, nh = Rr - L, Bb - T                            # load_STB.py:87
    j2 = (j2 + [-l, 0] + [0, -t]) * (OUT / nw)         # load_STB.py:89-93: scale = 224 / new_width for both axes
    n = min(max(int(math.floor(nw / OUT + 0.5)), 1), 4)
    lab = np.concatenate([j3.reshape(-1), j2.reshape(-1)])    # load_STB.py:286-289
    return lab, dict(M=M, box=(l, t, r, b), L=L, T=T, nw=nw, nh=nh, nW=nW, nH=nH, n=n)


def half_distance(plan):
    """distance of the un-rounded box coordinates from the nearest half-integer (where PIL's rounding flips)"""
    return min(abs(v - math.floor(v) - 0.5) for v in plan["box"])


def blurred(src, flip, k, vert):
    """HxWx3 uint8 -> float64 mirrored (ImageOps.mirror) and motion-blurred frame: cv2.filter2D with a k x k kernel
    whose middle column (vertical) or row (horizontal) (k-1)//2 is 1/k, anchor k//2, BORDER_REFLECT_101."""
    H, W, _ = src.shape
    F = (src[:, ::-1] if flip else src).astype(np.float64)
    if k:
        m, a = (k - 1) // 2, k // 2
        ys, xs = np.arange(H), np.arange(W)
        acc = np.zeros_like(F)
        for i in range(k):
            if vert:
                acc += F[r101(ys + i - a, H)][:, r101(xs + m - a, W)]
            else:
                acc += F[r101(ys + m - a, H)][:, r101(xs + i - a, W)]
        F = acc / k
    return F


def sample_points(plan, sx, sy, n):
    Mi = np.linalg.inv(np.vstack([plan["M"], [0, 0, 1]]))
    o = np.arange(OUT)
    u = plan["L"] + (o + (sx + 0.5) / n) * plan["nw"] / OUT - 0.5
    v = plan["T"] + (o + (sy + 0.5) / n) * plan["nh"] / OUT - 0.5
    U, V = np.meshgrid(u, v)
    return Mi[0, 0] * U + Mi[0, 1] * V + Mi[0, 2], Mi[1, 0] * U + Mi[1, 1] * V + Mi[1, 2]


def image(src, flip, k, vert, plan, coord_dtype=np.float64):
    """src HxWx3 uint8 -> 3x224x224 float64: the mean of n x n bilinear samples of the blurred frame, lattice points
    outside the frame counted as 0, /127.5 - 1.  coord_dtype=np.float32 rounds the sample coordinates to fp32 (to
    measure what such a kernel would lose)."""
    H, W, _ = src.shape
    F = blurred(src, flip, k, vert)
    n = plan.get("n") or min(max(int(math.floor(plan["nw"] / OUT + 0.5)), 1), 4)
    Fp = np.pad(F, ((2, 2), (2, 2), (0, 0)))           # two black pixels all round: lattice points -2 .. W+1
    out = np.zeros((OUT, OUT, 3))
    for sy in range(n):
        for sx in range(n):
            X, Y = sample_points(plan, sx, sy, n)
            X = np.clip(X.astype(coord_dtype).astype(np.float64), -2, W)
            Y = np.clip(Y.astype(coord_dtype).astype(np.float64), -2, H)
            x0, y0 = np.floor(X).astype(int), np.floor(Y).astype(int)
            wx, wy = (X - x0)[..., None], (Y - y0)[..., None]
            g = lambda yy, xx: Fp[yy + 2, xx + 2]
            out += (g(y0, x0) * (1 - wx) + g(y0, x0 + 1) * wx) * (1 - wy) \
                + (g(y0 + 1, x0) * (1 - wx) + g(y0 + 1, x0 + 1) * wx) * wy
    return (out / (n * n) / 127.5 - 1).transpose(2, 0, 1)


def seeded_joints(rng, B, W=640, H=480, ext=(40, 110)):
    """hand centre well inside the frame, extent ext pixels -> j2d [B,21,2], j3d [B,21,3] float32"""
    ctr = rng.uniform([220, 170], [W - 220, H - 170], (B, 1, 2))
    e = rng.uniform(ext[0], ext[1], (B, 1, 1))
    j2 = ctr + rng.uniform(-1, 1, (B, 21, 2)) * e
    j3 = rng.normal(0, 0.03, (B, 21, 3))
    return j2.astype(np.float32), j3.astype(np.float32)
