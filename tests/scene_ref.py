"""Numpy / pure-Python restatement of the scene-window stage (datasets/scene_dataset.py, csrc/scene.hip): the window plan, the jitter
draws, the window cut with fill, and the shift / intersection-over-foreground / keep rule of the labels — with the operation order the
header fixes, so that the device results can be compared bit for bit.  The reference has no such stage; these semantics are this
project's and this file is what pins them.  Python floats are IEEE doubles and every operation below is a single rounded one (no fused
multiply-add), which is what the kernel is built to do (-ffp-contract=off)."""
import math

import numpy as np

FILL = 114


# ---------------------------------------------------------------------------------------------- window plan
def starts(L, size, stride):
    if L <= size:
        return [0]
    out, x = [], 0
    while x + size < L:
        out.append(x)
        x += stride
    out.append(L - size)
    return out


def scene_windows(H, W, size, overlap, rates=(1.0,)):
    out = []
    for ri, r in enumerate(rates):
        c = int(size / r + 0.5)
        stride = c - int(overlap / r + 0.5)
        for y0 in starts(H, c, stride):
            for x0 in starts(W, c, stride):
                out.append((ri, x0, y0, c))
    return out


# ---------------------------------------------------------------------------------------------- jitter
def jitter_window(wrng, H, W, c, polys, p_object):
    """Draw order: the coin, the label index if drawn, x, y."""
    lox, hix = min(0, W - c), max(0, W - c)
    loy, hiy = min(0, H - c), max(0, H - c)
    coin = wrng.random()
    if coin < p_object and len(polys):
        p = [float(v) for v in polys[wrng.randrange(len(polys))]]
        mx = (p[0] + p[2] + p[4] + p[6]) / 4.0
        my = (p[1] + p[3] + p[5] + p[7]) / 4.0
        a, b = max(lox, math.ceil(mx) - c + 1), min(hix, math.floor(mx))
        if a <= b:
            lox, hix = a, b
        a, b = max(loy, math.ceil(my) - c + 1), min(hiy, math.floor(my))
        if a <= b:
            loy, hiy = a, b
    x0 = wrng.randint(lox, hix)
    y0 = wrng.randint(loy, hiy)
    return x0, y0


# ---------------------------------------------------------------------------------------------- pixels
def cut_window(scene, x0, y0, c):
    """The c x c window of a uint8 HWC scene, FILL wherever it lies outside."""
    H, W = scene.shape[:2]
    out = np.full((c, c, 3), FILL, dtype=np.uint8)
    xa, xb, ya, yb = max(x0, 0), min(x0 + c, W), max(y0, 0), min(y0 + c, H)
    if xa < xb and ya < yb:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = scene[ya:yb, xa:xb]
    return out


# ---------------------------------------------------------------------------------------------- labels
def shoelace(pts):
    """sum of (x_k y_k+1 - x_k+1 y_k) in vertex order, left to right (floats or Fractions)."""
    s = 0
    n = len(pts)
    for k in range(n):
        xk, yk = pts[k]
        xj, yj = pts[(k + 1) % n]
        s = s + (xk * yj - xj * yk)
    return s


def clip_plane(pts, axis, bound, ge):
    out = []
    n = len(pts)
    for k in range(n):
        a, b = pts[k], pts[(k + 1) % n]
        ak, ao, bk, bo = a[axis], a[1 - axis], b[axis], b[1 - axis]
        ain = ak >= bound if ge else ak <= bound
        bin_ = bk >= bound if ge else bk <= bound
        if ain:
            out.append(a)
        if ain != bin_:
            t = (bound - ak) / (bk - ak)
            o = ao + t * (bo - ao)
            out.append((bound, o) if axis == 0 else (o, bound))
    return out


def clip_window(pts, c, zero=0.0):
    """Sutherland-Hodgman against [0, c]^2, planes x >= 0, x <= c, y >= 0, y <= c; a vertex on a plane is inside."""
    for axis, bound, ge in ((0, zero, True), (0, c, False), (1, zero, True), (1, c, False)):
        pts = clip_plane(pts, axis, bound, ge)
    return pts


def iof_quad(pts, c, arith=float):
    """(IoF of the quad [(x, y)] * 4 with [0, c]^2, vertex count of the clip); (None, 0) when the quad has no area.  `arith` converts the
    inputs: float = the kernel's fp64 operations one by one, fractions.Fraction = exact."""
    pts = [(arith(x), arith(y)) for x, y in pts]
    area = abs(shoelace(pts))
    if not area > 0:
        return None, 0
    cl = clip_window(pts, arith(c), arith(0))
    return min(arith(1), abs(shoelace(cl)) / area), len(cl)


def shift_poly(poly, x0, y0):
    """p' = fl32(p - origin) per coordinate, fp32."""
    p = np.asarray(poly, dtype=np.float32).reshape(-1, 8).copy()
    p[:, 0::2] = p[:, 0::2] - np.float32(x0)
    p[:, 1::2] = p[:, 1::2] - np.float32(y0)
    return p


def label_rows(polys, x0, y0, c, thr):
    """polys float32 [n, 8] in scene pixels -> (shifted float32 [n, 8], iof float64 [n] (0 for a quad without area), keep bool [n])."""
    sh = shift_poly(polys, x0, y0)
    iof = np.zeros(len(sh), dtype=np.float64)
    keep = np.zeros(len(sh), dtype=bool)
    for i, p in enumerate(sh):
        v, _ = iof_quad([(float(p[2 * k]), float(p[2 * k + 1])) for k in range(4)], c)
        if v is not None:
            iof[i] = v
            keep[i] = v >= thr
    return sh, iof, keep


def cull(polys, x0, y0, c):
    """The host-side cull: labels whose bounding box overlaps the window with positive extent (file order)."""
    polys = np.asarray(polys, dtype=np.float32).reshape(-1, 8)
    if not len(polys):
        return np.zeros(0, dtype=np.int64)
    xs, ys = polys[:, 0::2], polys[:, 1::2]
    return np.nonzero((xs.max(1) > x0) & (xs.min(1) < x0 + c) & (ys.max(1) > y0) & (ys.min(1) < y0 + c))[0]


def window_labels(polys, cls, x0, y0, c, thr):
    """What a pre-cut window's label file would hold: the kept labels of the window, shifted, in file order."""
    polys = np.asarray(polys, dtype=np.float32).reshape(-1, 8)
    cls = np.asarray(cls, dtype=np.float32).reshape(-1)
    idx = cull(polys, x0, y0, c)
    sh, _, keep = label_rows(polys[idx], x0, y0, c, thr)
    return sh[keep], cls[idx][keep]
