"""Numpy / pure-Python restatement of rotated window cuts (SceneDataset(rotate=...), INTERP_ROT of ryolo_resize_hsv_windows; not a test
module): the two affine maps of a rotated use, the cut (oracle.ref_data.warp_perspective_numpy of the whole scene under the pixel map,
border 114, then the hsv restatement), the label map into the window frame, and the angle draws.  Written from the definitions in
DESIGN.md §4.5, not from datasets/augment.py; every float operation is a single rounded double operation."""
import contextlib
import math
import random

import numpy as np

from oracle import ref_data
from tests import scene_ref as SR

FILL = 114
INTERP_ROT = 3


# ---------------------------------------------------------------------------------------------- the maps
def cos_sin(phi_deg):
    """(cos, sin) of the angle; exactly 0 / +-1 at multiples of 90 degrees."""
    q = phi_deg / 90.0
    if q == math.floor(q):
        return ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(q) % 4]
    r = math.radians(phi_deg)
    return math.cos(r), math.sin(r)


def maps(x0, y0, c, N, phi_deg):
    """(minv, fwd), float64 [6] each.  s = c / N, k = (c - 1) / 2, q = (x0 + k, y0 + k).
    minv: result pixel (u, v) -> scene pixel index q + R (wx, wy), wx = (u + 0.5) s - 0.5 - k, wy likewise, R = [[cos, -sin], [sin, cos]].
    fwd:  scene coordinate p -> R^T (p - q) + k, the c x c window frame."""
    cs, sn = cos_sin(float(phi_deg))
    s, k = c / N, (c - 1) / 2.0
    qx, qy = x0 + k, y0 + k
    t = 0.5 * s - 0.5 - k                                            # w at u = 0
    minv = np.array([cs * s, -sn * s, qx + (cs - sn) * t, sn * s, cs * s, qy + (sn + cs) * t], dtype=np.float64)
    fwd = np.array([cs, sn, k - (cs * qx + sn * qy), -sn, cs, k - (cs * qy - sn * qx)], dtype=np.float64)
    return minv, fwd


def apply(m6, x, y):
    return m6[0] * x + m6[1] * y + m6[2], m6[3] * x + m6[4] * y + m6[5]


# ---------------------------------------------------------------------------------------------- pixels
@contextlib.contextmanager
def _inverse_is(minv3):
    """warp_perspective_numpy inverts the matrix it is given; the kernel is handed the inverse map.  For the duration of the call the
    inversion returns that map, so the restatement samples with exactly the doubles the kernel reads (as tests/copy_paste_ref.py does)."""
    saved = np.linalg.inv
    np.linalg.inv = lambda _: minv3
    try:
        yield
    finally:
        np.linalg.inv = saved


def rot_cut(scene, minv, N, gains=None):
    """The N x N rotated cut of a uint8 HWC scene under `minv`, then the hsv gains (hue, sat, val) when given."""
    minv3 = np.array([list(minv[0:3]), list(minv[3:6]), [0.0, 0.0, 1.0]], dtype=np.float64)
    with _inverse_is(minv3):
        out = ref_data.warp_perspective_numpy(np.ascontiguousarray(scene), np.eye(3), (N, N), border=FILL)
    return out if gains is None else ref_data.hsv_gain_numpy(out, np.asarray(gains, dtype=np.float64))


# ---------------------------------------------------------------------------------------------- labels
def map_polys(polys, fwd):
    """float32 [n, 8] scene pixels -> float32 [n, 8] in the window frame: float64 a x + b y + c left to right, one rounding to float32."""
    p = np.asarray(polys, dtype=np.float32).reshape(-1, 8).astype(np.float64)
    out = np.empty_like(p)
    out[:, 0::2], out[:, 1::2] = apply(fwd, p[:, 0::2], p[:, 1::2])
    return out.astype(np.float32)


def label_rows(polys, fwd, c, thr):
    """The labels of a rotated use: (mapped float32 [n, 8], iof float64 [n], keep bool [n]) — the mapped polygons through the existing
    window rule against (0, 0, c)."""
    return SR.label_rows(map_polys(polys, fwd), 0, 0, c, thr)


def window_labels(polys, cls, fwd, c, thr):
    """What the label file of the rotated cut would hold: kept labels in file order, in the window frame."""
    cls = np.asarray(cls, dtype=np.float32).reshape(-1)
    mp, _, keep = label_rows(polys, fwd, c, thr)
    return mp[keep], cls[keep]


# ---------------------------------------------------------------------------------------------- draws
class Draws:
    """The angle draws of Rotate(degrees, p, step, seed): per use one coin; under p one uniform angle; with step > 0 the multiple k * step,
    k = round(angle / step) clamped to |k| <= floor(degrees / step)."""

    def __init__(self, degrees=180.0, p=0.5, step=0.0, seed=0):
        self.degrees, self.p, self.step, self.rng = degrees, p, step, random.Random(seed)

    def draw(self):
        if not self.rng.random() < self.p:
            return None
        a = self.rng.uniform(-self.degrees, self.degrees)
        if self.step > 0:
            kmax = math.floor(self.degrees / self.step)
            a = max(-kmax, min(kmax, round(a / self.step))) * self.step
        return a
