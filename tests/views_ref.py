"""Host restatements for the tests of the flip / 90-degree views of full-scene detection (include/ryolo.h, lib/tiled.py VIEWS): the
pixel definition, the point map, the fp32 box map the collect kernel must reproduce on the bits, the polygon identity against
oracle.ref_data.xywha2xyxyxyxy, and the class-wise oracle merge over entries (windows x views).  Written from the table of the eight
views, not from the code under test."""
import numpy as np
import torch

import oracle
from oracle import ref_data

f32 = np.float32
NAMES = ("id", "hflip", "vflip", "rot180", "transpose", "rot90", "rot270", "antitranspose")
HALF_PI, PI = f32(np.pi / 2), f32(np.pi)

_PIXELS = {
    "id": lambda w: w,
    "hflip": lambda w: w[:, ::-1],
    "vflip": lambda w: w[::-1],
    "rot180": lambda w: w[::-1, ::-1],
    "transpose": lambda w: w.transpose(1, 0, 2),
    "rot90": lambda w: np.rot90(w, 1),
    "rot270": lambda w: np.rot90(w, 3),
    "antitranspose": lambda w: np.rot90(w, 2).transpose(1, 0, 2),
}
# view point (x, y) -> window point, theta' before the wrap
_POINT = {
    "id": lambda x, y, S, t, hp: (x, y, t),
    "hflip": lambda x, y, S, t, hp: (S - x, y, -t),
    "vflip": lambda x, y, S, t, hp: (x, S - y, -t),
    "rot180": lambda x, y, S, t, hp: (S - x, S - y, t),
    "transpose": lambda x, y, S, t, hp: (y, x, hp - t),
    "rot90": lambda x, y, S, t, hp: (S - y, x, t + hp),
    "rot270": lambda x, y, S, t, hp: (y, S - x, t - hp),
    "antitranspose": lambda x, y, S, t, hp: (S - y, S - x, hp - t),
}


def view_pixels(win, name):
    """[S, S, 3] window -> the view's pixels (a numpy view)."""
    return _PIXELS[name](win)


def np_window(img, x0, y0, S):
    """The S x S x 3 uint8 window at (x0, y0): the scene crop, 114 outside the scene."""
    win = np.full((S, S, 3), 114, dtype=np.uint8)
    part = img[y0:y0 + S, x0:x0 + S]
    win[:part.shape[0], :part.shape[1]] = part
    return win


def np_cut_view(img, x0, y0, S, name):
    """The network input of a view: view(win)[:, :, ::-1] / 255 as [3, S, S] fp32."""
    v = view_pixels(np_window(img, x0, y0, S), name)
    return np.ascontiguousarray((v[:, :, ::-1].astype(f32) / f32(255)).transpose(2, 0, 1))


def point_map(name, x, y, S):
    """view point -> window point in the dtype of x / y (float64 for the geometry checks)."""
    px, py, _ = _POINT[name](x, y, S, 0.0, 0.0)
    return px, py


def map_rows(rows, name, S):
    """fp32 restatement of the collect kernel's inverse map: rows [n, >= 5] (x, y, w, h, theta, ...) of a view -> a copy with x, y,
    theta in the window; one fp32 operation per step, theta' once through norm_angle's two selects for the six views that change it."""
    r = np.array(rows, dtype=f32, copy=True)
    x, y, t = r[:, 0].copy(), r[:, 1].copy(), r[:, 4].copy()
    px, py, tt = _POINT[name](x, y, f32(S), t, HALF_PI)
    tt = np.asarray(tt, dtype=f32)
    if name not in ("id", "rot180"):
        tt = np.where(tt >= HALF_PI, tt - PI, tt).astype(f32)
        tt = np.where(tt < -HALF_PI, tt + PI, tt).astype(f32)
    assert np.asarray(px).dtype == f32 and tt.dtype == f32
    r[:, 0], r[:, 1], r[:, 4] = px, py, tt
    return r


def polygon(rows):
    """(x, y, w, h, theta) rows -> [n, 4, 2] float64 vertices by the oracle's xywha2xyxyxyxy."""
    return ref_data.xywha2xyxyxyxy(torch.from_numpy(np.asarray(rows, dtype=np.float32)[:, :5].copy())).numpy().astype(np.float64)


def polygon_gap(rows, name, S):
    """Largest distance (px) between the vertex set of the mapped box and the mapped vertex set of the view's box."""
    a = polygon(map_rows(rows, name, S))
    p = polygon(rows)
    bx, by = point_map(name, p[:, :, 0], p[:, :, 1], float(S))
    b = np.stack([bx, by], -1)
    d = np.linalg.norm(a[:, :, None, :] - b[:, None, :, :], axis=-1)          # [n, 4, 4]
    return float(max(d.min(2).max(), d.min(1).max())) if len(a) else 0.0


def shift_rows(rows, x0, y0, rate):
    """The collect kernel's shift: ((x + x0) / rate, (y + y0) / rate, w / rate, h / rate, rest unchanged), fp32."""
    r = np.array(rows, dtype=f32, copy=True)
    q = f32(rate)
    r[:, 0] = (r[:, 0] + f32(x0)) / q
    r[:, 1] = (r[:, 1] + f32(y0)) / q
    r[:, 2] = r[:, 2] / q
    r[:, 3] = r[:, 3] / q
    return r


def oracle_merge(entries, rates, S, dets, nums, mk, nc, thr, gt, max_nms, max_det):
    """entries [(rate_index, x0, y0, view)]: inverse view map and fp32 shift of every entry's rows, per-class oracle NMS over the
    max_nms best candidates (score desc, slot asc), final order (score desc, slot asc) capped at max_det -> rows [n, 7]."""
    rows, slots = [], []
    for e, (ri, x0, y0, name) in enumerate(entries):
        n = int(nums[e])
        if n:
            rows.append(shift_rows(map_rows(dets[e, :n], name, S), x0, y0, rates[ri]))
            slots.extend(e * mk + j for j in range(n))
    rows = np.concatenate(rows).astype(f32) if rows else np.zeros((0, 7), f32)
    slots = np.array(slots, dtype=np.int64)
    kept = []
    for c in range(nc):
        idx = np.nonzero(rows[:, 6] == c)[0]
        o = np.array(sorted(idx, key=lambda i: (-rows[i, 5], slots[i]))[:max_nms], dtype=np.int64)
        if len(o) == 0:
            continue
        b = rows[o, :5].copy()
        b[:, 4] = b[:, 4] / f32(np.pi) * f32(180.0)
        kept.extend(o[oracle.nms_rotated(b, rows[o, 5], thr, gt)])
    kept = sorted(kept, key=lambda i: (-rows[i, 5], slots[i]))[:max_det]
    return rows[np.array(kept, dtype=np.int64)].reshape(-1, 7)
