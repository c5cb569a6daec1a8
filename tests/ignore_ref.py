"""Numpy restatement of the ignore regions of the fused loss and of the loader that feeds them (not a test module).

  * the CELL RULE of include/ryolo.h (ryolo_loss): which cells of a scale a table of ignore rows covers — float64, operation by operation,
    with the one fp32 multiply that makes the grid coordinates;
  * what ignoring does to the objectness term, in float64;
  * the SELECTION RULE of SceneDataset(ignore=Ignore(...)): which labels of a window become ignore rows (IoF through tests/scene_ref.py);
  * the VERTEX PATH of an ignore row on the non-mosaic paths: window shift, resize, letterbox pad, warp matrix, flip, division by the
    canvas side — float64 after the fp32 shift — and, for counting the rows of a mosaic batch, the stage's mean-vertex filters in fp32.
"""
import numpy as np

from tests import scene_ref as SR


# ---------------------------------------------------------------------------------------------- the cell rule
def grid_quad(row, gs):
    """Grid coordinates of a row's quad at grid size gs: fl32(coordinate * (float)gs), promoted to float64.  -> (x[4], y[4])."""
    c = np.asarray(row, dtype=np.float32).reshape(9)[1:]
    with np.errstate(over="ignore", invalid="ignore"):
        v = (c * np.float32(gs)).astype(np.float64)
    return v[0::2], v[1::2]


def shoelace(x, y):
    """sum of (x_k y_k+1 - x_k+1 y_k) in vertex order, left to right, float64, every operation rounded on its own."""
    s = np.float64(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(4):
            j = (k + 1) % 4
            s = s + (x[k] * y[j] - x[j] * y[k])
    return s


def row_live(row, batch, gs):
    """The LIVE rule: image in [0, batch) after truncation (a NaN image is not live), eight finite coordinates, a shoelace sum that is
    neither 0 nor NaN on the grid coordinates of this scale."""
    r = np.asarray(row, dtype=np.float32).reshape(9)
    img = r[0]
    if not (img > np.float32(-1.0) and img < np.float32(batch)):
        return False
    if not np.all(np.isfinite(r[1:])):
        return False
    s = shoelace(*grid_quad(r, gs))
    return bool(s > 0.0 or s < 0.0)


def row_cells(row, gs):
    """bool [gs, gs] (gj, gi): cells whose centre (gi + 0.5, gj + 0.5) is INSIDE the quad of a live row — inside the bounding box and on
    the inner side (>= 0: a centre on an edge is inside) of each of the four edges, the sign taken from the shoelace sum."""
    x, y = grid_quad(row, gs)
    sg = 1.0 if shoelace(x, y) > 0.0 else -1.0
    out = np.zeros((gs, gs), dtype=bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for gj in range(gs):
            for gi in range(gs):
                cx, cy = np.float64(gi) + 0.5, np.float64(gj) + 0.5
                ok = cx >= x.min() and cx <= x.max() and cy >= y.min() and cy <= y.max()
                for k in range(4):
                    j = (k + 1) % 4
                    e = sg * ((x[j] - x[k]) * (cy - y[k]) - (y[j] - y[k]) * (cx - x[k]))
                    ok = ok and bool(e >= 0.0)
                out[gj, gi] = ok
    return out


def covered(ignore, batch, gs):
    """bool [batch, gs, gs]: cells whose centre lies inside some live row of their image."""
    out = np.zeros((batch, gs, gs), dtype=bool)
    for row in np.asarray(ignore, dtype=np.float32).reshape(-1, 9):
        if row_live(row, batch, gs):
            out[int(row[0])] |= row_cells(row, gs)
    return out


def matched_mask(records, batch, na, gs):
    """bool [batch, na, gs, gs] from the match records of one scale (criterion.debug_matches(): b, a, gj, gi in columns 0..3)."""
    m = np.zeros((batch, na, gs, gs), dtype=bool)
    rec = np.asarray(records).reshape(-1, 8)
    m[rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]] = True
    return m


def ignored(ignore, batch, na, gs, records):
    """bool [batch, na, gs, gs]: the IGNORED cells of a scale — covered, for every anchor alike, and owned by no match."""
    cov = covered(ignore, batch, gs)
    return np.broadcast_to(cov[:, None], (batch, na, gs, gs)) & ~matched_mask(records, batch, na, gs)


# ---------------------------------------------------------------------------------------------- the objectness term
def obj_element(x, gamma=0.0, alpha=0.25):
    """One objectness element against target 0 with pos_weight anything, float64: BCE-with-logits x + softplus(-|x|) + max(-x, 0), inside
    FocalLoss (alpha (1 - alpha for target 0), gamma) when gamma > 0."""
    x = np.asarray(x, dtype=np.float64)
    l = x + np.log1p(np.exp(-np.abs(x))) + np.maximum(-x, 0.0)
    if gamma > 0.0:
        p = 1.0 / (1.0 + np.exp(-x))
        l = l * (1.0 - alpha) * p ** gamma
    return l


def conf_without(conf_plain, obj_gain, logits, masks, gamma=0.0):
    """conf of a call with ignore rows from the conf of the same call without: every ignored cell held target 0 (it is unmatched), so the
    term loses obj_gain * sum over scales of (sum over the scale's ignored cells of obj_element(logit)) / (cells of the scale) —
    the denominator is NOT reduced.  logits[i] [B, na, gs, gs] objectness logits, masks[i] the ignored cells."""
    lost = 0.0
    for x, m in zip(logits, masks):
        lost += float(obj_element(np.asarray(x, dtype=np.float64)[m], gamma).sum()) / m.size
    return float(conf_plain) - obj_gain * lost


def conf_no_targets(obj_gain, logits, masks, gamma=0.0):
    """conf of a call WITHOUT targets (every cell has target 0), in float64: the whole term restated."""
    tot = 0.0
    for x, m in zip(logits, masks):
        tot += float(obj_element(np.asarray(x, dtype=np.float64)[~m], gamma).sum()) / m.size
    return obj_gain * tot


# ---------------------------------------------------------------------------------------------- the loader: which labels become rows
def select(polys, difficult, x0, y0, c, iof_lo, iof_thr, use_difficult):
    """Labels of a scene (float32 [n, 8] scene pixels, difficult flags [n]) against the window (x0, y0, c), in file order ->
    (main, shadow): indices that stay TARGET candidates of the window (IoF >= iof_thr, and not difficult when use_difficult) and indices
    that become IGNORE candidates: IoF >= iof_lo and (IoF < iof_thr or (use_difficult and difficult)).  Both still pass through the stage's
    filters (a row the stage drops is in neither)."""
    polys = np.asarray(polys, dtype=np.float32).reshape(-1, 8)
    difficult = np.asarray(difficult).reshape(-1) != 0
    idx = SR.cull(polys, x0, y0, c)
    _, iof, _ = SR.label_rows(polys[idx], x0, y0, c, iof_thr)
    main, shadow = [], []
    for i, v in zip(idx, iof):
        hard = bool(use_difficult and difficult[i])
        if v >= iof_thr and not hard:
            main.append(int(i))
        if v >= iof_lo and (v < iof_thr or hard):
            shadow.append(int(i))
    return main, shadow


# ---------------------------------------------------------------------------------------------- the loader: where the vertices go
def vertex_path(poly, x0, y0, c, hw, pad, M, flip, S):
    """One label quad (scene pixels) -> the eight normalised coordinates of its ignore row on a NON-mosaic canvas: fp32 shift by the window
    origin, then float64: / c * (w, h) of the resized window, + (padw, padh) of the letterbox, the warp matrix M (3x3, None: none),
    / S, and 1 - x for a left-right flip (bit 0 of flip), 1 - y for an up-down one (bit 1)."""
    q = SR.shift_poly(poly, x0, y0).reshape(8).astype(np.float64)
    h, w = hw
    x = q[0::2] / c * w + pad[1]                                    # pad = (padh, padw), as LabelRow holds it
    y = q[1::2] / c * h + pad[0]
    if M is not None:
        M = np.asarray(M, dtype=np.float64).reshape(3, 3)
        x, y = M[0, 0] * x + M[0, 1] * y + M[0, 2], M[1, 0] * x + M[1, 1] * y + M[1, 2]
    x, y = x / S, y / S
    if flip & 1:
        x = 1.0 - x
    if flip & 2:
        y = 1.0 - y
    out = np.empty(8, dtype=np.float64)
    out[0::2], out[1::2] = x, y
    return out


def stage_keeps(poly, x0, y0, c, hw, border, crop, pad):
    """The filters of ryolo_label_stage on one shadow row (fp32, the kernel's operations): the shifted quad / c * (w, h), its mean vertex
    strictly inside `border` = (x1, x2, y1, y2) when there is one (the visible source rectangle of a mosaic use), then + pad = (padh, padw)
    and the mean strictly inside `crop` (mosaic-9).  True: the row stays finite."""
    f = np.float32
    q = SR.shift_poly(poly, x0, y0).reshape(8)
    h, w = hw
    x, y = q[0::2] / f(c) * f(w), q[1::2] / f(c) * f(h)

    def mean_ok(x, y, b):
        mx, my = (((x[0] + x[1]) + x[2]) + x[3]) / f(4), (((y[0] + y[1]) + y[2]) + y[3]) / f(4)
        return bool(mx > f(b[0]) and mx < f(b[1]) and my > f(b[2]) and my < f(b[3]))

    ok = True
    if border is not None:
        ok = mean_ok(x, y, border)
    x, y = x + f(pad[1]), y + f(pad[0])
    if ok and crop is not None:
        ok = mean_ok(x, y, crop)
    return ok
