"""Numpy / pure-Python restatement of object-level copy-paste (datasets/copy_paste.py, csrc/copypaste.hip): the draw sequence, the
destination quads and bounding boxes, the pixel rule (warp_perspective_numpy under a mask, later paste wins) and the label rule (a
literal fp64 Sutherland-Hodgman clip), with the operation order include/ryolo.h fixes, so that the device results can be compared bit
for bit.  The reference has no such stage; these semantics are this project's and this file is what pins them.  Python floats are IEEE
doubles and every operation below is a single rounded one, which is what the kernels are built to do (-ffp-contract=off)."""
import contextlib
import math

import numpy as np

from oracle import ref_data

FILL = 114
MAXV = 20


def make_item(src, SH, SW, slot, cls, quad, M, Minv):
    """An item as a dict; `src` names the scene (the device table holds its byte offset instead)."""
    return dict(src=src, SH=int(SH), SW=int(SW), slot=int(slot), cls=np.float32(cls), quad=np.asarray(quad, dtype=np.float32).reshape(8),
                M=[float(v) for v in M], Minv=[float(v) for v in Minv])


def first_table(items, B):
    slots = np.asarray([it["slot"] for it in items], dtype=np.int64)
    assert (np.diff(slots) >= 0).all(), "items are sorted by slot"
    return np.searchsorted(slots, np.arange(B + 1)).astype(np.int32)


def item_valid(items, j, first, B):
    s = items[j]["slot"]
    if not 0 <= s < B:
        return False
    return bool(first[s] <= j < first[s + 1] <= len(items) and items[j]["SH"] > 0 and items[j]["SW"] > 0)


# ---------------------------------------------------------------------------------------------- geometry
def shoelace(pts):
    s = 0
    n = len(pts)
    for k in range(n):
        xk, yk = pts[k]
        xj, yj = pts[(k + 1) % n]
        s = s + (xk * yj - xj * yk)
    return s


def dest_quad(item):
    """x' = M0 x + M1 y + M2, y' = M3 x + M4 y + M5 in double, left to right, rounded to float."""
    M, q = item["M"], item["quad"]
    out = np.zeros(8, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for v in range(4):
            x, y = float(q[2 * v]), float(q[2 * v + 1])
            out[2 * v] = np.float32(M[0] * x + M[1] * y + M[2])
            out[2 * v + 1] = np.float32(M[3] * x + M[4] * y + M[5])
    return out


def quad_pts(dq):
    return [(float(dq[2 * v]), float(dq[2 * v + 1])) for v in range(4)]


def quad_sign(dq):
    """(has finite vertices and a non-zero shoelace sum, +1.0 / -1.0)."""
    pts = quad_pts(dq)
    fin = all(math.isfinite(x) and math.isfinite(y) for x, y in pts)
    s = shoelace(pts)
    return fin and (s > 0 or s < 0), (1.0 if s > 0 else -1.0)


def prepare(items, first, B, S):
    """(dq float32 [np, 8], bbox int32 [np, 4] = (x0, y0, x1, y1), zero when the item is not live or misses the canvas)."""
    dq = np.zeros((len(items), 8), dtype=np.float32)
    bbox = np.zeros((len(items), 4), dtype=np.int32)
    for j, it in enumerate(items):
        dq[j] = dest_quad(it)
        live, _ = quad_sign(dq[j])
        if not (live and item_valid(items, j, first, B)):
            continue
        xs, ys = [float(v) for v in dq[j][0::2]], [float(v) for v in dq[j][1::2]]
        x0 = int(min(max(math.ceil(min(xs)), 0.0), float(S)))
        x1 = int(min(max(math.floor(max(xs)) + 1.0, 0.0), float(S)))
        y0 = int(min(max(math.ceil(min(ys)), 0.0), float(S)))
        y1 = int(min(max(math.floor(max(ys)) + 1.0, 0.0), float(S)))
        if x0 < x1 and y0 < y1:
            bbox[j] = (x0, y0, x1, y1)
    return dq, bbox


def edge(a, b, s, p):
    return s * ((b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]))


def inside_mask(dq, S):
    """bool [S, S]: the canvas pixels inside the destination quad (all four edge expressions >= 0), zeros for a quad that is not live."""
    live, sg = quad_sign(dq)
    m = np.zeros((S, S), dtype=bool)
    if not live:
        return m
    pts = quad_pts(dq)
    px, py = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64))
    m[:] = True
    for e in range(4):
        (ax, ay), (bx, by) = pts[e], pts[(e + 1) & 3]
        m &= sg * ((bx - ax) * (py - ay) - (by - ay) * (px - ax)) >= 0.0
    return m


# ---------------------------------------------------------------------------------------------- pixels
@contextlib.contextmanager
def _inverse_is(minv3):
    """warp_perspective_numpy inverts the matrix it is given; the kernel is handed the inverse map in the table.  For the duration of the
    call the inversion returns the table's matrix, so the restatement samples with exactly the doubles the kernel reads."""
    saved = np.linalg.inv
    np.linalg.inv = lambda _: minv3
    try:
        yield
    finally:
        np.linalg.inv = saved


def sample(scene, Minv, S):
    """The S x S canvas sampled from `scene` through the inverse map (Minv; 0 0 1): ryolo_warp_perspective_u8's rule, border 114."""
    minv3 = np.array([Minv[0:3], Minv[3:6], [0.0, 0.0, 1.0]], dtype=np.float64)
    with _inverse_is(minv3):
        return ref_data.warp_perspective_numpy(np.ascontiguousarray(scene), np.eye(3), (S, S), border=FILL)


def paste_pixels(scenes, items, first, B, final):
    """final uint8 [B, S, S, 3] -> (pasted copy, union of masks bool [B, S, S], cover int [B, S, S] = items a pixel is inside)."""
    S = final.shape[1]
    dq, bbox = prepare(items, first, B, S)
    out = final.copy()
    union = np.zeros(final.shape[:3], dtype=bool)
    cover = np.zeros(final.shape[:3], dtype=np.int64)
    for j, it in enumerate(items):
        if not item_valid(items, j, first, B) or not bbox[j].any():
            continue
        m = inside_mask(dq[j], S)
        x0, y0, x1, y1 = bbox[j]
        box = np.zeros_like(m)
        box[y0:y1, x0:x1] = True
        assert not (m & ~box).any(), "a pixel inside the quad lies inside its bounding box"
        if not m.any():
            continue
        out[it["slot"]][m] = sample(scenes[it["src"]], it["Minv"], S)[m]              # in table order: a later item overwrites
        union[it["slot"]] |= m
        cover[it["slot"]] += m
    return out, union, cover


# ---------------------------------------------------------------------------------------------- labels
def clip_edge(pts, a, b, s):
    out = []
    n = len(pts)
    for k in range(n):
        p, q = pts[k], pts[(k + 1) % n]
        da, db = edge(a, b, s, p), edge(a, b, s, q)
        ain, bin_ = da >= 0, db >= 0
        if ain and len(out) < MAXV:
            out.append(p)
        if ain != bin_ and len(out) < MAXV:
            t = da / (da - db)
            out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def clip_ratio(row_pts, quad, arith=float):
    """|shoelace(clip(row, quad))| / |shoelace(row)| (None when the row has no area or the quad no sign); arith = float: the kernel's fp64
    operations one by one, fractions.Fraction: exact."""
    row_pts = [(arith(x), arith(y)) for x, y in row_pts]
    quad = [(arith(x), arith(y)) for x, y in quad]
    area = abs(shoelace(row_pts))
    sq = shoelace(quad)
    if not area > 0 or not (sq > 0 or sq < 0):
        return None
    s = arith(1) if sq > 0 else arith(-1)
    pts = row_pts
    for e in range(4):
        pts = clip_edge(pts, quad[e], quad[(e + 1) & 3], s)
    return abs(shoelace(pts)) / area


def _occluded(row8, slot, items, dq, lo, hi, occ_thr, first, B):
    pts = quad_pts(row8)
    with np.errstate(all="ignore"):
        area = abs(shoelace(pts))
        if not area > 0:
            return False
        for k in range(max(lo, 0), min(hi, len(items))):
            if items[k]["slot"] != slot or not item_valid(items, k, first, B) or not quad_sign(dq[k])[0]:
                continue
            r = clip_ratio(pts, quad_pts(dq[k]))
            if r is not None and r >= occ_thr:
                return True
    return False


def paste_labels(targets10, items, first, B, S, occ_thr):
    """[nt, 10] -> [nt + np, 10] float32 (NaN coordinates for buried rows)."""
    tg = np.asarray(targets10, dtype=np.float32).reshape(-1, 10)
    nt, n = len(tg), len(items)
    dq, _ = prepare(items, first, B, S)
    out = np.zeros((nt + n, 10), dtype=np.float32)
    for i in range(nt):
        out[i] = tg[i]
        if tg[i, 0] >= 0 and tg[i, 0] < np.float32(B):
            slot = int(tg[i, 0])
            if _occluded(tg[i, 2:], slot, items, dq, int(first[slot]), int(first[slot + 1]), occ_thr, first, B):
                out[i, 2:] = np.nan
    for j, it in enumerate(items):
        out[nt + j, 1] = it["cls"]
        if not item_valid(items, j, first, B):
            out[nt + j, 0] = 0.0
            out[nt + j, 2:] = np.nan
            continue
        out[nt + j, 0] = np.float32(it["slot"])
        out[nt + j, 2:] = dq[j]
        if _occluded(dq[j], it["slot"], items, dq, j + 1, int(first[it["slot"] + 1]), occ_thr, first, B):
            out[nt + j, 2:] = np.nan
    return out


def compose(scenes, items, B, final, targets10, occ_thr):
    """The three stages: (pasted canvases, targets10 [nt + np, 10], union of masks, cover counts)."""
    first = first_table(items, B)
    out, union, cover = paste_pixels(scenes, items, first, B, final)
    return out, paste_labels(targets10, items, first, B, final.shape[1], occ_thr), union, cover


# ---------------------------------------------------------------------------------------------- the draws
def strictly_convex(quad):
    q = [float(v) for v in quad]
    if not all(math.isfinite(v) for v in q):
        return False
    pts = [(q[2 * k], q[2 * k + 1]) for k in range(4)]
    cr = []
    for e in range(4):
        a, b, c = pts[e], pts[(e + 1) % 4], pts[(e + 2) % 4]
        cr.append((b[0] - a[0]) * (c[1] - b[1]) - (b[1] - a[1]) * (c[0] - b[0]))
    return all(v > 0 for v in cr) or all(v < 0 for v in cr)


def bank_of(scene_labels, scenes):
    """scene_labels {scene: (polys [n, 8], classes [n])} -> {class: [(scene, label index, quad)]}, scenes ascending, file order."""
    bank = {}
    for s in sorted(set(scenes)):
        polys, cls = scene_labels[s]
        for i in range(len(cls)):
            if strictly_convex(polys[i]):
                bank.setdefault(float(cls[i]), []).append((s, i, np.asarray(polys[i], dtype=np.float32)))
    return bank


def class_counts(scene_labels):
    counts = {}
    for s in scene_labels:
        for c in np.asarray(scene_labels[s][1]).tolist():
            counts[float(c)] = counts.get(float(c), 0) + 1
    return counts


def matrices(quad, angle, scale, cx, cy):
    q = [float(v) for v in quad]
    mx = (q[0] + q[2] + q[4] + q[6]) / 4.0
    my = (q[1] + q[3] + q[5] + q[7]) / 4.0
    ang = angle * math.pi / 180.0
    a, b = scale * math.cos(ang), scale * math.sin(ang)
    ia, ib = a / (scale * scale), b / (scale * scale)
    return ((a, b, cx - a * mx - b * my, -b, a, cy + b * mx - a * my), (ia, -ib, mx - ia * cx + ib * cy, ib, ia, my - ib * cx - ia * cy))


def draw(rng, B, S, bank, counts, unit_scale, p=0.5, max_objects=8, alpha=0.5, scale=(0.75, 1.25), rotate=180.0, min_side=4.0):
    """Draw order per slot: the coin; n; per object class, object, angle, scale, cx, cy; the skip test comes after the draws.
    -> [(slot, scene, label index, class, quad, angle, scale, cx, cy)]."""
    classes = sorted(c for c in bank if len(bank[c]))
    out = []
    if not classes:
        return out
    for slot in range(B):
        coin = rng.random()
        if not coin < p:
            continue
        n = rng.randint(1, max_objects)
        for _ in range(n):
            w = [float(counts[c]) ** -alpha for c in classes]
            total = 0.0
            for v in w:
                total += v
            x = rng.random() * total
            acc, cls = 0.0, classes[-1]
            for c, v in zip(classes, w):
                acc += v
                if x < acc:
                    cls = c
                    break
            scene, label, quad = bank[cls][rng.randrange(len(bank[cls]))]
            angle = rng.uniform(-rotate, rotate)
            sc = rng.uniform(scale[0], scale[1]) * unit_scale[slot]
            q = [float(v) for v in quad]
            mx = (q[0] + q[2] + q[4] + q[6]) / 4.0
            my = (q[1] + q[3] + q[5] + q[7]) / 4.0
            rad = max(math.hypot(q[2 * k] - mx, q[2 * k + 1] - my) for k in range(4))
            side = min(math.hypot(q[2 * ((k + 1) % 4)] - q[2 * k], q[2 * ((k + 1) % 4) + 1] - q[2 * k + 1]) for k in range(4))
            r = sc * rad
            cx = r + (S - 2.0 * r) * rng.random()
            cy = r + (S - 2.0 * r) * rng.random()
            if 2.0 * r > S or sc * side < min_side:
                continue
            out.append((slot, scene, label, cls, quad, angle, sc, cx, cy))
    return out


def items_of(drawn, scene_shapes):
    out = []
    for slot, scene, _, cls, quad, angle, sc, cx, cy in drawn:
        M, Minv = matrices(quad, angle, sc, cx, cy)
        H, W = scene_shapes[scene]
        out.append(make_item(scene, H, W, slot, cls, quad, M, Minv))
    return out
