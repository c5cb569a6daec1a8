"""DOTA-protocol evaluation restated in float64 numpy (csrc/evaluate.hip: ryolo_dota_match, ryolo_ap_voc; include/ryolo.h states the rule).

  rect_corners     (x, y, w, h, theta) float32 rows -> corners in float64, h along x before the rotation
  prep_labels      quad or its rectangle, orientation normalised, area, bounds
  clip_area        Sutherland-Hodgman over arrays of pairs: at most 8 vertices, the kernel's statements in the kernel's order
  clip_area_exact  the same walk for ONE pair over any number type (fractions.Fraction: the exact value)
  match            status / best IoU / best label / npos of one scene, closed form (owner = smallest index), and its decision gaps
  ap_voc           voc07 / voc12 AP per class and threshold
  make_scene       the generated cases of the tests (tests/scene_eval_ref.make_scene plus quads, difficult flags, bad classes)

Only cos and sin differ between this file and the kernel (numpy's against the device's, an ulp or two); +, -, *, / are IEEE on both sides and
the file is compiled without contraction.  That is why a case must keep its DECISION GAPS: `gap_thr`, the smallest |IoU - thr[k]| over all
(detection, best label) pairs, and `gap_top2`, the smallest difference between a detection's largest IoU and its largest IoU with a label of
OTHER geometry.  Labels with bit-identical vertices tie exactly on both sides and the first in order wins, and a detection whose largest IoU
is 0 has status 0 whichever label is called its best, so neither is a decision rounding could flip; they do not enter gap_top2."""
import numpy as np

from tests import scene_eval_ref as SR

EPS = 2.220446049250313e-16
GRID11 = np.arange(0., 1.1, 0.1)


def rect_corners(b):
    b = np.asarray(b, np.float32).reshape(-1, 5).astype(np.float64)
    x, y, hy, hx, th = b[:, 0], b[:, 1], b[:, 2] / 2.0, b[:, 3] / 2.0, b[:, 4]
    c, s = np.cos(th)[:, None], np.sin(th)[:, None]
    dx, dy = np.stack([-hx, hx, hx, -hx], 1), np.stack([-hy, -hy, hy, hy], 1)
    return np.stack([x[:, None] + (dx * c + dy * s), y[:, None] + (dy * c - dx * s)], 2)


def fan(P, n):
    """Twice the signed area of the first n vertices of P [N, K, 2] as a fan around vertex 0, terms added in ascending order."""
    s = np.zeros(len(P))
    x0, y0 = P[:, 0, 0], P[:, 0, 1]
    for j in range(1, P.shape[1] - 1):
        t = (P[:, j, 0] - x0) * (P[:, j + 1, 1] - y0) - (P[:, j + 1, 0] - x0) * (P[:, j, 1] - y0)
        s = np.where(j + 1 < n, s + t, s)
    return s


def prep_labels(quads, rects):
    """quads [nl, 8] (NaN rows: none), rects [nl, 5] -> (V [nl, 4, 2] counter-clockwise, area [nl], bounds [nl, 4] = min x, max x, min y,
    max y (empty for a label without finite vertices), used_quad bool [nl])."""
    q = np.asarray(quads, np.float32).reshape(-1, 4, 2).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        f, g = np.roll(q, -1, 1), np.roll(q, -2, 1)
        cr = (f[..., 0] - q[..., 0]) * (g[..., 1] - f[..., 1]) - (f[..., 1] - q[..., 1]) * (g[..., 0] - f[..., 0])
        quad = np.isfinite(q).all((1, 2)) & ((cr > 0).all(1) | (cr < 0).all(1))
        V = np.where(quad[:, None, None], q, rect_corners(rects))
        live = np.isfinite(V).all((1, 2))
        s = fan(V, 4)
        V[s < 0] = V[s < 0][:, [0, 3, 2, 1]]
        bounds = np.stack([V[..., 0].min(1), V[..., 0].max(1), V[..., 1].min(1), V[..., 1].max(1)], 1)
    bounds[~live] = (np.inf, -np.inf, np.inf, -np.inf)
    return V, 0.5 * np.abs(s), bounds, quad


def clip_area(S, Q):
    """Area of S[p] (any orientation) inside Q[p] (counter-clockwise), S, Q [N, 4, 2]."""
    N = len(S)
    r = np.arange(N)
    P, n = np.zeros((N, 8, 2)), np.full(N, 4)
    P[:, :4] = S
    for e in range(4):
        a, b = Q[:, e], Q[:, (e + 1) & 3]
        ex, ey = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
        d = ex[:, None] * (P[:, :, 1] - a[:, 1, None]) - ey[:, None] * (P[:, :, 0] - a[:, 0, None])
        last = np.maximum(n - 1, 0)
        pr, prd = P[r, last], d[r, last]
        O, m = np.zeros((N, 8, 2)), np.zeros(N, np.int64)
        for j in range(8):
            act, ic = j < n, d[:, j] >= 0
            with np.errstate(invalid="ignore", divide="ignore"):
                u = prd / (prd - d[:, j])
                cut = pr + (P[:, j] - pr) * u[:, None]
            w = act & (ic != (prd >= 0)) & (m < 8)
            O[r[w], m[w]] = cut[w]
            m[w] += 1
            w = act & ic & (m < 8)
            O[r[w], m[w]] = P[w, j]
            m[w] += 1
            pr, prd = P[:, j], d[:, j]
        P, n = O, m
    return 0.5 * np.abs(fan(P, n))


def clip_area_exact(S, Q, num=float):
    """One pair, the same walk in the number type `num`; Q in either orientation (normalised here as prep_labels does)."""
    S = [(num(x), num(y)) for x, y in S]
    Q = [(num(x), num(y)) for x, y in Q]

    def fan1(P):
        s = num(0)
        for j in range(1, len(P) - 1):
            s = s + ((P[j][0] - P[0][0]) * (P[j + 1][1] - P[0][1]) - (P[j + 1][0] - P[0][0]) * (P[j][1] - P[0][1]))
        return s
    if fan1(Q) < 0:
        Q = [Q[0], Q[3], Q[2], Q[1]]
    P = list(S)
    for e in range(4):
        a, b = Q[e], Q[(e + 1) & 3]
        ex, ey = b[0] - a[0], b[1] - a[1]
        d = [ex * (p[1] - a[1]) - ey * (p[0] - a[0]) for p in P]
        O = []
        for j in range(len(P)):
            pr, prd = P[j - 1], d[j - 1]
            if (d[j] >= 0) != (prd >= 0):
                u = prd / (prd - d[j])
                O.append((pr[0] + (P[j][0] - pr[0]) * u, pr[1] + (P[j][1] - pr[1]) * u))
            if d[j] >= 0:
                O.append(P[j])
        P = O[:8]
    return abs(fan1(P)) / 2 if len(P) >= 3 else num(0), abs(fan1(S)) / 2, abs(fan1(Q)) / 2


def iou_exact(S, Q, num=float):
    inter, a, b = clip_area_exact(S, Q, num)
    den = a + b - inter
    return num(0) if den <= 0 else inter / den


def _valid_class(cls, nc):
    with np.errstate(invalid="ignore"):
        return (cls >= 0) & (cls < nc) & (cls == np.floor(cls))


def iou_table(dets, V, area, bounds, same):
    """IoU [n, nl] in float64 for the pairs marked in `same`, 0 elsewhere."""
    n, nl = same.shape
    D = rect_corners(dets[:, :5])
    with np.errstate(invalid="ignore"):
        live = np.isfinite(D).all((1, 2))
        db = np.stack([D[..., 0].min(1), D[..., 0].max(1), D[..., 1].min(1), D[..., 1].max(1)], 1)
        ad = 0.5 * np.abs(fan(D, 4))
        apart = (db[:, None, 1] < bounds[None, :, 0]) | (bounds[None, :, 1] < db[:, None, 0]) | \
                (db[:, None, 3] < bounds[None, :, 2]) | (bounds[None, :, 3] < db[:, None, 2])
    M = np.zeros((n, nl))
    i, t = np.nonzero(same & live[:, None] & ~apart)
    if len(i):
        inter = clip_area(D[i], V[t])
        den = ad[i] + area[t] - inter
        with np.errstate(invalid="ignore", divide="ignore"):
            M[i, t] = np.where(den <= 0, 0.0, inter / den)
    return M


def match(dets, quads, rects, classes, difficult, nc, iouv):
    """One scene -> dict(status uint8 [n, niou], best_iou float64 [n] (-1: none), best_t int64 [n] (caller's label order, -1: none),
    npos int64 [nc], iou [n, nl], gap_thr, gap_top2).  quads may be None (boxes only: rects are the labels)."""
    dets = np.asarray(dets, np.float32).reshape(-1, 7)
    lc = np.asarray(classes, np.float64).reshape(-1)
    nl, n = len(lc), len(dets)
    rects = np.asarray(rects, np.float32).reshape(nl, 5)
    quads = np.full((nl, 8), np.nan, np.float32) if quads is None else np.asarray(quads, np.float32).reshape(nl, 8)
    hard = np.zeros(nl, bool) if difficult is None else np.asarray(difficult).reshape(-1) != 0
    thr = np.asarray(iouv, np.float32).astype(np.float64)
    V, area, bounds, _ = prep_labels(quads, rects)
    cls = dets[:, 6].astype(np.float64)
    same = _valid_class(cls, nc)[:, None] & (cls[:, None] == lc[None, :])
    M = iou_table(dets, V, area, bounds, same)
    Mm = np.where(same, M, -1.0)
    r = np.arange(n)
    if nl:
        best_t = Mm.argmax(1)                                         # first maximum
        best_iou = Mm[r, best_t]
        best_t = np.where(same.any(1), best_t, -1)
    else:
        best_t, best_iou = np.full(n, -1, np.int64), np.full(n, -1.0)
    has = best_t >= 0
    status = np.zeros((n, len(thr)), np.uint8)
    for k in range(len(thr)):
        cand = has & (best_iou > thr[k])
        owner = np.full(max(nl, 1), SR.INT_MAX, np.int64)
        np.minimum.at(owner, best_t[cand], r[cand])
        bt = np.where(has, best_t, 0)
        ignored = cand & (hard[bt] if nl else False)
        status[:, k] = np.where(ignored, 2, np.where(cand & (owner[bt] == r), 1, 0))
    ok = _valid_class(lc, nc)
    npos = np.bincount(lc[ok & ~hard].astype(np.int64), minlength=nc).astype(np.int64)
    gap_thr = float(np.abs(best_iou[has, None] - thr[None, :]).min()) if has.any() else np.inf
    gap_top2 = np.inf
    for i in np.nonzero(has & (best_iou > 0))[0]:
        other = same[i] & ~(V == V[best_t[i]]).all((1, 2))
        if other.any():
            gap_top2 = min(gap_top2, float(best_iou[i] - M[i, other].max()))
    return {"status": status, "best_iou": best_iou, "best_t": best_t, "npos": npos, "iou": M, "gap_thr": gap_thr, "gap_top2": gap_top2}


def voc07(rec, prec):
    ap = 0.0
    for t in GRID11:
        p = prec[rec >= t].max() if (rec >= t).any() else 0.0
        ap = ap + p / 11.0
    return ap


def voc12(rec, prec):
    mrec, mpre = np.concatenate([[0.0], rec, [1.0]]), np.concatenate([[0.0], prec, [0.0]])
    for i in range(len(mpre) - 1, 0, -1):
        mpre[i - 1] = max(mpre[i - 1], mpre[i])
    ap = 0.0
    for i in np.nonzero(mrec[1:] != mrec[:-1])[0]:
        ap = ap + (mrec[i + 1] - mrec[i]) * mpre[i + 1]
    return ap


def ap_voc(status, conf, pcls, npos, nc, metric):
    """-> (ap float64 [nc, niou], NaN for classes without positives; n_pred int64 [nc])."""
    status = np.asarray(status, np.uint8)
    conf, pcls = np.asarray(conf, np.float32), np.asarray(pcls, np.float32)
    status = status[:, None] if status.ndim == 1 else status
    fn = {"voc07": voc07, "voc12": voc12}[metric]
    order = np.argsort(-conf, kind="stable")
    ap, n_pred = np.full((nc, status.shape[1]), np.nan), np.zeros(nc, np.int64)
    for c in range(nc):
        rows = order[pcls[order] == c]
        n_pred[c] = len(rows)
        if npos[c] <= 0:
            continue
        for k in range(status.shape[1]):
            st = status[rows, k]
            st = st[st != 2]
            tpc, fpc = np.cumsum(st == 1).astype(np.float64), np.cumsum(st != 1).astype(np.float64)
            ap[c, k] = fn(tpc / float(npos[c]), tpc / np.maximum(tpc + fpc, EPS))
    return ap, n_pred


def mean_ap(ap, npos):
    keep = np.asarray(npos) > 0
    return ap[keep].mean(0) if keep.any() else np.full(ap.shape[1], np.nan)


# ---------------------------------------------------------------------------------------------- cases
def box_quads(boxes, seed, warp=0.12, clockwise=0.5, nonconvex=0.06):
    """Quadrilaterals around boxes [nl, 5]: the box's corners with every vertex moved by up to `warp` of the short side (still convex),
    a share walked clockwise, a share made non-convex (one vertex pulled through the opposite diagonal).  float32 [nl, 8]."""
    g = np.random.default_rng(seed)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 5)
    C = rect_corners(boxes)
    short = np.minimum(boxes[:, 2], boxes[:, 3]).astype(np.float64)
    C = C + g.uniform(-1, 1, C.shape) * (warp * short)[:, None, None]
    flip = g.random(len(C)) < clockwise
    C[flip] = C[flip][:, [0, 3, 2, 1]]
    bad = np.nonzero(g.random(len(C)) < nonconvex)[0]
    ctr = C[bad].mean(1)
    C[bad, 1] = ctr + 0.5 * (C[bad, 3] - ctr)                        # vertex 1 moves to vertex 3's side of the centre: a dart
    return C.reshape(-1, 8).astype(np.float32), bad


def make_scene(seed, per_class, ndet, hard=0.25, quads=True, square=False):
    """tests/scene_eval_ref.make_scene plus label quads, difficult flags and detections of classes NaN and nc; square: every box gets
    h = w.  -> dict(dets, boxes, quads (or None), classes, difficult uint8)."""
    dets, boxes, classes = SR.make_scene(seed, per_class, ndet if ndet else 3 * int(sum(per_class)))
    dets = dets if ndet else dets[:0]                                 # ndet = 0: the labels of a scene, no detection
    if square:
        dets[:, 3], boxes[:, 3] = dets[:, 2], boxes[:, 2]
    g = np.random.default_rng(seed + 1000)
    nl = len(classes)
    difficult = (g.random(nl) < hard).astype(np.uint8)
    q = None
    if quads and nl:
        q, _ = box_quads(boxes, seed + 2000)
        big = np.nonzero(classes == np.argmax(per_class))[0]
        if len(big) > 1:
            q[big[1]] = q[big[0]]                                     # the duplicate label stays a duplicate
    elif quads:
        q = np.zeros((0, 8), np.float32)
    if len(dets) > 8:
        dets[len(dets) // 2, 6] = np.nan
        dets[len(dets) // 3, 6] = len(per_class)
    return {"dets": dets, "boxes": boxes, "quads": q, "classes": classes, "difficult": difficult}


# name -> (seed, labels per class, detections, quads, share of difficult labels, thresholds, the decision gap the case must keep).
# "mixed" is the scene of the GPU tests (every prefix of it keeps at least the gaps of the whole), "boxes" the same labels as [nl, 5]
# boxes, "cross" and "square" the cases compared with ryolo_scene_match: its float pair function and the float64 clip may differ in the
# last float32 digits, hence the wider gap ("square": every box has h = w, see tests/test_gpu_dota_eval.py).
GPU_CASES = {"mixed": (190, (130, 0, 1, 40, 29), 360, True, 0.25, (0.5, 0.75, 0.9), 1e-9),
             "boxes": (190, (130, 0, 1, 40, 29), 360, False, 0.25, (0.5, 0.75, 0.9), 1e-9),
             "cross": (191, (130, 0, 1, 40, 29), 360, False, 0.0, (0.5,), 1e-4),
             "square": (192, (130, 0, 1, 40, 29), 360, False, 0.0, (0.5,), 1e-4)}
GPU_NC = 5


def gpu_case(name):
    """-> (scene dict of make_scene, nc, iouv, gap)."""
    seed, per_class, ndet, quads, hard, iouv, gap = GPU_CASES[name]
    return make_scene(seed, per_class, ndet, hard=hard, quads=quads, square=name == "square"), GPU_NC, iouv, gap
