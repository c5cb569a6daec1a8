"""Full-scene error breakdown: a numpy restatement of the rule of ryolo_scene_errors (include/ryolo.h states it operation by operation;
csrc/evaluate.hip computes it) over oracle.pairwise_iou_rotated, as scene_eval_ref.owner_rule restates ryolo_scene_match, and the case the
tests run on.

planted_case is scene_eval_ref.case("mixed") (360 detections, 200 labels, 5 classes) with 50 rows planted on randomly drawn labels — 20
copies with only the angle off by +-U(0.35, 0.7) rad, 10 copies written the other way round (h, w, theta + pi/2), 20 copies shifted by 0.6 w
across the short side — after which scores are rounded to 1/64 and the rows stably re-sorted.  The generated scene alone has hardly any
detection that is right in place and size and wrong only in angle, and few that are merely mislocated.

hand_scene is one label and one detection per category with the expected codes and statuses written out by hand, not computed.

errors_rule works on the labels GROUPED BY CLASS (stable), as the kernel sees them: s_t, o_t and the statuses are indices / rows of that
order, and `order` maps them back."""
import numpy as np

import oracle
from tests import scene_eval_ref as R

INT_MAX = R.INT_MAX
CODES = ("BELOW", "TP", "DUP", "CLS", "ANG", "LOC", "BOTH", "BKG")
STATUSES = ("FOUND", "CONFUSED", "MISLOCATED", "MISSED")
EDGES = (32.0 ** 2, 96.0 ** 2)
PLANT_SEED = 112         # of the seeds tried, one where every code and status occurs often enough at conf_thres 0.0 and 0.5 (test_scene_errors_cpu.py)


def planted_case(seed=PLANT_SEED):
    """-> (dets float32 [410, 7] score-descending, boxes float32 [200, 5], classes float32 [200])."""
    dets, boxes, classes = R.case("mixed")
    g = np.random.default_rng(seed)
    rows = []
    for kind, count in (("angle", 20), ("swapped", 10), ("shifted", 20)):
        for t in g.integers(0, len(boxes), count):
            x, y, w, h, th = (float(v) for v in boxes[t])
            if kind == "angle":
                th += float(g.choice([-1.0, 1.0]) * g.uniform(0.35, 0.7))
            elif kind == "swapped":
                w, h, th = h, w, th + np.pi / 2
            else:                                                     # the w axis of (x, y, w, h, theta) runs along (cos, -sin)
                x, y = x + 0.6 * w * np.cos(th), y - 0.6 * w * np.sin(th)
            rows.append([x, y, w, h, th, g.uniform(0.05, 1.0), classes[t]])
    p = np.concatenate([dets, np.array(rows, np.float32)], 0)
    p[:, 5] = np.round(p[:, 5] * 64) / 64
    p = p[np.argsort(-p[:, 5], kind="stable")]
    return np.ascontiguousarray(p), boxes, classes


def hand_scene():
    """One label and one detection per category, 200 px apart; nc = 2, fg 0.5, bg 0.1, conf_thres 0.3.  -> (dets, boxes, classes, the
    expected codes per detection row, the expected statuses per label in the caller's order), both written out by hand."""
    boxes = np.array([[100, 100, 20, 60, 0], [300, 100, 20, 60, 0], [500, 100, 20, 60, 0], [700, 100, 20, 60, 0], [900, 100, 20, 60, 0],
                      [1100, 100, 20, 60, 0], [1500, 100, 20, 60, 0]], np.float32)
    classes = np.array([0, 1, 0, 0, 0, 1, 0], np.float32)
    dets = np.array([
        [100, 100, 20, 60, 0, 0.95, 0],                      # the label itself: TP
        [101, 100, 20, 60, 0, 0.90, 0],                      # the same label again (IoU 19 / 21): DUP
        [300, 100, 20, 60, 0, 0.85, 0],                      # on a label of class 1: CLS
        [500, 100, 20, 60, 0.6, 0.80, 0],                    # turned by 0.6 rad (IoU about 0.42), exact once turned back: ANG
        [700, 100, 60, 20, np.pi / 2 + 0.6, 0.75, 0],        # the same written the other way round: turned to the label's angle as written it
                                                             # is a cross (IoU 400 / 2000), only with w and h swapped it is exact: ANG
        [912, 100, 20, 60, 0, 0.70, 0],                      # shifted by 0.6 w (IoU 480 / 1920 = 0.25), turning changes nothing: LOC
        [1112, 100, 20, 60, 0, 0.65, 0],                     # the same beside a label of class 1: BOTH
        [1300, 100, 20, 60, 0, 0.60, 0],                     # nothing there: BKG
        [1500, 100, 20, 60, 0, 0.10, 0],                     # on the last label, but below conf_thres: BELOW
    ], np.float32)
    return dets, boxes, classes, [1, 2, 3, 4, 4, 5, 6, 7, 0], [0, 1, 2, 2, 2, 3, 3]


def _deg(b):
    b = np.array(b, np.float32).reshape(-1, 5)
    b[:, 4] = b[:, 4] / np.float32(np.pi) * np.float32(180)
    return b


def _far_apart(a, b):
    """boxes_far_apart of csrc/rotated_iou.h, float32 operation by operation; a and b broadcast against each other over their leading axes."""
    f = np.float32
    rad = lambda q: f(0.5) * np.sqrt(q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3]) * f(1.001) + f(0.02)     # noqa: E731
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1]
        r = rad(a) + rad(b)
        return dx * dx + dy * dy > r * r


def _iou_matrix(a_deg, b_deg):
    m = oracle.pairwise_iou_rotated(np.ascontiguousarray(a_deg), np.ascontiguousarray(b_deg))
    m[_far_apart(a_deg[:, None, :], b_deg[None, :, :])] = 0
    return m


def _iou_diag(a_deg, b_deg):
    v = oracle.diag_iou_rotated(np.ascontiguousarray(a_deg), np.ascontiguousarray(b_deg))
    v[_far_apart(a_deg, b_deg)] = 0
    return v


def _class_index(cls, nc):
    cls = np.asarray(cls, np.float32)
    with np.errstate(invalid="ignore"):
        ok = (cls >= 0) & (cls < nc) & (cls == np.floor(cls))
    return np.where(ok, np.where(ok, cls, 0).astype(np.int64), -1)


def _first_max(m, mask):
    """Per row of m [n, nl]: the first maximum over the columns where mask holds -> (iou float32 [n], t int64 [n]); (-1, -1) without any."""
    n = m.shape[0]
    iou, t = np.full(n, -1, np.float32), np.full(n, -1, np.int64)
    if m.shape[1]:
        j = np.where(mask, m, -np.inf).argmax(1)
        has = mask.any(1)
        iou[has], t[has] = m[np.arange(n), j][has], j[has]
    return iou, t


def errors_rule(dets, boxes, classes, nc, fg=0.5, bg=0.1, conf_thres=0.0, edges=EDGES):
    """-> dict: order (the grouping), code uint8 [n], conf, pcls, ocls, s_iou, o_iou, a_iou float32 [n], s_t, o_t int64 [n] (grouped rows),
    owner int64 [nl], status int64 [nl] (grouped rows), det_hist [nc + 1, 8], cm [nc + 1, nc + 1], lab_hist [nc, 3, 4] int64."""
    f = np.float32
    dets, boxes = np.asarray(dets, f).reshape(-1, 7), np.asarray(boxes, f).reshape(-1, 5)
    lcls = np.asarray(classes, f).reshape(-1)
    order = np.argsort(lcls, kind="stable")
    boxes, lcls = boxes[order], lcls[order].astype(np.int64)
    fg, bg, conf_thres = f(fg), f(bg), f(conf_thres)
    n, nl = len(dets), len(boxes)
    d5, l5 = _deg(dets[:, :5]), _deg(boxes)
    m = _iou_matrix(d5, l5)
    pc = _class_index(dets[:, 6], nc)
    mine = (pc[:, None] == lcls[None, :]) & (pc[:, None] >= 0)
    s_iou, s_t = _first_max(m, mine)
    o_iou, o_t = _first_max(m, ~mine)
    a_iou = np.full(n, -1, f)
    has = np.nonzero(s_t >= 0)[0]
    if len(has):
        lab = l5[s_t[has]]
        turned = d5[has].copy()
        turned[:, 4] = lab[:, 4]
        a0 = _iou_diag(turned, lab)
        a1 = _iou_diag(turned[:, [0, 1, 3, 2, 4]], lab)
        a_iou[has] = np.where(a1 > a0, a1, a0)
    with np.errstate(invalid="ignore"):
        active = dets[:, 5] >= conf_thres
    cand = active & (s_iou > fg)
    owner = np.full(nl, INT_MAX, np.int64)
    np.minimum.at(owner, s_t[cand], np.nonzero(cand)[0])
    code = np.full(n, 7, np.uint8)
    for c, cond in ((6, o_iou > bg), (5, s_iou > bg), (4, (s_iou > bg) & (a_iou > fg)), (3, o_iou > fg), (2, cand)):     # the later wins
        code[cond] = c
    code[cand] = np.where(owner[s_t[cand]] == np.nonzero(cand)[0], 1, 2)
    code[~active] = 0
    status = np.full(nl, 3, np.int64)
    status[s_t[(code == 4) | (code == 5)]] = 2
    status[o_t[code == 3]] = 1
    status[owner != INT_MAX] = 0
    ocls = np.where(o_t >= 0, lcls[np.maximum(o_t, 0)] if nl else -1, -1).astype(f)
    det_hist = np.zeros((nc + 1, 8), np.int64)
    np.add.at(det_hist, (np.where(pc < 0, nc, pc), code), 1)
    cm = np.zeros((nc + 1, nc + 1), np.int64)
    ok = pc >= 0
    np.add.at(cm, (pc[ok & (code == 1)], pc[ok & (code == 1)]), 1)
    np.add.at(cm, (lcls[o_t[ok & (code == 3)]], pc[ok & (code == 3)]), 1)
    rest = ok & np.isin(code, (2, 4, 5, 6, 7))
    np.add.at(cm, (np.full(int(rest.sum()), nc), pc[rest]), 1)
    np.add.at(cm, (lcls[status != 0], np.full(int((status != 0).sum()), nc)), 1)
    area = boxes[:, 2] * boxes[:, 3]
    bucket = (area >= f(edges[0])).astype(np.int64) + (area >= f(edges[1])).astype(np.int64)
    lab_hist = np.zeros((nc, 3, 4), np.int64)
    np.add.at(lab_hist, (lcls, bucket, status), 1)
    return {"order": order, "code": code, "conf": dets[:, 5].copy(), "pcls": dets[:, 6].copy(), "ocls": ocls, "s_iou": s_iou, "o_iou": o_iou,
            "a_iou": a_iou, "s_t": s_t, "o_t": o_t, "owner": owner, "status": status, "det_hist": det_hist, "cm": cm, "lab_hist": lab_hist}
