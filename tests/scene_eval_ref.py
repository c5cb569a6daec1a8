"""Full-scene mAP matching: the case generator and a numpy restatement of the OWNER rule (csrc/evaluate.hip: ryolo_scene_match).

make_scene is `make_case` of tests/golden/make_golden_map.py stretched to one scene: 0-3 jittered detections per label, 15 % of them with
a wrong class, clutter with classes in [0, nc] (nc itself: a class no label has), one exact duplicate detection and one exact duplicate
label, scores rounded to 1/64 so that ties exist, stable score-descending order.  The labels come in shuffled class order, so grouping
them by class has something to keep stable.

owner_rule states the matching without a walk: the owner of label t is the smallest detection index whose best label (first maximum of
its own class) is t with IoU > iouv[0]; a detection is a true positive at threshold k iff it owns its best label and that IoU > iouv[k].
tests/test_scene_eval_cpu.py shows that it equals the walk of oracle/ref_ops.get_batch_statistics (pinned to the reference by fixture G8).
"""
import numpy as np
import torch

import oracle
from oracle import ref_ops

IOUV = torch.linspace(0.5, 0.95, 10)
INT_MAX = np.iinfo(np.int32).max

# (seed, labels per class, detections): the three cases of the CPU test; the first is the shape of the GPU tests
CASES = {"mixed": (90, (130, 0, 1, 40, 29), 360), "nolabels": (91, (0, 0, 0), 10), "scene": (92, None, 3501)}
SCENE_LABELS, SCENE_CLASSES = 1765, 16


def make_scene(seed, per_class, ndet):
    """-> (dets float32 [ndet, 7] (x, y, w, h, theta_rad, score, cls) score-descending, boxes float32 [nl, 5], classes float32 [nl])."""
    g = np.random.default_rng(seed)
    nc, nl = len(per_class), int(sum(per_class))
    side = 80.0 + 22.0 * np.sqrt(max(nl, 1))                          # the label density of make_case's 256 px images
    cls = g.permutation(np.repeat(np.arange(nc), per_class)).astype(np.float32)
    t = np.zeros((nl, 5), np.float32)
    t[:, 0:2] = g.uniform(40, side - 40, (nl, 2))
    t[:, 2] = g.uniform(8, 30, nl)
    t[:, 3] = t[:, 2] * g.uniform(1, 4, nl)
    t[:, 4] = g.uniform(-np.pi / 2, np.pi / 2, nl)
    if nl:
        big = np.nonzero(cls == np.argmax(per_class))[0]
        if len(big) > 1:
            t[big[1]] = t[big[0]]                                     # an exact duplicate label of the same class: IoU ties between labels
    rows = []
    for k in range(nl):
        for _ in range(int(g.integers(0, 4))):
            r = t[k].copy()
            r[:2] += g.normal(0, 2.0, 2)
            r[2:4] *= g.uniform(0.85, 1.15, 2)
            r[4] += g.normal(0, 0.06)
            c = cls[k] if g.random() < 0.85 else g.integers(0, nc)
            rows.append(np.concatenate([r, [g.uniform(0.05, 1.0), c]]))
    assert len(rows) <= ndet, (len(rows), ndet)
    while len(rows) < ndet:                                           # clutter, possibly of class nc
        rows.append(np.array([g.uniform(0, side), g.uniform(0, side), g.uniform(8, 30), g.uniform(20, 90), g.uniform(-1.5, 1.5),
                              g.uniform(0.05, 1.0), g.integers(0, nc + 1)]))
    p = np.array(rows, np.float32).reshape(-1, 7)
    p[:, 5] = np.round(p[:, 5] * 64) / 64                             # score ties
    if len(p) > 3:
        p[1, :5] = p[0, :5]                                           # an exact duplicate box ...
        p[1, 6] = p[0, 6]                                             # ... of the same class: IoU ties between detections
    p = p[np.argsort(-p[:, 5], kind="stable")]
    return np.ascontiguousarray(p), t, cls


def case(name):
    seed, per_class, ndet = CASES[name]
    if per_class is None:
        per_class = np.random.default_rng(seed).multinomial(SCENE_LABELS, np.full(SCENE_CLASSES, 1.0 / SCENE_CLASSES))
    return make_scene(seed, tuple(int(c) for c in per_class), ndet)


def targets_of(boxes, classes):
    """[nl, 7] = (img 0, cls, x, y, w, h, theta_rad): what get_batch_statistics takes."""
    tg = np.zeros((len(classes), 7), np.float32)
    tg[:, 1], tg[:, 2:] = classes, boxes
    return torch.from_numpy(tg)


def walk(dets, boxes, classes, iouv=IOUV):
    """The reference's statistics of ONE scene from the CPU oracle's walk: (tp bool [n, niou], conf, pcls, tcls list), or None when the
    scene has neither detections nor labels."""
    st = ref_ops.get_batch_statistics([torch.from_numpy(np.array(dets, np.float32)).reshape(-1, 7)], targets_of(boxes, classes), iouv, len(iouv))
    if not st:
        return None
    tp, conf, pcls, tcls = st[0]
    return np.asarray(tp).astype(bool), np.asarray(conf, np.float32), np.asarray(pcls, np.float32), tcls


def owner_rule(dets, boxes, classes, nc, iouv=IOUV):
    """-> (tp bool [n, niou], best_iou float32 [n], best_t int64 [n] (-1: none), owner int64 [nl] (INT_MAX: unclaimed))."""
    dets, boxes = np.asarray(dets, np.float32).reshape(-1, 7), np.asarray(boxes, np.float32).reshape(-1, 5)
    lcls, th = np.asarray(classes, np.float32).reshape(-1), np.asarray(iouv, np.float32)
    n, nl = len(dets), len(boxes)
    d5, l5 = dets[:, :5].copy(), boxes.copy()
    d5[:, 4] = d5[:, 4] / np.float32(np.pi) * np.float32(180)
    l5[:, 4] = l5[:, 4] / np.float32(np.pi) * np.float32(180)
    best_iou, best_t = np.full(n, -1, np.float32), np.full(n, -1, np.int64)
    for c in range(nc):
        pi, ti = np.nonzero(dets[:, 6] == c)[0], np.nonzero(lcls == c)[0]
        if len(pi) and len(ti):
            m = oracle.pairwise_iou_rotated(np.ascontiguousarray(d5[pi]), np.ascontiguousarray(l5[ti]))
            j = m.argmax(1)                                           # first maximum
            best_iou[pi], best_t[pi] = m[np.arange(len(pi)), j], ti[j]
    cand = (best_t >= 0) & (best_iou > th[0])
    owner = np.full(nl, INT_MAX, np.int64)
    np.minimum.at(owner, best_t[cand], np.nonzero(cand)[0])
    mine = cand.copy()
    mine[cand] = owner[best_t[cand]] == np.nonzero(cand)[0]
    return mine[:, None] & (best_iou[:, None] > th[None, :]), best_iou, best_t, owner
