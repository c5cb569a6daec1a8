"""CPU tests of the DOTA-protocol evaluation as tests/dota_eval_ref.py restates it (csrc/evaluate.hip: ryolo_dota_match, ryolo_ap_voc are held
to that restatement in tests/test_gpu_dota_eval.py), and of the "difficult" flags of the scene datasets.

  1  the closed form (owner = smallest index) equals a literal serial walk of the protocol, written here and nowhere else;
  2  hand cases of the match;
  3  the float64 clip against exact rationals on lattice quads, bound 1e-12;
  4  voc07 / voc12 by hand;
  5  SceneDataset.scene_difficult / DOTASceneDataset field 9;
  6  every generated case of the GPU tests keeps its decision gaps, so that no row has to be left out of a comparison there."""
import os
import random
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import ref_data
from tests import dota_eval_ref as R

IOUV = (0.5, 0.75, 0.9)


def _rects(quads):
    """xyxyxyxy2xywha of the oracle: the rectangle handed over beside every quad."""
    q = np.asarray(quads, np.float32).reshape(-1, 8)
    return ref_data.xyxyxyxy2xywha(torch.from_numpy(q)).numpy() if len(q) else np.zeros((0, 5), np.float32)


def _match(sc, nc, iouv=IOUV):
    rects = sc["boxes"] if sc["quads"] is None else _rects(sc["quads"])
    return R.match(sc["dets"], sc["quads"], rects, sc["classes"], sc["difficult"], nc, iouv)


# ---------------------------------------------------------------------------------------------- 1. the serial walk
def serial_walk(dets, iou, classes, difficult, nc, iouv):
    """The protocol as the devkit walks it: per threshold and class, detections by score (equal scores: row order), the label with the
    largest overlap (first maximum), a det[] flag per label."""
    n = len(dets)
    thr = np.asarray(iouv, np.float32).astype(np.float64)
    status = np.zeros((n, len(thr)), np.uint8)
    for k, th in enumerate(thr):
        for c in range(nc):
            rows = sorted((i for i in range(n) if dets[i, 6] == c), key=lambda i: (-float(dets[i, 5]), i))
            labs = [t for t in range(len(classes)) if classes[t] == c]
            det = {t: False for t in labs}
            for i in rows:
                ovmax, jmax = -np.inf, -1
                for t in labs:
                    if iou[i, t] > ovmax:
                        ovmax, jmax = iou[i, t], t
                if jmax >= 0 and ovmax > th:
                    if not difficult[jmax]:
                        if not det[jmax]:
                            status[i, k] = 1
                            det[jmax] = True
                    else:
                        status[i, k] = 2
    npos = np.array([sum(1 for t in range(len(classes)) if classes[t] == c and not difficult[t]) for c in range(nc)], np.int64)
    return status, npos


@pytest.mark.parametrize("seed,per_class,ndet", [(11, (60, 0, 1, 50, 39), 300), (12, (0, 0, 0, 0, 0), 12), (13, (20, 5, 0, 3, 2), 0)])
def test_closed_form_equals_the_serial_walk(seed, per_class, ndet):
    sc = R.make_scene(seed, per_class, ndet)
    got = _match(sc, 5)
    status, npos = serial_walk(sc["dets"], got["iou"], sc["classes"], sc["difficult"], 5, IOUV)
    assert np.array_equal(got["status"], status) and np.array_equal(got["npos"], npos)
    if ndet and sum(per_class):
        assert (status == 1).sum() > 50 and (status == 2).sum() > 20 and (status[:, 0] != status[:, 2]).any()
        assert 30 <= sc["difficult"].sum() <= 45 and npos.sum() == len(sc["classes"]) - sc["difficult"].sum()
    else:
        assert not status.any() and status.shape == (ndet, 3)


# ---------------------------------------------------------------------------------------------- 2. hand cases
SQ = [0, 0, 10, 0, 10, 10, 0, 10]                                     # the square [0, 10]^2
DET = [5, 5, 10, 10, 0.0]                                              # the detection rectangle that covers it exactly


def _hand(dets, quads, classes, difficult, rects=None, iouv=(0.5, 0.75)):
    quads = np.asarray(quads, np.float32).reshape(-1, 8)
    return R.match(np.asarray(dets, np.float32), quads, _rects(quads) if rects is None else rects, classes, difficult, 2, iouv)


def test_difficult_label_is_ignored_and_not_a_positive():
    m = _hand([DET + [0.9, 0]], [SQ], [0], [1])
    assert m["best_iou"][0] == 1.0 and m["status"].tolist() == [[2, 2]] and m["npos"].tolist() == [0, 0]
    m = _hand([DET + [0.9, 0]], [SQ], [0], [0])
    assert m["status"].tolist() == [[1, 1]] and m["npos"].tolist() == [1, 0]
    m = _hand([DET + [0.9, 1]], [SQ], [0], [0])                       # another class: no best label
    assert m["status"].tolist() == [[0, 0]] and m["best_t"][0] == -1 and m["best_iou"][0] == -1.0


def test_second_detection_on_a_claimed_label_is_a_false_positive():
    m = _hand([DET + [0.9, 0], [5, 5.5, 10, 10, 0.0, 0.8, 0], DET + [0.8, 0]], [SQ], [0], [0])
    assert m["status"].tolist() == [[1, 1], [0, 0], [0, 0]]
    # each threshold is a run of its own: the first detection reaches 0.5 only, so at 0.75 the label is still free for the second
    m = _hand([[5, 7, 10, 10, 0.0, 0.9, 0], DET + [0.8, 0]], [SQ], [0], [0])
    assert abs(m["best_iou"][0] - 80.0 / 120.0) < 1e-15 and m["status"].tolist() == [[1, 0], [0, 1]]


def test_difficult_label_at_iou_six_tenths():
    m = _hand([DET + [0.9, 0]], [[0, 0, 10, 0, 10, 6, 0, 6]], [0], [1])
    assert m["best_iou"][0] == 0.6 and m["status"].tolist() == [[2, 0]], "ignored at 0.5, a false positive at 0.75"


def test_non_convex_quad_falls_back_to_its_rectangle():
    dart = [0, 0, 10, 0, 10, 10, 8, 2]                                # vertex 3 pulled inside: not convex
    rect = np.array([[5, 5, 10, 10, 0.0]], np.float32)
    V, area, bounds, used = R.prep_labels(np.array([dart, SQ], np.float32), np.concatenate([rect, rect]))
    assert used.tolist() == [False, True] and area.tolist() == [100.0, 100.0] and np.array_equal(bounds[0], [0, 10, 0, 10])
    m = _hand([DET + [0.9, 0]], [dart], [0], [0], rects=rect)
    assert m["best_iou"][0] == 1.0 and m["status"].tolist() == [[1, 1]]
    own = _rects([dart])                                              # and with the rectangle python computes for it
    m2 = _hand([DET + [0.9, 0]], [dart], [0], [0])
    assert m2["best_iou"][0] == R.match(np.array([DET + [0.9, 0]], np.float32), None, own, [0], [0], 2, (0.5,))["best_iou"][0]
    for bad in ([0, 0, 5, 0, 10, 0, 5, 5], [0, 0, 10, 0, np.nan, 10, 0, 10], [0, 0, 10, 10, 10, 0, 0, 10]):     # collinear, NaN, a bow tie
        assert not R.prep_labels(np.array([bad], np.float32), rect)[3][0]
    V, area, bounds, _ = R.prep_labels(np.full((1, 8), np.nan, np.float32), np.full((1, 5), np.nan, np.float32))
    assert bounds[0].tolist() == [np.inf, -np.inf, np.inf, -np.inf], "a label without finite vertices overlaps nothing"


def test_clockwise_and_counter_clockwise_quads_give_the_same_iou():
    quad = np.array([1.5, 0.25, 11.0, 2.0, 9.5, 12.75, -0.5, 9.0], np.float32)
    back = quad.reshape(4, 2)[[0, 3, 2, 1]].reshape(8)                 # the same vertices from the same start, the other way round
    det = [5, 6, 9, 12, 0.3, 0.9, 0]
    a, b = _hand([det], [quad], [0], [0]), _hand([det], [back], [0], [0])
    assert 0.5 < a["best_iou"][0] < 1.0
    assert np.float64(a["best_iou"][0]).tobytes() == np.float64(b["best_iou"][0]).tobytes()
    for other in (np.roll(quad.reshape(4, 2), 1, 0), quad.reshape(4, 2)[::-1]):       # another starting vertex: the same up to rounding
        assert abs(a["best_iou"][0] - _hand([det], [other.reshape(8)], [0], [0])["best_iou"][0]) < 1e-14


# ---------------------------------------------------------------------------------------------- 3. exact rationals
def _lattice_quads(count, seed, span=40):
    """Strictly convex quadrilaterals with integer vertices, both orientations."""
    rnd = random.Random(seed)
    out = []
    while len(out) < count:
        p = [(rnd.randint(0, span), rnd.randint(0, span)) for _ in range(4)]
        cr = [(p[(e + 1) & 3][0] - p[e][0]) * (p[(e + 2) & 3][1] - p[(e + 1) & 3][1]) - (p[(e + 1) & 3][1] - p[e][1]) * (p[(e + 2) & 3][0] - p[(e + 1) & 3][0])
              for e in range(4)]
        if all(c > 0 for c in cr) or all(c < 0 for c in cr):
            out.append(p)
    return out


def test_iou_fp64_against_exact_rationals():
    S, Q = _lattice_quads(1500, 5), _lattice_quads(1500, 6)
    exact = [R.iou_exact(s, q, Fraction) for s, q in zip(S, Q)]
    one = np.array([R.iou_exact(s, q, float) for s, q in zip(S, Q)])
    V, area, _, used = R.prep_labels(np.array(Q, np.float32).reshape(-1, 8), np.zeros((len(Q), 5), np.float32))
    assert used.all()
    Sa = np.array(S, np.float64)
    inter = R.clip_area(Sa, V)
    many = inter / (0.5 * np.abs(R.fan(Sa, 4)) + area - inter)
    assert np.array_equal(one, many), "the walk over one pair and the walk over arrays of pairs are the same statements"
    dev = max(abs(Fraction(float(v)) - e) for v, e in zip(many, exact))
    print(f"max |fp64 - exact| over {len(S)} lattice pairs: {float(dev):.3e}; {sum(e > 0 for e in exact)} overlap")
    assert sum(e > 0 for e in exact) > 1000 and sum(e == 0 for e in exact) > 20
    assert dev <= Fraction(1, 10 ** 12)
    # the detection rectangle itself: theta = 0 has cos 1 and sin 0 exactly, so lattice rectangles stay on the lattice
    dets = np.array([[s[0][0] + 3, s[0][1] + 2, 4, 6, 0.0] for s in S[:300]], np.float32)
    D = R.rect_corners(dets)
    assert np.array_equal(D[0], [[S[0][0][0], S[0][0][1]], [S[0][0][0] + 6, S[0][0][1]], [S[0][0][0] + 6, S[0][0][1] + 4], [S[0][0][0], S[0][0][1] + 4]])
    M = R.iou_table(np.concatenate([dets, np.zeros((300, 2), np.float32)], 1), V[:300], area[:300], R.prep_labels(np.array(Q[:300], np.float32).reshape(-1, 8),
                    np.zeros((300, 5), np.float32))[2], np.eye(300, dtype=bool))
    for i in range(300):
        assert abs(Fraction(float(M[i, i])) - R.iou_exact([tuple(v) for v in D[i]], Q[i], Fraction)) <= Fraction(1, 10 ** 12)


# ---------------------------------------------------------------------------------------------- 4. AP by hand
def test_voc07_and_voc12_by_hand():
    # five counted rows of one class with 4 positives: TP FP TP FP TP, and an ignored row between them that must change nothing
    status = np.array([1, 0, 2, 1, 0, 1], np.uint8)[:, None]
    conf = np.array([0.9, 0.8, 0.75, 0.7, 0.6, 0.5], np.float32)
    pcls = np.zeros(6, np.float32)
    # rec = 1/4 1/4 2/4 2/4 3/4, prec = 1 1/2 2/3 2/4 3/5
    # voc07: t = 0, .1, .2 -> 1;  .3, .4, .5 -> 2/3;  .6, .7 -> 3/5;  .8, .9, 1 -> 0
    v07 = (3 * 1.0 + 3 * (2.0 / 3.0) + 2 * 0.6) / 11.0
    # voc12: envelope 1, 2/3, 2/3, 3/5, 3/5; recall steps of 1/4 at rows 0, 2, 4: (1 + 2/3 + 3/5) / 4
    v12 = (1.0 + 2.0 / 3.0 + 0.6) / 4.0
    a07, n_pred = R.ap_voc(status, conf, pcls, np.array([4, 0]), 2, "voc07")
    a12, _ = R.ap_voc(status, conf, pcls, np.array([4, 0]), 2, "voc12")
    assert abs(a07[0, 0] - v07) < 1e-15 and abs(a12[0, 0] - v12) < 1e-15 and abs(v07 - v12) > 1e-3
    assert np.isnan(a07[1, 0]) and np.isnan(a12[1, 0]) and n_pred.tolist() == [6, 0]
    assert R.mean_ap(a07, np.array([4, 0]))[0] == a07[0, 0]
    same = R.ap_voc(np.delete(status, 2, 0), np.delete(conf, 2), np.delete(pcls, 2), np.array([4, 0]), 2, "voc07")[0]
    assert same[0, 0] == a07[0, 0]
    # equal confidence: the earlier row first — FP before TP here, TP before FP after swapping the rows
    st, cf = np.array([[0], [1]], np.uint8), np.array([0.5, 0.5], np.float32)
    assert R.ap_voc(st, cf, np.zeros(2, np.float32), np.array([1]), 1, "voc12")[0][0, 0] == 0.5
    assert R.ap_voc(st[::-1], cf, np.zeros(2, np.float32), np.array([1]), 1, "voc12")[0][0, 0] == 1.0
    # positives and no detection: 0, not NaN
    assert R.ap_voc(np.zeros((0, 1), np.uint8), np.zeros(0, np.float32), np.zeros(0, np.float32), np.array([3]), 1, "voc07")[0][0, 0] == 0.0


# ---------------------------------------------------------------------------------------------- 5. the datasets' difficult flags
CLASSES = ["plane", "small vehicle", "ship"]


def test_scene_difficult_from_label_files(tmp_path):
    from ryolov4_amd.datasets.scene_dataset import DOTASceneDataset
    base = str(tmp_path)
    os.makedirs(os.path.join(base, "images"))
    os.makedirs(os.path.join(base, "annfiles"))
    images, lines = {}, {
        "000": ["10 10 30 10 30 20 10 20 plane 0", "40 40 60 40 60 50 40 50 small-vehicle 1", "5 5 9 5 9 9 5 9 ship 2"],
        # the tenth field may be absent: empty after a blank, or the file ends after the name (the parser, which is not touched, takes the
        # name up to the next blank, so a line cannot simply end after it)
        "001": ["10 10 30 10 30 20 10 20 ship ", "40 40 60 40 60 50 40 50 plane 1", "1 1 5 1 5 5 1 5 plane"],
        "002": []}
    for name, rows in lines.items():
        ip = os.path.join(base, "images", name + ".png")
        with open(ip, "wb") as fh:
            fh.write(b"\0")
        with open(os.path.join(base, "annfiles", name + ".txt"), "w") as fh:
            fh.write("\n".join(rows))
        images[ip] = np.zeros((64, 64, 3), np.uint8)
    ds = DOTASceneDataset(base, CLASSES, {}, False, 64, False, device="cpu", keep_empty=True, overlap=16, imread=lambda p: images[p],
                          imsize=lambda p: images[p].shape[:2])
    assert [ds.scene_difficult(s).tolist() for s in range(3)] == [[0, 1, 1], [0, 1, 0], []]
    assert all(ds.scene_difficult(s).dtype == np.uint8 and len(ds.scene_difficult(s)) == len(ds.scene_labels(s)[1]) for s in range(3))
    assert ds.scene_labels(0)[1].tolist() == [0, 1, 2] and ds.scene_labels(1)[1].tolist() == [2, 0, 0]


def test_scene_difficult_of_arrays():
    from ryolov4_amd.datasets.scene_dataset import SceneDataset
    rs = np.random.RandomState(0)
    scenes = [rs.randint(0, 256, (80, 90, 3)).astype(np.uint8) for _ in range(2)]
    polys = [np.array([[10, 10, 30, 10, 30, 20, 10, 20]] * 3, np.float32), np.zeros((0, 8), np.float32)]
    labels = [np.array([0, 1, 2], np.float32), np.zeros(0, np.float32)]
    ds = SceneDataset({}, 64, False, False, device="cpu", keep_empty=True, overlap=16)
    ds.set_arrays(scenes, polys, labels)                              # the call every existing caller makes
    assert ds.scene_difficult(0).tolist() == [0, 0, 0] and ds.scene_difficult(1).tolist() == [] and ds.scene_difficult(0).dtype == np.uint8
    ds.set_arrays(scenes, polys, labels, difficult=[[0, 3, 0], []])
    assert ds.scene_difficult(0).tolist() == [0, 1, 0] and ds.scene_difficult(1).tolist() == []
    with pytest.raises(ValueError):
        ds.set_arrays(scenes, polys, labels, difficult=[[0, 1], []])
    with pytest.raises(ValueError):
        ds.set_arrays(scenes, polys, labels, difficult=[[0, 1, 0]])


# ---------------------------------------------------------------------------------------------- 6. the GPU cases keep their gaps
@pytest.mark.parametrize("name", sorted(R.GPU_CASES))
def test_gpu_cases_keep_their_decision_gaps(name):
    sc, nc, iouv, gap = R.gpu_case(name)
    m = _match(sc, nc, iouv)
    print(f"{name}: gap to a threshold {m['gap_thr']:.3e}, gap between the two largest IoUs {m['gap_top2']:.3e}")
    assert m["gap_thr"] >= gap and m["gap_top2"] >= gap
    if name == "mixed":
        quads, bad = R.box_quads(sc["boxes"], R.GPU_CASES[name][0] + 2000)
        used = R.prep_labels(sc["quads"], _rects(sc["quads"]))[3]
        assert len(bad) >= 5 and not used[bad].any() and used.sum() >= 180, "non-convex quads are in the case and fall back"
        st = m["status"]
        assert (st == 1).sum() > 100 and (st == 2).sum() > 40 and (st[:, 0] != st[:, 2]).any() and sc["difficult"].sum() > 30
        assert np.isnan(sc["dets"][:, 6]).sum() == 1 and (sc["dets"][:, 6] == nc).sum() >= 1
