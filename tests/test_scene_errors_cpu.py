"""Full-scene error breakdown, CPU side (r-yolov4_amd/lib/scene_errors.py; tests/scene_errors_ref.py; no device is touched).

  rule     the restatement the kernel is held to (scene_errors_ref.errors_rule): its TP code is the true positive of
           scene_eval_ref.owner_rule — and with that of the reference's walk — on every generated case; every detection has one code, FOUND
           labels and TP rows are the same number, the confusion matrix and the two histograms agree; a hand-made scene with one detection
           and one label per category, the expected codes written out; the planted case is not vacuous;
  python   SceneErrorAnalyzer's argument checks that need no device, the derived counts and the text report."""
import numpy as np
import pytest

from tests import scene_errors_ref as E
from tests import scene_eval_ref as R

NC = 5
# label area edges under which the generated labels (w in [8, 30], h = w .. 4 w) fill all three size buckets
EDGES = (300.0, 1200.0)


@pytest.fixture(scope="module")
def planted():
    dets, boxes, classes = E.planted_case()
    return dets, boxes, classes, {ct: E.errors_rule(dets, boxes, classes, NC, conf_thres=ct, edges=EDGES) for ct in (0.0, 0.5)}


# ---------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("name,nc", [("mixed", 5), ("nolabels", 3), ("scene", 16)])
def test_tp_code_equals_the_owner_rule(name, nc):
    dets, boxes, classes = R.case(name)
    r = E.errors_rule(dets, boxes, classes, nc, fg=0.5, conf_thres=0.0)
    tp, best_iou, best_t, _ = R.owner_rule(dets, boxes, classes, nc)
    assert np.array_equal(r["code"] == 1, tp[:, 0])
    assert np.array_equal(r["s_iou"].view(np.uint32), best_iou.view(np.uint32)), "same(i) is best(i) of ryolo_scene_match"
    assert np.array_equal(np.where(r["s_t"] >= 0, r["order"][np.maximum(r["s_t"], 0)] if len(boxes) else -1, -1), best_t)
    assert not (r["code"] == 0).any()
    if name == "mixed":
        assert tp[:, 0].sum() >= 100
    if name == "nolabels":
        assert (r["code"] == 7).all() and (r["a_iou"] == -1).all() and r["cm"][nc].sum() == (dets[:, 6] < nc).sum()


@pytest.mark.parametrize("ct", [0.0, 0.5])
def test_counts_agree(planted, ct):
    dets, boxes, classes, ref = planted
    r = ref[ct]
    code, status, det_hist, cm, lab_hist = r["code"], r["status"], r["det_hist"], r["cm"], r["lab_hist"]
    assert code.shape == (410,) and code.max() <= 7 and det_hist.sum() == 410, "one code per detection"
    assert np.array_equal(det_hist.sum(0), np.bincount(code, minlength=8))
    assert (status == 0).sum() == (code == 1).sum() == np.trace(cm), "every FOUND label has exactly one TP row"
    assert np.array_equal(lab_hist.sum((1, 2)), np.bincount(classes.astype(int), minlength=NC))
    assert np.array_equal(lab_hist.sum((0, 1)), np.bincount(status, minlength=4))
    assert (lab_hist.sum((0, 2)) >= 10).all(), "all three size buckets hold labels"
    assert np.array_equal(cm[:, :NC].sum(0), det_hist[:NC, 1:].sum(1)), "a column of cm: the active detections of that class"
    assert np.array_equal(cm[:NC, NC], lab_hist[:, :, 1:].sum((1, 2))), "the last column: the labels that are not FOUND"
    assert np.array_equal(cm[NC, :NC], det_hist[:NC][:, [2, 4, 5, 6, 7]].sum(1)) and cm[NC, NC] == 0
    assert cm[:NC, :NC].sum() - np.trace(cm) == det_hist[:NC, 3].sum(), "off the diagonal: the CLS rows"
    assert det_hist[NC, 1:].sum() == (dets[dets[:, 5] >= ct, 6] == NC).sum() > 0, "clutter of class nc is counted in the invalid row"
    assert ((code == 0) == (dets[:, 5] < np.float32(ct))).all()


def test_the_planted_case_is_not_vacuous(planted):
    dets, boxes, classes, ref = planted
    assert dets.shape == (410, 7) and np.all(np.diff(dets[:, 5]) <= 0)
    for ct in (0.0, 0.5):
        codes, statuses = np.bincount(ref[ct]["code"], minlength=8), np.bincount(ref[ct]["status"], minlength=4)
        print(f"conf_thres {ct}: codes {codes.tolist()}, statuses {statuses.tolist()}")
        assert (codes[1:] >= 3).all() and (statuses >= 3).all()
    r = ref[0.0]
    ang = r["code"] == 4
    assert (r["a_iou"][ang] > 0.5).all() and (r["s_iou"][ang] <= 0.5).all()
    assert ((r["code"] == 5) & (r["a_iou"] > r["s_iou"])).any(), "LOC rows that turning helps, but not above fg"


def test_hand_made_scene():
    dets, boxes, classes, codes, statuses = E.hand_scene()
    r = E.errors_rule(dets, boxes, classes, 2, fg=0.5, bg=0.1, conf_thres=0.3)
    assert r["code"].tolist() == codes
    assert r["status"][np.argsort(r["order"])].tolist() == statuses
    assert 0.3 < r["s_iou"][3] < 0.5 and r["a_iou"][3] > 0.99
    assert abs(r["s_iou"][4] - r["s_iou"][3]) < 1e-3 and r["a_iou"][4] > 0.99, "without the swapped box a_iou would be 0.2"
    assert r["ocls"].tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 1] and r["o_t"][2] == 5, "grouped rows: class 0 has five labels, then class 1"
    assert r["cm"].tolist() == [[1, 0, 4], [1, 0, 2], [6, 0, 0]]
    assert r["det_hist"].tolist() == [[1, 1, 1, 1, 2, 1, 1, 1], [0] * 8, [0] * 8]


# ---------------------------------------------------------------------------------------------- the Python side
@pytest.mark.parametrize("kw", [dict(num_classes=0), dict(num_classes=257), dict(num_classes=3, capacity=0), dict(num_classes=3, bg=0.5),
                                dict(num_classes=3, fg=0.3, bg=0.4), dict(num_classes=3, bg=-0.1), dict(num_classes=3, fg=float("nan")),
                                dict(num_classes=3, fg=float("inf")), dict(num_classes=3, conf_thres=float("nan")),
                                dict(num_classes=3, conf_thres=-1.0), dict(num_classes=3, size_edges=(100.0, 10.0)),
                                dict(num_classes=3, size_edges=(1.0, 2.0, 3.0)), dict(num_classes=3, size_edges=(1.0, float("inf"))),
                                dict(num_classes=3, fg="high")])
def test_analyzer_rejects_bad_arguments(kw):
    from ryolov4_amd.lib.scene_errors import SceneErrorAnalyzer
    with pytest.raises(ValueError):
        SceneErrorAnalyzer(**kw)


def test_analyzer_needs_no_device_until_the_first_scene():
    import torch
    from ryolov4_amd.lib import scene_errors as S
    assert S.CODES == E.CODES and S.STATUSES == E.STATUSES
    an = S.SceneErrorAnalyzer(5)
    assert (an.fg, an.bg, an.conf_thres, an.size_edges, an.niou) == (0.5, float(np.float32(0.1)), 0.0, (1024.0, 9216.0), 1)
    with pytest.raises(RuntimeError):                                 # the product path has no CPU fallback
        an.add(torch.zeros((4, 7)), torch.zeros(1, dtype=torch.int32), np.zeros((0, 5), np.float32), np.zeros(0, np.float32))
    res = an.result()
    assert res["rows"] == 0 and not res["det_hist"].any() and res["confusion"].shape == (6, 6) and res["label_hist"].shape == (5, 3, 4)
    assert np.isnan(res["recall_by_size"]).all()
    assert an.rows().shape == (0,) and an.rows().dtype.names == ("code", "conf", "pred_cls", "other_cls", "iou", "other_iou", "aligned_iou")
    assert "none" in S.format_report(res)


def test_derived_counts_and_report(planted):
    from ryolov4_amd.lib import scene_errors as S
    r = planted[3][0.5]
    an = S.SceneErrorAnalyzer(NC, conf_thres=0.5, size_edges=EDGES)
    res = S.summarize(r["det_hist"], r["cm"], r["lab_hist"], 410, an)
    pc = res["per_class"]
    assert pc["labels"].tolist() == [130, 0, 1, 40, 29]
    assert np.array_equal(pc["found"], pc["tp"]) and np.array_equal(pc["found"] + pc["confused"] + pc["mislocated"] + pc["missed"], pc["labels"])
    assert np.array_equal(pc["detections"], sum(pc[k.lower()] for k in S.CODES[1:]))
    found = np.array([((r["status"] == 0) & (b == np.arange(3)[:, None])).sum(1) for b in [_buckets(planted[1][r["order"]])]])[0]
    assert np.allclose(res["recall_by_size"], found / res["labels_by_size"]) and res["labels_by_size"].sum() == 200
    text = S.format_report(res, ["plane", "ship", "tank", "court", "bridge"])
    print(text)
    assert "plane" in text and "(invalid)" in text and "MISLOCATED" in text and "<-" in text
    assert f"{int(r['det_hist'][0, 1]):>7}" in text


def _buckets(boxes):
    area = boxes[:, 2] * boxes[:, 3]
    return (area >= np.float32(EDGES[0])).astype(int) + (area >= np.float32(EDGES[1])).astype(int)
