"""Full-scene mAP, CPU side (r-yolov4_amd/lib/scene_eval.py; no device is touched).

  rule     the owner rule the kernel rests on (tests/scene_eval_ref.owner_rule: no walk, one minimum per label) gives exactly the
           true-positive matrix of the walk of oracle/ref_ops.get_batch_statistics on the three generated scenes;
  labels   group_labels: offsets, stability, empty classes, no labels, the ValueErrors;
  errors   SceneEvaluator's argument checks that need no device."""
import numpy as np
import pytest
import torch

from tests import scene_eval_ref as R


# ---------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("name,n,nl,nc", [("mixed", 360, 200, 5), ("nolabels", 10, 0, 3), ("scene", 3501, 1765, 16)])
def test_owner_rule_equals_the_reference_walk(name, n, nl, nc):
    dets, boxes, classes = R.case(name)
    assert dets.shape == (n, 7) and boxes.shape == (nl, 5) and classes.shape == (nl,)
    assert np.all(np.diff(dets[:, 5]) <= 0), "score-descending"
    ref_tp, conf, pcls, tcls = R.walk(dets, boxes, classes)
    tp, best_iou, best_t, owner = R.owner_rule(dets, boxes, classes, nc)
    assert tp.shape == ref_tp.shape == (n, 10)
    assert np.array_equal(tp, ref_tp)
    assert np.array_equal(conf, dets[:, 5]) and np.array_equal(pcls, dets[:, 6]) and tcls == classes.tolist()
    cand = best_iou > np.float32(0.5)
    losers = int(cand.sum() - ref_tp[:, 0].sum())
    print(f"{name}: TP at 0.5 {int(ref_tp[:, 0].sum())}, TP at 0.95 {int(ref_tp[:, 9].sum())}, candidates {int(cand.sum())}, lose their label {losers}")
    if name == "mixed":                                               # judged on the REFERENCE's output: the case is not vacuous
        assert np.bincount(classes.astype(int), minlength=5).tolist() == [130, 0, 1, 40, 29]
        assert ref_tp[:, 0].sum() >= 100
        assert losers >= 50
        assert not np.array_equal(ref_tp[:, 9], ref_tp[:, 0])
        assert (dets[:, 6] == 5).any(), "clutter of class nc"
        assert len(np.unique(dets[:, 5])) < n, "score ties"
    if name == "nolabels":
        assert not ref_tp.any() and tcls == []
    if name == "scene":
        assert ref_tp[:, 0].sum() >= 1000 and losers >= 500


def test_owner_rule_on_a_hand_made_scene():
    """Two detections share a best label: the earlier one owns it, the later one stays a false positive although a second label overlaps
    it above the threshold."""
    boxes = np.array([[50, 50, 10, 20, 0.0], [53, 50, 10, 20, 0.0]], np.float32)
    classes = np.array([0, 0], np.float32)
    dets = np.array([[50, 50, 10, 20, 0.0, 0.9, 0], [50.5, 50, 10, 20, 0.0, 0.8, 0], [53, 50, 10, 20, 0.0, 0.7, 0]], np.float32)
    tp, best_iou, best_t, owner = R.owner_rule(dets, boxes, classes, 1)
    assert best_t.tolist() == [0, 0, 1] and owner.tolist() == [0, 2]
    assert tp[:, 0].tolist() == [True, False, True]
    assert np.array_equal(tp, R.walk(dets, boxes, classes)[0])


# ---------------------------------------------------------------------------------------------- group_labels
def test_group_labels_offsets_and_stability():
    from ryolov4_amd.lib.scene_eval import group_labels
    cls = np.array([3, 0, 3, 2, 0, 3, 0], np.float32)
    order, off = group_labels(cls, 5)
    assert order.tolist() == [1, 4, 6, 3, 0, 2, 5], "ascending class, the caller's order inside a class"
    assert off.dtype == np.int32 and off.tolist() == [0, 3, 3, 4, 7, 7], "classes 1 and 4 are empty"
    _, _, classes = R.case("mixed")
    order, off = group_labels(classes, 5)
    assert np.diff(off).tolist() == [130, 0, 1, 40, 29]
    assert np.array_equal(order, np.argsort(classes, kind="stable"))
    for c in range(5):
        assert np.all(classes[order[off[c]:off[c + 1]]] == c)


def test_group_labels_without_labels():
    from ryolov4_amd.lib.scene_eval import group_labels
    order, off = group_labels(np.zeros(0, np.float32), 3)
    assert order.shape == (0,) and off.tolist() == [0, 0, 0, 0]
    order, off = group_labels([], 256)
    assert off.shape == (257,) and not off.any()


@pytest.mark.parametrize("cls,nc", [([0, 3], 3), ([-1], 3), ([0.5], 3), ([float("nan")], 3), ([0], 257), ([0], 0)])
def test_group_labels_rejects(cls, nc):
    from ryolov4_amd.lib.scene_eval import group_labels
    with pytest.raises(ValueError):
        group_labels(np.asarray(cls, np.float32), nc)


# ---------------------------------------------------------------------------------------------- argument errors
@pytest.mark.parametrize("kw", [dict(num_classes=0), dict(num_classes=257), dict(num_classes=2.5), dict(num_classes=3, capacity=0),
                                dict(num_classes=3, iouv=[]), dict(num_classes=3, iouv=np.linspace(0.1, 0.9, 17)),
                                dict(num_classes=3, iouv=[0.75, 0.5]), dict(num_classes=3, iouv=[0.5, float("nan")])])
def test_evaluator_rejects_bad_arguments(kw):
    from ryolov4_amd.lib.scene_eval import SceneEvaluator
    with pytest.raises(ValueError):
        SceneEvaluator(**kw)


def test_evaluator_needs_no_device_until_the_first_scene_and_refuses_host_detections():
    from ryolov4_amd.lib.scene_eval import SceneEvaluator
    ev = SceneEvaluator(5)
    assert ev.niou == 10 and ev.capacity == 1 << 20 and np.array_equal(ev.iouv, R.IOUV.numpy())
    with pytest.raises(RuntimeError):                                 # the product path has no CPU fallback
        ev.add(torch.zeros((4, 7)), torch.zeros(1, dtype=torch.int32), np.zeros((0, 5), np.float32), np.zeros(0, np.float32))
    tp, conf, pcls, tcls = ev.stats()                                 # nothing added: empty statistics, still no device
    assert tp.shape == (0, 10) and tp.dtype == bool and conf.shape == pcls.shape == tcls.shape == (0,)
    res = ev.result(host=True)
    assert res[-1] == 0.0 and len(res) == 11
