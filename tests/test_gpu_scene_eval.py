"""GPU tests of full-scene mAP matching (csrc/evaluate.hip: ryolo_scene_match; lib/scene_eval.py).

  kernel     through the C ABI, bit-equal in tp / conf / pcls / cursor to the CPU oracle's walk (oracle/ref_ops.get_batch_statistics) on the
             360 x 200 x 5 scene of tests/scene_eval_ref.py in a max_det = 700 buffer with garbage past num: a class whose 130 labels take
             three lane strides, an empty class, a one-label class, duplicate labels and detections, clutter of class nc; every num around
             the wave size; no labels; a NaN class; equal to the existing ryolo_map_match; `out` untouched; accumulation over scenes;
             overflow; determinism; captured in a graph;
  evaluator  SceneEvaluator / evaluate_scenes with a TiledDetector on two random scenes against the oracle's statistics."""
import numpy as np
import pytest
import torch

from ryolov4_amd.synth import CFG, HYP, fill_state
from tests import scene_eval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NC, MAX_DET, NIOU = 5, 700, 10
NUMS = (0, 1, 63, 64, 65, 360)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


@pytest.fixture(scope="module")
def scene():
    """The 360 x 200 x 5 case and the oracle's walk for every prefix the tests use (computed once, never modified)."""
    dets, boxes, classes = R.case("mixed")
    ref = {n: R.walk(dets[:n], boxes, classes) for n in NUMS}
    return dets, boxes, classes, ref


def _padded(dets, max_det=MAX_DET, seed=0):
    """dets in a [max_det, 7] device buffer whose remaining rows are garbage: huge, negative and NaN values, classes in range."""
    rs = np.random.RandomState(seed)
    buf = (rs.standard_normal((max_det, 7)) * 1e6).astype(np.float32)
    buf[::3, 2] = np.nan
    buf[:, 6] = rs.randint(0, NC, max_det)
    buf[:len(dets)] = dets
    return torch.from_numpy(buf).to(DEV)


class Raw:
    """The accumulators of ryolo_scene_match, driven through the C ABI."""

    def __init__(self, cap, nc=NC, iouv=R.IOUV):
        self.cap, self.nc, self.niou = cap, nc, len(iouv)
        self.tp = torch.full((cap, self.niou), 7, dtype=torch.uint8, device=DEV)
        self.conf = torch.full((cap,), -5.0, device=DEV)
        self.pcls = torch.full((cap,), -5.0, device=DEV)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.iouv = iouv.float().to(DEV)
        self.keep = []

    def match(self, out, n, boxes, classes):
        from ryolov4_amd import hip
        from ryolov4_amd.lib.scene_eval import group_labels
        order, off = group_labels(classes, self.nc)
        nl = len(order)
        lab = torch.from_numpy(np.concatenate([np.asarray(classes, np.float32)[order, None], np.asarray(boxes, np.float32).reshape(-1, 5)[order]], 1)).to(DEV)
        cls_off = torch.from_numpy(off).to(DEV)
        num = torch.tensor([n], dtype=torch.int32, device=DEV)
        need = hip._Z()
        hip.call("ryolo_scene_match_workspace_bytes", out.shape[0], nl, need)
        ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
        self.keep = [lab, cls_off, num, ws]
        self.launch = lambda: hip.call("ryolo_scene_match", hip.ptr(out), hip.ptr(num), out.shape[0], hip.ptr(lab) if nl else None,
                                       hip.ptr(cls_off), nl, self.nc, hip.ptr(self.iouv), self.niou, hip.ptr(self.tp), hip.ptr(self.conf),
                                       hip.ptr(self.pcls), self.cap, hip.ptr(self.cursor), hip.ptr(self.overflow), hip.ptr(ws), ws.numel(),
                                       hip.stream())
        self.launch()

    def rows(self):
        n = int(self.cursor.item())
        return self.tp[:n].cpu().numpy(), self.conf[:n].cpu().numpy(), self.pcls[:n].cpu().numpy()


def _assert_rows(raw, ref, n):
    tp, conf, pcls = raw.rows()
    assert int(raw.cursor.item()) == n and int(raw.overflow.item()) == 0
    assert tp.shape == (n, NIOU)
    if n:
        assert np.array_equal(tp, ref[0].astype(np.uint8))
        assert np.array_equal(_bits(conf), _bits(ref[1])) and np.array_equal(_bits(pcls), _bits(ref[2]))
    assert (raw.tp[n:] == 7).all() and (raw.conf[n:] == -5).all() and (raw.pcls[n:] == -5).all(), "rows past the cursor are untouched"


# ---------------------------------------------------------------------------------------------- the kernel against the oracle
@pytest.mark.parametrize("n", NUMS)
def test_match_equals_the_oracle_walk(scene, n):
    dets, boxes, classes, ref = scene
    out = _padded(dets)
    before = out.clone()
    raw = Raw(1000)
    raw.match(out, n, boxes, classes)
    _assert_rows(raw, ref[n], n)
    assert torch.equal(out.view(torch.int32), before.view(torch.int32)), "the detector's buffer is only read"
    if n == 360:
        assert ref[n][0][:, 0].sum() >= 100 and not ref[n][0][:, 9].all()


def test_num_beyond_the_buffer_is_clamped(scene):
    dets, boxes, classes, ref = scene
    raw = Raw(1000)
    raw.match(torch.from_numpy(dets).to(DEV), 10 ** 6, boxes, classes)       # max_det = 360
    _assert_rows(raw, ref[360], 360)
    raw.match(torch.from_numpy(dets).to(DEV), -3, boxes, classes)
    assert int(raw.cursor.item()) == 360


def test_no_labels(scene):
    dets = scene[0]
    raw = Raw(1000)
    raw.match(_padded(dets), 65, np.zeros((0, 5), np.float32), np.zeros(0, np.float32))
    tp, conf, pcls = raw.rows()
    assert tp.shape == (65, NIOU) and not tp.any()
    assert np.array_equal(_bits(conf), _bits(dets[:65, 5])) and np.array_equal(_bits(pcls), _bits(dets[:65, 6]))


def test_nan_class_and_classes_out_of_range_are_false_positives(scene):
    dets, boxes, classes, ref = scene
    hit = np.nonzero(ref[360][0][:, 0])[0]
    d = dets.copy()
    d[hit[0], 6], d[hit[1], 6], d[hit[2], 6], d[hit[3], 6] = np.nan, -1.0, 2.5, 1e9
    exp = R.walk(d, boxes, classes)
    assert not exp[0][hit[:4]].any() and exp[0][:, 0].sum() >= 100
    raw = Raw(1000)
    raw.match(_padded(d), 360, boxes, classes)
    tp, conf, pcls = raw.rows()
    assert np.array_equal(tp, exp[0].astype(np.uint8))
    assert np.array_equal(_bits(pcls), _bits(d[:, 6]))


def test_equals_the_per_image_kernel(scene):
    """The existing ryolo_map_match (one workgroup per image, the serial walk) with batch = 1 on the same inputs."""
    from ryolov4_amd import hip
    dets, boxes, classes, _ = scene
    raw = Raw(1000)
    raw.match(_padded(dets), 360, boxes, classes)
    preds = torch.from_numpy(dets).to(DEV)
    tg = R.targets_of(boxes, classes).to(DEV)
    poff = torch.tensor([0, 360], dtype=torch.int64, device=DEV)
    toff = torch.tensor([0, len(classes)], dtype=torch.int64, device=DEV)
    tp = torch.empty((360, NIOU), dtype=torch.uint8, device=DEV)
    need = hip._Z()
    hip.call("ryolo_map_match_workspace_bytes", 360, len(classes), need)
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    hip.call("ryolo_map_match", hip.ptr(preds), hip.ptr(poff), hip.ptr(tg), hip.ptr(toff), 1, 360, len(classes), hip.ptr(raw.iouv), NIOU, NC + 1,
             hip.ptr(tp), hip.ptr(ws), need.value, hip.stream())
    assert torch.equal(tp, raw.tp[:360]) and int(tp[:, 0].sum()) >= 100


def test_two_runs_are_bit_identical(scene):
    dets, boxes, classes, _ = scene
    got = []
    for _ in range(2):
        raw = Raw(400)
        raw.match(_padded(dets), 360, boxes, classes)
        got.append(raw.rows())
    for a, b in zip(*got):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_unsupported_sizes(scene):
    from ryolov4_amd import hip
    raw = Raw(8, nc=257)
    with pytest.raises(ValueError):
        raw.match(_padded(scene[0]), 1, np.zeros((0, 5), np.float32), np.zeros(0, np.float32))      # group_labels refuses first
    z = torch.zeros(1024, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        hip.call("ryolo_scene_match", hip.ptr(z), hip.ptr(z), 4, None, hip.ptr(z), 0, 257, hip.ptr(z), 10, hip.ptr(z), hip.ptr(z), hip.ptr(z), 4,
                 hip.ptr(z), hip.ptr(z), hip.ptr(z), 1024, hip.stream())
    with pytest.raises(RuntimeError, match="workspace"):
        hip.call("ryolo_scene_match", hip.ptr(z), hip.ptr(z), 4, None, hip.ptr(z), 0, 3, hip.ptr(z), 10, hip.ptr(z), hip.ptr(z), hip.ptr(z), 4,
                 hip.ptr(z), hip.ptr(z), hip.ptr(z), 16, hip.stream())


def test_captured_in_a_graph(scene):
    dets, boxes, classes, ref = scene
    out = _padded(dets)
    raw = Raw(1000)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        raw.match(out, 360, boxes, classes)                           # eager, twice: the rows to expect (and the warm-up)
        raw.launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    exp = raw.rows()
    assert exp[0].shape[0] == 720 and np.array_equal(exp[0][:360], exp[0][360:]) and np.array_equal(exp[0][:360], ref[360][0].astype(np.uint8))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        raw.launch()
    raw.cursor.zero_()
    raw.tp.fill_(7)
    raw.conf.fill_(-5)
    raw.pcls.fill_(-5)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    got = raw.rows()
    for a, b in zip(exp, got):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert int(raw.overflow.item()) == 0


# ---------------------------------------------------------------------------------------------- the evaluator
def _ev(**kw):
    from ryolov4_amd.lib.scene_eval import SceneEvaluator
    return SceneEvaluator(NC, device=DEV, **kw)


def _num(n):
    return torch.tensor([n], dtype=torch.int32, device=DEV)


def test_three_scenes_accumulate(scene):
    dets, boxes, classes, ref = scene
    ev = _ev(capacity=1000)
    none = (np.zeros((0, 5), np.float32), np.zeros(0, np.float32))
    ev.add(_padded(dets), _num(65), boxes, classes)
    ev.add(_padded(dets, seed=1), _num(0), *none)                     # neither detections nor labels: contributes nothing
    ev.add(_padded(dets, seed=2), _num(0), boxes[:7], classes[:7])    # labels without detections: their classes count
    ev.add(_padded(dets, seed=3), _num(360), torch.from_numpy(boxes).to(DEV), torch.from_numpy(classes).to(DEV))   # labels already on the device
    tp, conf, pcls, tcls = ev.stats()
    assert int(ev._buf[3][0].item()) == 425
    assert np.array_equal(tp, np.concatenate([ref[65][0], ref[360][0]]))
    assert np.array_equal(_bits(conf), _bits(np.concatenate([ref[65][1], ref[360][1]])))
    assert np.array_equal(_bits(pcls), _bits(np.concatenate([ref[65][2], ref[360][2]])))
    assert tcls.tolist() == classes.tolist() + classes[:7].tolist() + classes.tolist()
    ev.reset()
    tp, conf, pcls, tcls = ev.stats()
    assert tp.shape == (0, NIOU) and tcls.shape == (0,)


def test_polygon_labels_equal_box_labels(scene):
    from ryolov4_amd.lib import general
    dets, boxes, classes, _ = scene
    polys = general.xywha2xyxyxyxy(torch.from_numpy(boxes).to(DEV)).reshape(-1, 8)
    back = general.xyxyxyxy2xywha(polys).cpu().numpy()                # what the evaluator sees of the polygons
    exp = R.walk(dets, back, classes)
    for lab in (polys.cpu().numpy(), polys):
        ev = _ev(capacity=400)
        ev.add(_padded(dets), _num(360), lab, classes if isinstance(lab, np.ndarray) else torch.from_numpy(classes).to(DEV))
        tp = ev.stats()[0]
        assert np.array_equal(tp, exp[0]) and tp[:, 0].sum() >= 100


def test_capacity_one_row_short(scene):
    dets, boxes, classes, ref = scene
    ev = _ev(capacity=65 + 360 - 1)
    ev.add(_padded(dets), _num(65), boxes, classes)
    ev.add(_padded(dets), _num(360), boxes, classes)
    tp, conf, pcls, state, _ = ev._buf
    st = state.cpu().numpy()
    assert int(st[0]) == 65 and int(st.view(np.int32)[2]) == 1, "the cursor stays, the flag is up"
    assert np.array_equal(tp[:65].cpu().numpy(), ref[65][0].astype(np.uint8)) and np.array_equal(_bits(conf[:65].cpu().numpy()), _bits(ref[65][1]))
    with pytest.raises(RuntimeError, match="capacity"):
        ev.stats()
    ev.reset()
    ev.add(_padded(dets), _num(360), boxes, classes)
    assert np.array_equal(ev.stats()[0], ref[360][0])


# ---------------------------------------------------------------------------------------------- end to end with a detector
def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y)), (x, y)


def test_scenes_through_a_detector_equal_the_oracle():
    from oracle import ref_ops
    from ryolov4_amd.datasets.scene_dataset import SceneDataset
    from ryolov4_amd.lib import evaluate, general
    from ryolov4_amd.lib.scene_eval import SceneEvaluator, evaluate_scenes
    from ryolov4_amd.lib.tiled import TiledDetector
    from ryolov4_amd.model.yolo import Yolo
    net = Yolo(3, CFG, "kfiou", "yolov5")
    net.load_state_dict(fill_state(net.state_dict()))
    det = TiledDetector(net.to(DEV).eval(), size=256, overlap=64, batch=4, conf_thres=0.05)
    rs = np.random.RandomState(5)
    scenes = [rs.randint(0, 256, (520, 700, 3)).astype(np.uint8) for _ in range(2)]
    ev = SceneEvaluator(3, device=DEV)
    polys, labels, ref = [], [], []
    for sc in scenes:
        d = det(sc)
        assert len(d) > 10
        sub = d[::3, :5].clone()                                      # labels: a subset of the scene's own detections, jittered
        sub[:, :2] += torch.from_numpy(rs.normal(0, 1.0, (len(sub), 2)).astype(np.float32)).to(DEV)
        sub[:, 2:4] *= torch.from_numpy(rs.uniform(0.9, 1.1, (len(sub), 2)).astype(np.float32)).to(DEV)
        p = general.xywha2xyxyxyxy(sub).reshape(-1, 8)
        c = d[::3, 6].cpu().numpy().copy()
        c[::5] = (c[::5] + 1) % 3                                     # some labels of another class
        polys.append(p.cpu().numpy())
        labels.append(c)
        ev.add_scene(det, sc, polys[-1], c)
        boxes = general.xyxyxyxy2xywha(p).cpu().numpy()               # the labels as the evaluator sees them
        ref.append(ref_ops.get_batch_statistics([d.cpu().clone()], R.targets_of(boxes, c), R.IOUV, NIOU)[0])
    cat = [np.concatenate([np.asarray(s[i]) for s in ref], 0) for i in range(4)]
    got = ev.stats()
    assert cat[0][:, 0].sum() > 5, "true positives exist"
    assert np.array_equal(got[0], cat[0]) and np.array_equal(_bits(got[1]), _bits(cat[1])) and np.array_equal(_bits(got[2]), _bits(cat[2]))
    assert np.array_equal(got[3], cat[3])
    exp = evaluate.calculate_eval_stats(cat, 3)
    res = ev.result()
    _same(res, exp)
    assert res[-2] > 0
    ds = SceneDataset(HYP, 256, False, False, device=DEV, overlap=64, keep_empty=True)
    ds.set_arrays(scenes, polys, labels)
    _same(evaluate_scenes(det, ds), exp)
    _same(evaluate_scenes(det, ds, overlap=False), exp)
