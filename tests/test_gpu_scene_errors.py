"""GPU tests of the full-scene error breakdown (csrc/evaluate.hip: ryolo_scene_errors; lib/scene_errors.py) against the numpy restatement
of the rule (tests/scene_errors_ref.py), bit for bit.

  kernel     through the C ABI on the planted 410 x 200 x 5 case in a max_det = 700 buffer with garbage past num: codes, ocls, the three
             IoU columns as uint32 bits, the three histograms, the cursor, rows past the cursor untouched, `dets` only read; every num
             around the wave size; conf_thres 0.0, 0.5 and above every score; the hand-made scene with its codes written out; no labels; labels without detections; NaN, negative,
             fractional and huge classes; num beyond the buffer and negative; the TP code equal to ryolo_scene_match's tp on the same
             buffers; determinism; a captured graph; the unsupported, argument and workspace statuses;
  analyzer   SceneErrorAnalyzer over three scenes (host boxes, polygons, labels on the device), a capacity one row short, and
             analyze_scenes / add_scene with a TiledDetector on two random scenes."""
import numpy as np
import pytest
import torch

from ryolov4_amd.synth import CFG, HYP, fill_state
from tests import scene_errors_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NC, MAX_DET = 5, 700
NUMS = (0, 1, 63, 64, 65, 410)
EDGES = (300.0, 1200.0)          # all three size buckets hold labels of the generated case
FLOATS = ("conf", "pcls", "ocls", "s_iou", "o_iou", "a_iou")
NONE = (np.zeros((0, 5), np.float32), np.zeros(0, np.float32))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


class Refs:
    """The restatement on a prefix of the planted case, computed once per (n, conf_thres) and never modified."""

    def __init__(self):
        self.dets, self.boxes, self.classes = E.planted_case()
        self._memo = {}

    def __call__(self, n, ct=0.0):
        if (n, ct) not in self._memo:
            self._memo[n, ct] = E.errors_rule(self.dets[:n], self.boxes, self.classes, NC, conf_thres=ct, edges=EDGES)
        return self._memo[n, ct]


@pytest.fixture(scope="module")
def scene():
    return Refs()


def _padded(dets, max_det=MAX_DET, seed=0):
    """dets in a [max_det, 7] device buffer whose remaining rows are garbage: huge, negative and NaN values, classes in range."""
    rs = np.random.RandomState(seed)
    buf = (rs.standard_normal((max_det, 7)) * 1e6).astype(np.float32)
    buf[::3, 2] = np.nan
    buf[:, 6] = rs.randint(0, NC, max_det)
    buf[:len(dets)] = dets
    return torch.from_numpy(buf).to(DEV)


class Raw:
    """The accumulators of ryolo_scene_errors, driven through the C ABI."""

    def __init__(self, cap, nc=NC, fg=0.5, bg=0.1, ct=0.0, edges=EDGES):
        self.cap, self.nc, self.scalars = cap, nc, (fg, bg, ct, *edges)
        self.code = torch.full((cap,), 9, dtype=torch.uint8, device=DEV)
        self.f = {k: torch.full((cap,), -5.0, device=DEV) for k in FLOATS}
        self.det_hist = torch.zeros((nc + 1, 8), dtype=torch.int64, device=DEV)
        self.cm = torch.zeros((nc + 1, nc + 1), dtype=torch.int64, device=DEV)
        self.lab_hist = torch.zeros((nc, 3, 4), dtype=torch.int64, device=DEV)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.keep = []

    def run(self, out, n, boxes, classes):
        from ryolov4_amd import hip
        from ryolov4_amd.lib.scene_eval import group_labels
        order, off = group_labels(classes, self.nc)
        nl, max_det = len(order), int(out.shape[0])
        lab = torch.from_numpy(np.concatenate([np.asarray(classes, np.float32)[order, None], np.asarray(boxes, np.float32).reshape(-1, 5)[order]], 1)).to(DEV)
        cls_off = torch.from_numpy(off).to(DEV)
        num = torch.tensor([n], dtype=torch.int32, device=DEV)
        need = hip._Z()
        hip.call("ryolo_scene_errors_workspace_bytes", max_det, nl, need)
        ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
        self.keep = [lab, cls_off, num, ws]
        self.launch = lambda: hip.call("ryolo_scene_errors", hip.ptr(out) if max_det else None, hip.ptr(num), max_det, hip.ptr(lab) if nl else None,
                                       hip.ptr(cls_off), nl, self.nc, *self.scalars, hip.ptr(self.code), *(hip.ptr(self.f[k]) for k in FLOATS),
                                       hip.ptr(self.det_hist), hip.ptr(self.cm), hip.ptr(self.lab_hist), self.cap, hip.ptr(self.cursor),
                                       hip.ptr(self.overflow), hip.ptr(ws), ws.numel(), hip.stream())
        self.launch()

    def clear(self):
        self.code.fill_(9)
        for t in self.f.values():
            t.fill_(-5)
        for t in (self.det_hist, self.cm, self.lab_hist, self.cursor, self.overflow):
            t.zero_()

    def everything(self):
        """All the accumulators as numpy arrays: the rows as bits, the histograms, the cursor."""
        got = {"code": self.code.cpu().numpy(), "det_hist": self.det_hist.cpu().numpy(), "cm": self.cm.cpu().numpy(),
               "lab_hist": self.lab_hist.cpu().numpy(), "cursor": int(self.cursor.item()), "overflow": int(self.overflow.item())}
        got.update({k: _bits(self.f[k].cpu().numpy()) for k in FLOATS})
        return got


def _assert_equal(raw, refs):
    """The accumulators of `raw` hold the scenes `refs` (results of errors_rule), one after the other, and nothing else."""
    got = raw.everything()
    n = sum(len(r["code"]) for r in refs)
    assert got["cursor"] == n and got["overflow"] == 0
    assert np.array_equal(got["code"][:n], np.concatenate([r["code"] for r in refs]))
    for k in FLOATS:
        assert np.array_equal(got[k][:n], _bits(np.concatenate([r[k] for r in refs]))), k
        assert (got[k][n:] == _bits(np.float32(-5.0))).all(), "rows past the cursor are untouched"
    assert (got["code"][n:] == 9).all(), "rows past the cursor are untouched"
    for k in ("det_hist", "cm", "lab_hist"):
        assert np.array_equal(got[k], sum(r[k] for r in refs)), k


# ---------------------------------------------------------------------------------------------- the kernel against the restatement
@pytest.mark.parametrize("ct", [0.0, 0.5])
@pytest.mark.parametrize("n", NUMS)
def test_errors_equal_the_restatement(scene, n, ct):
    out = _padded(scene.dets)
    before = out.clone()
    raw = Raw(1000, ct=ct)
    raw.run(out, n, scene.boxes, scene.classes)
    ref = scene(n, ct)
    _assert_equal(raw, [ref])
    assert torch.equal(out.view(torch.int32), before.view(torch.int32)), "the detector's buffer is only read"
    if n == 410:
        assert (np.bincount(ref["code"], minlength=8)[1:] >= 3).all() and (np.bincount(ref["status"], minlength=4) >= 3).all()
        assert (ref["lab_hist"].sum((0, 2)) >= 10).all()


def test_conf_thres_above_every_score(scene):
    raw = Raw(1000, ct=2.0)
    raw.run(_padded(scene.dets), 410, scene.boxes, scene.classes)
    ref = scene(410, 2.0)
    assert (ref["code"] == 0).all() and ref["lab_hist"][:, :, 3].sum() == 200 and ref["cm"][:NC, NC].sum() == 200
    _assert_equal(raw, [ref])


def test_hand_made_scene():
    """One detection and one label per category, the codes written out by hand (scene_errors_ref.hand_scene): among them the ANG row that
    only the swapped box of a_iou rescues."""
    dets, boxes, classes, codes, statuses = E.hand_scene()
    raw = Raw(16, nc=2, ct=0.3)
    raw.run(torch.from_numpy(dets).to(DEV), len(dets), boxes, classes)
    ref = E.errors_rule(dets, boxes, classes, 2, conf_thres=0.3, edges=EDGES)
    _assert_equal(raw, [ref])
    assert raw.code[:len(dets)].tolist() == codes
    assert raw.lab_hist.sum((0, 1)).tolist() == np.bincount(statuses, minlength=4).tolist()


def test_no_labels(scene):
    raw = Raw(1000)
    raw.run(_padded(scene.dets), 65, *NONE)
    ref = E.errors_rule(scene.dets[:65], *NONE, NC, edges=EDGES)
    assert (ref["code"] == 7).all() and (ref["ocls"] == -1).all() and (ref["s_iou"] == -1).all()
    _assert_equal(raw, [ref])


def test_labels_without_detections(scene):
    """num == 0 in a full buffer, then max_det == 0: only the label side moves, and every label is MISSED."""
    raw = Raw(1000)
    raw.run(_padded(scene.dets), 0, scene.boxes, scene.classes)
    raw.run(torch.zeros((0, 7), device=DEV), 5, scene.boxes[:7], scene.classes[:7])
    refs = [scene(0), E.errors_rule(scene.dets[:0], scene.boxes[:7], scene.classes[:7], NC, edges=EDGES)]
    assert refs[0]["lab_hist"][:, :, 3].sum() == 200 and refs[1]["lab_hist"].sum() == refs[1]["cm"][:NC, NC].sum() == 7
    _assert_equal(raw, refs)


def test_nan_negative_fractional_and_huge_classes(scene):
    base = scene(410)
    hit, cls_err = np.nonzero(base["code"] == 1)[0], np.nonzero(base["code"] == 3)[0]
    d = scene.dets.copy()
    d[hit[0], 6], d[hit[1], 6], d[hit[2], 6], d[hit[3], 6], d[cls_err[0], 6] = np.nan, -1.0, 2.5, 1e9, np.nan
    ref = E.errors_rule(d, scene.boxes, scene.classes, NC, edges=EDGES)
    bad = np.r_[hit[:4], cls_err[0]]
    assert (ref["code"][bad] == 3).all() and (ref["s_t"][bad] == -1).all(), "with no class of their own they lie on a label of another"
    assert ref["det_hist"][NC, 3] == base["det_hist"][NC, 3] + 5 and ref["cm"][:, :NC].sum() == base["cm"][:, :NC].sum() - 5, "counted in the invalid row, not in cm"
    raw = Raw(1000)
    raw.run(_padded(d), 410, scene.boxes, scene.classes)
    _assert_equal(raw, [ref])


def test_num_beyond_the_buffer_and_negative(scene):
    raw = Raw(1000)
    out = torch.from_numpy(scene.dets).to(DEV)                          # max_det = 410
    raw.run(out, 10 ** 6, scene.boxes, scene.classes)
    _assert_equal(raw, [scene(410)])
    raw.run(out, -3, scene.boxes, scene.classes)
    _assert_equal(raw, [scene(410), scene(0)])


def test_tp_code_equals_scene_match(scene):
    """On the same buffers, code == TP is ryolo_scene_match's tp at iouv[0] = fg."""
    from ryolov4_amd import hip
    out = _padded(scene.dets)
    raw = Raw(1000)
    raw.run(out, 410, scene.boxes, scene.classes)
    lab, cls_off, num, _ = raw.keep
    iouv = torch.tensor([0.5], device=DEV)
    tp = torch.zeros((MAX_DET, 1), dtype=torch.uint8, device=DEV)
    conf, pcls = torch.zeros(MAX_DET, device=DEV), torch.zeros(MAX_DET, device=DEV)
    state = torch.zeros(2, dtype=torch.int64, device=DEV)
    need = hip._Z()
    hip.call("ryolo_scene_match_workspace_bytes", MAX_DET, len(lab), need)
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    hip.call("ryolo_scene_match", hip.ptr(out), hip.ptr(num), MAX_DET, hip.ptr(lab), hip.ptr(cls_off), len(lab), NC, hip.ptr(iouv), 1, hip.ptr(tp),
             hip.ptr(conf), hip.ptr(pcls), MAX_DET, state.data_ptr(), state.data_ptr() + 8, hip.ptr(ws), ws.numel(), hip.stream())
    assert int(state[0].item()) == 410
    assert torch.equal(tp[:410, 0], (raw.code[:410] == 1).to(torch.uint8)) and int(tp[:410].sum()) >= 100


def test_two_runs_are_bit_identical(scene):
    got = []
    for _ in range(2):
        raw = Raw(500, ct=0.5)
        raw.run(_padded(scene.dets), 410, scene.boxes, scene.classes)
        got.append(raw.everything())
    for k, v in got[0].items():
        assert np.array_equal(v, got[1][k]), k


def test_statuses(scene):
    from ryolov4_amd import hip
    z = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = hip.ptr(z)

    def call(nc=3, fg=0.5, bg=0.1, ct=0.0, e0=1.0, e1=2.0, ws=4096, max_det=4, cap=4):
        hip.call("ryolo_scene_errors", p, p, max_det, None, p, 0, nc, fg, bg, ct, e0, e1, p, p, p, p, p, p, p, p, p, p, cap, p, p, p, ws, hip.stream())

    call()                                                            # the arguments the others vary: num = 0, no labels, nothing moves
    torch.cuda.synchronize()
    assert not z.any()
    with pytest.raises(RuntimeError, match="unsupported"):
        call(nc=257)
    for kw in (dict(bg=0.5), dict(fg=0.1, bg=0.3), dict(bg=-0.1), dict(fg=float("nan")), dict(ct=float("nan")), dict(e0=3.0), dict(e1=float("nan")),
               dict(nc=0), dict(max_det=-1), dict(cap=-1)):
        with pytest.raises(RuntimeError, match="invalid argument"):
            call(**kw)
    with pytest.raises(RuntimeError, match="workspace"):
        call(ws=16)
    need = hip._Z()
    with pytest.raises(RuntimeError, match="invalid argument"):
        hip.call("ryolo_scene_errors_workspace_bytes", -1, 0, need)


def test_captured_in_a_graph(scene):
    out = _padded(scene.dets)
    raw = Raw(1000, ct=0.5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        raw.run(out, 410, scene.boxes, scene.classes)                 # eager, twice: what to expect (and the warm-up)
        raw.launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _assert_equal(raw, [scene(410, 0.5)] * 2)
    exp = raw.everything()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        raw.launch()
    raw.clear()
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    got = raw.everything()
    for k, v in exp.items():
        assert np.array_equal(v, got[k]), k


# ---------------------------------------------------------------------------------------------- the analyzer
def _an(**kw):
    from ryolov4_amd.lib.scene_errors import SceneErrorAnalyzer
    return SceneErrorAnalyzer(NC, size_edges=EDGES, device=DEV, **kw)


def _num(n):
    return torch.tensor([n], dtype=torch.int32, device=DEV)


def _assert_analyzer(an, refs):
    rows, res = an.rows(), an.result()
    n = sum(len(r["code"]) for r in refs)
    assert rows.shape == (n,) and res["rows"] == n
    assert np.array_equal(rows["code"], np.concatenate([r["code"] for r in refs]))
    for name, k in zip(rows.dtype.names[1:], FLOATS):
        assert np.array_equal(_bits(rows[name]), _bits(np.concatenate([r[k] for r in refs]))), name
    for name, k in (("det_hist", "det_hist"), ("confusion", "cm"), ("label_hist", "lab_hist")):
        assert res[name].dtype == np.int64 and np.array_equal(res[name], sum(r[k] for r in refs)), name
    return res


def test_three_scenes_accumulate(scene):
    from ryolov4_amd.lib import general
    dets, boxes, classes = scene.dets, scene.boxes, scene.classes
    polys = general.xywha2xyxyxyxy(torch.from_numpy(boxes).to(DEV)).reshape(-1, 8)
    back = general.xyxyxyxy2xywha(polys).cpu().numpy()                # what the analyzer sees of the polygons
    an = _an(capacity=1000, conf_thres=0.5)
    an.add(_padded(dets), _num(65), boxes, classes)
    an.add(_padded(dets, seed=1), _num(0), *NONE)                     # neither detections nor labels: contributes nothing
    an.add(_padded(dets, seed=2), _num(64), polys.cpu().numpy(), classes)
    an.add(_padded(dets, seed=3), _num(410), torch.from_numpy(boxes).to(DEV), torch.from_numpy(classes).to(DEV))   # labels already on the device
    refs = [scene(65, 0.5), E.errors_rule(dets[:64], back, classes, NC, conf_thres=0.5, edges=EDGES), scene(410, 0.5)]
    res = _assert_analyzer(an, refs)
    assert res["per_class"]["labels"].tolist() == [390, 0, 3, 120, 87] and res["labels_by_size"].sum() == 600
    assert np.array_equal(res["per_class"]["tp"], res["per_class"]["found"]) and res["per_class"]["tp"].sum() > 100
    an.reset()
    res = an.result()
    assert res["rows"] == 0 and not res["det_hist"].any() and not res["confusion"].any() and not res["label_hist"].any()
    assert an.rows().shape == (0,)


def test_capacity_one_row_short(scene):
    dets, boxes, classes = scene.dets, scene.boxes, scene.classes
    an = _an(capacity=65 + 410 - 1)
    an.add(_padded(dets), _num(65), boxes, classes)
    an.add(_padded(dets), _num(410), boxes, classes)
    buf = an._buf
    st = buf[3].cpu().numpy()
    assert int(st[0]) == 65 and int(st.view(np.int32)[2]) == 1, "the cursor stays, the flag is up"
    ref = scene(65)
    assert np.array_equal(buf[0][:65, 0].cpu().numpy(), ref["code"]) and np.array_equal(_bits(buf[5][:65].cpu().numpy()), _bits(ref["s_iou"]))
    for t, k in zip(buf[8:11], ("det_hist", "cm", "lab_hist")):
        assert np.array_equal(t.cpu().numpy(), ref[k]), f"{k} stays where it was"
    with pytest.raises(RuntimeError, match="capacity"):
        an.result()
    with pytest.raises(RuntimeError, match="capacity"):
        an.rows()
    an.reset()
    an.add(_padded(dets), _num(410), boxes, classes)
    _assert_analyzer(an, [scene(410)])


# ---------------------------------------------------------------------------------------------- end to end with a detector
def test_scenes_through_a_detector_equal_the_restatement():
    from ryolov4_amd.datasets.scene_dataset import SceneDataset
    from ryolov4_amd.lib import general
    from ryolov4_amd.lib.scene_errors import SceneErrorAnalyzer, analyze_scenes, format_report
    from ryolov4_amd.lib.tiled import TiledDetector
    from ryolov4_amd.model.yolo import Yolo
    net = Yolo(3, CFG, "kfiou", "yolov5")
    net.load_state_dict(fill_state(net.state_dict()))
    det = TiledDetector(net.to(DEV).eval(), size=256, overlap=64, batch=4, conf_thres=0.05)
    rs = np.random.RandomState(5)
    scenes = [rs.randint(0, 256, (520, 700, 3)).astype(np.uint8) for _ in range(2)]
    kw = dict(fg=0.5, bg=0.1, conf_thres=0.1, size_edges=(100.0, 400.0))
    an = SceneErrorAnalyzer(3, device=DEV, **kw)
    polys, labels, refs = [], [], []
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
        an.add_scene(det, sc, polys[-1], c)
        boxes = general.xyxyxyxy2xywha(p).cpu().numpy()               # the labels as the analyzer sees them
        refs.append(E.errors_rule(d.cpu().numpy(), boxes, c, 3, edges=kw["size_edges"], **{k: kw[k] for k in ("fg", "bg", "conf_thres")}))
    res = _assert_analyzer(an, refs)
    assert res["det_hist"][:, 1].sum() > 5 and res["det_hist"][:, 3].sum() > 0, "true positives and class confusions exist"
    ds = SceneDataset(HYP, 256, False, False, device=DEV, overlap=64, keep_empty=True)
    ds.set_arrays(scenes, polys, labels)
    for overlap in (True, False):
        got = analyze_scenes(det, ds, overlap=overlap, **kw)
        for k in ("det_hist", "confusion", "label_hist"):
            assert np.array_equal(got[k], res[k]), k
        assert got["rows"] == res["rows"]
    assert "detections by code" in format_report(res, ["a", "b", "c"])
