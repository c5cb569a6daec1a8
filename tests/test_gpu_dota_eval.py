"""GPU tests of the DOTA-protocol evaluation (csrc/evaluate.hip: ryolo_dota_match, ryolo_ap_voc; lib/dota_eval.py) against the float64
restatement tests/dota_eval_ref.py.

  match      through the C ABI: status / conf / pcls / npos / cursor bit-equal and the best IoU per detection within 1e-12 on the 360 x 200 x 5
             scene "mixed" (a max_det = 700 buffer with garbage past num; a class whose 130 labels take three lane strides, an empty and a
             one-label class, duplicate labels and detections, a NaN class and a class nc, difficult labels, clockwise, counter-clockwise and
             non-convex quads, thresholds 0.5 / 0.75 / 0.9); every num around the wave size; no labels; labels as boxes; `out` untouched;
             accumulation; overflow; determinism; a captured graph; status == 1 equal to ryolo_scene_match's tp on the cases "square" and "cross";
  AP         ryolo_ap_voc within 1e-12 for both metrics on the matched scene and on 20 000 random rows x 16 classes with confidence ties;
  evaluator  DotaEvaluator / evaluate_scenes_dota with a TiledDetector on two random scenes; DotaEvaluator and SceneEvaluator interleaved on one
             stream leave each with the bytes it has alone (the two share one matching skeleton and one base class).
No row and no case is left out of a comparison: tests/test_dota_eval_cpu.py asserts that the generated cases keep their decision gaps (the
restatement and the kernel differ in cos / sin by an ulp or two), and the gaps are asserted again here with the rectangles the device
computes for the quads."""
import numpy as np
import pytest
import torch

from ryolov4_amd.synth import CFG, HYP, fill_state
from tests import dota_eval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NC, MAX_DET = R.GPU_NC, 700
NUMS = (0, 1, 63, 64, 65, 360)
TOL = 1e-12


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _rects(quads):
    """The rectangle python hands over beside every quad: the device's xyxyxyxy2xywha, as DotaEvaluator computes it."""
    from ryolov4_amd.lib import general
    q = np.asarray(quads, np.float32).reshape(-1, 8)
    return general.xyxyxyxy2xywha(torch.from_numpy(q).to(DEV)).cpu().numpy() if len(q) else np.zeros((0, 5), np.float32)


def _ref(sc, nc, iouv, gap):
    rects = sc["boxes"] if sc["quads"] is None else _rects(sc["quads"])
    m = R.match(sc["dets"], sc["quads"], rects, sc["classes"], sc["difficult"], nc, iouv)
    assert m["gap_thr"] >= gap and m["gap_top2"] >= gap, (m["gap_thr"], m["gap_top2"])
    return m


@pytest.fixture(scope="module")
def scene():
    """The case "mixed" and its restatement (computed once, never modified).  The owner of a label is the smallest row that names it, so the
    rows of a prefix of the detections are the prefix of the rows."""
    sc, nc, iouv, gap = R.gpu_case("mixed")
    return sc, iouv, _ref(sc, nc, iouv, gap)


def _padded(dets, max_det=MAX_DET, seed=0):
    """dets in a [max_det, 7] device buffer whose remaining rows are garbage: huge, negative and NaN values, classes in range."""
    rs = np.random.RandomState(seed)
    buf = (rs.standard_normal((max_det, 7)) * 1e6).astype(np.float32)
    buf[::3, 2] = np.nan
    buf[:, 6] = rs.randint(0, NC, max_det)
    buf[:len(dets)] = dets
    return torch.from_numpy(buf).to(DEV)


class Raw:
    """The accumulators of ryolo_dota_match, driven through the C ABI."""

    def __init__(self, cap, iouv, nc=NC):
        self.cap, self.nc, self.niou = cap, nc, len(iouv)
        self.status = torch.full((cap, self.niou), 7, dtype=torch.uint8, device=DEV)
        self.conf = torch.full((cap,), -5.0, device=DEV)
        self.pcls = torch.full((cap,), -5.0, device=DEV)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=DEV)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.npos = torch.zeros(nc, dtype=torch.int64, device=DEV)
        self.iouv = torch.tensor(iouv, dtype=torch.float32, device=DEV)

    def match(self, out, n, sc):
        from ryolov4_amd import hip
        from ryolov4_amd.lib.scene_eval import group_labels
        classes = np.asarray(sc["classes"], np.float32)
        order, off = group_labels(classes, self.nc)
        nl = len(order)
        quads = np.full((nl, 8), np.nan, np.float32) if sc["quads"] is None else np.asarray(sc["quads"], np.float32).reshape(nl, 8)
        rects = np.asarray(sc["boxes"], np.float32).reshape(nl, 5) if sc["quads"] is None else _rects(quads)
        rows = np.concatenate([classes[:, None], np.asarray(sc["difficult"], np.float32).reshape(nl, 1), quads, rects], 1)[order]
        lab = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
        cls_off = torch.from_numpy(off).to(DEV)
        num = torch.tensor([n], dtype=torch.int32, device=DEV)
        need = hip._Z()
        hip.call("ryolo_dota_match_workspace_bytes", out.shape[0], nl, self.niou, need)
        self.ws = torch.zeros(need.value, dtype=torch.uint8, device=DEV)
        self.max_det = out.shape[0]
        self.keep = [lab, cls_off, num, out]
        self.launch = lambda: hip.call("ryolo_dota_match", hip.ptr(out), hip.ptr(num), out.shape[0], hip.ptr(lab) if nl else None, hip.ptr(cls_off),
                                       nl, self.nc, hip.ptr(self.iouv), self.niou, hip.ptr(self.status), hip.ptr(self.conf), hip.ptr(self.pcls),
                                       self.cap, hip.ptr(self.cursor), hip.ptr(self.overflow), hip.ptr(self.npos), hip.ptr(self.ws),
                                       self.ws.numel(), hip.stream())
        self.launch()

    def rows(self):
        n = int(self.cursor.item())
        return self.status[:n].cpu().numpy(), self.conf[:n].cpu().numpy(), self.pcls[:n].cpu().numpy()

    def best_iou(self, n):
        """IoU(i, best(i)) of the last call: the first max_det doubles of the workspace (include/ryolo.h)."""
        return self.ws[:self.max_det * 8].view(torch.float64)[:n].cpu().numpy()


def _assert_rows(raw, m, dets, n, at=0, scenes=1):
    status, conf, pcls = raw.rows()
    assert int(raw.cursor.item()) == at + n and int(raw.overflow.item()) == 0
    assert status.shape == (at + n, raw.niou)
    assert np.array_equal(status[at:], m["status"][:n])
    assert np.array_equal(_bits(conf[at:]), _bits(dets[:n, 5])) and np.array_equal(_bits(pcls[at:]), _bits(dets[:n, 6]))
    assert np.array_equal(raw.npos.cpu().numpy(), m["npos"] * scenes)
    assert (raw.status[at + n:] == 7).all() and (raw.conf[at + n:] == -5).all() and (raw.pcls[at + n:] == -5).all(), "rows past the cursor are untouched"
    dev = np.abs(raw.best_iou(n) - m["best_iou"][:n])
    print(f"num {n}: max |best IoU - restatement| {dev.max() if n else 0.0:.3e}")
    assert (dev <= TOL).all()


# ---------------------------------------------------------------------------------------------- the kernel against the restatement
@pytest.mark.parametrize("n", NUMS)
def test_match_equals_the_restatement(scene, n):
    sc, iouv, m = scene
    out = _padded(sc["dets"])
    before = out.clone()
    raw = Raw(1000, iouv)
    raw.match(out, n, sc)
    _assert_rows(raw, m, sc["dets"], n)
    assert torch.equal(out.view(torch.int32), before.view(torch.int32)), "the detector's buffer is only read"
    if n == 360:
        st = m["status"]
        assert (st[:, 0] == 1).sum() >= 80 and (st == 2).sum() >= 40 and (st[:, 0] != st[:, 2]).any() and (m["best_iou"] == -1).sum() >= 2


def test_num_beyond_the_buffer_is_clamped(scene):
    sc, iouv, m = scene
    raw = Raw(1000, iouv)
    raw.match(torch.from_numpy(sc["dets"]).to(DEV), 10 ** 6, sc)       # max_det = 360
    _assert_rows(raw, m, sc["dets"], 360)
    raw.match(torch.from_numpy(sc["dets"]).to(DEV), -3, sc)
    assert int(raw.cursor.item()) == 360 and np.array_equal(raw.npos.cpu().numpy(), 2 * m["npos"]), "no row, but the scene's labels count"


def test_no_labels(scene):
    sc, iouv, _ = scene
    none = {"dets": sc["dets"], "boxes": np.zeros((0, 5), np.float32), "quads": np.zeros((0, 8), np.float32), "classes": np.zeros(0, np.float32),
            "difficult": np.zeros(0, np.uint8)}
    raw = Raw(1000, iouv)
    raw.match(_padded(sc["dets"]), 65, none)
    status, conf, pcls = raw.rows()
    assert status.shape == (65, 3) and not status.any() and not raw.npos.any()
    assert np.array_equal(_bits(conf), _bits(sc["dets"][:65, 5])) and np.array_equal(_bits(pcls), _bits(sc["dets"][:65, 6]))
    assert (raw.best_iou(65) == -1).all()


def test_labels_as_boxes():
    sc, nc, iouv, gap = R.gpu_case("boxes")
    m = _ref(sc, nc, iouv, gap)
    raw = Raw(400, iouv)
    raw.match(_padded(sc["dets"]), 360, sc)
    _assert_rows(raw, m, sc["dets"], 360)
    assert (m["status"] == 1).sum() > 100 and (m["status"] == 2).sum() > 40


def test_two_scenes_accumulate(scene):
    sc, iouv, m = scene
    raw = Raw(1000, iouv)
    raw.match(_padded(sc["dets"]), 65, sc)
    _assert_rows(raw, m, sc["dets"], 65)
    raw.match(_padded(sc["dets"], seed=3), 360, sc)
    _assert_rows(raw, m, sc["dets"], 360, at=65, scenes=2)
    assert np.array_equal(raw.rows()[0][:65], m["status"][:65])


def test_overflow_writes_nothing(scene):
    sc, iouv, m = scene
    raw = Raw(65 + 360 - 1, iouv)
    raw.match(_padded(sc["dets"]), 65, sc)
    raw.match(_padded(sc["dets"]), 360, sc)
    assert int(raw.cursor.item()) == 65 and int(raw.overflow.item()) == 1, "the cursor stays, the flag is up"
    assert np.array_equal(raw.npos.cpu().numpy(), m["npos"]), "the labels of a dropped scene are not counted"
    assert np.array_equal(raw.rows()[0], m["status"][:65])
    assert (raw.status[65:] == 7).all() and (raw.conf[65:] == -5).all() and (raw.pcls[65:] == -5).all()


def test_two_runs_are_bit_identical(scene):
    sc, iouv, _ = scene
    got = []
    for _ in range(2):
        raw = Raw(400, iouv)
        raw.match(_padded(sc["dets"]), 360, sc)
        got.append(raw.rows() + (raw.best_iou(360), raw.npos.cpu().numpy()))
    for a, b in zip(*got):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_unsupported_sizes():
    from ryolov4_amd import hip
    z = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    args = lambda nc, niou, ws: ("ryolo_dota_match", hip.ptr(z), hip.ptr(z), 4, None, hip.ptr(z), 0, nc, hip.ptr(z), niou, hip.ptr(z), hip.ptr(z),   # noqa: E731
                                 hip.ptr(z), 4, hip.ptr(z), hip.ptr(z), hip.ptr(z), hip.ptr(z), ws, hip.stream())
    with pytest.raises(RuntimeError, match="unsupported"):
        hip.call(*args(257, 3, 4096))
    with pytest.raises(RuntimeError, match="unsupported"):
        hip.call(*args(3, 17, 4096))
    with pytest.raises(RuntimeError, match="workspace"):
        hip.call(*args(3, 3, 16))


def test_captured_in_a_graph(scene):
    sc, iouv, m = scene
    out = _padded(sc["dets"])
    raw = Raw(1000, iouv)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        raw.match(out, 360, sc)                                       # eager: the rows to expect (and the warm-up)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    exp = raw.rows() + (raw.npos.cpu().numpy(),)
    assert np.array_equal(exp[0], m["status"])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        raw.launch()
    for t, v in ((raw.cursor, 0), (raw.npos, 0), (raw.status, 7), (raw.conf, -5), (raw.pcls, -5)):
        t.fill_(v)
    g.replay()
    torch.cuda.synchronize()
    got = raw.rows() + (raw.npos.cpu().numpy(),)
    for a, b in zip(exp, got):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert int(raw.cursor.item()) == 360 and int(raw.overflow.item()) == 0


@pytest.mark.parametrize("name", ["square", "cross"])
def test_true_positives_equal_the_reference_rule_kernel(name):
    """No difficult label, rectangular labels, one threshold: there the two rules coincide, and status == 1 is ryolo_scene_match's tp row for
    row.  Both cases keep gaps >= 1e-4 (asserted on the CPU and in _ref): the float pair function of that kernel and the float64 clip may
    differ in the last float32 digits.
    The two kernels do not read (x, y, w, h, theta) as the same rectangle: the pair function of the NMS is detectron2's, w along x before
    the rotation, while the polygon of a detection — what xywha2xyxyxyxy draws, write_dota_task1 submits and this protocol intersects — has
    h along x; the reference scores every box turned by 90 degrees about its own centre, which is not a rigid motion of the scene, so on
    oblong boxes the reference-rule IoU is a different number, and "cross" fed to both kernels as it is does not give the same rows.  "square":
    every box has h = w, both readings are the same rectangle and the same rows go to both kernels.  "cross": oblong boxes, and the pinned
    kernel gets w and h exchanged, which is the same rectangles in its reading."""
    from ryolov4_amd import hip
    from ryolov4_amd.lib.scene_eval import group_labels
    sc, nc, iouv, gap = R.gpu_case(name)
    m = _ref(sc, nc, iouv, gap)
    assert gap == 1e-4 and not sc["difficult"].any() and sc["quads"] is None and iouv == (0.5,)
    raw = Raw(400, iouv)
    out = _padded(sc["dets"])
    raw.match(out, 360, sc)
    _assert_rows(raw, m, sc["dets"], 360)
    order, off = group_labels(sc["classes"], nc)
    cols = [0, 1, 3, 2, 4] if name == "cross" else [0, 1, 2, 3, 4]
    assert name == "cross" or (np.array_equal(sc["boxes"][:, 2], sc["boxes"][:, 3]) and np.array_equal(sc["dets"][:, 2], sc["dets"][:, 3]))
    lab = torch.from_numpy(np.ascontiguousarray(np.concatenate([sc["classes"][order, None], sc["boxes"][order][:, cols]], 1))).to(DEV)
    cls_off, num = torch.from_numpy(off).to(DEV), torch.tensor([360], dtype=torch.int32, device=DEV)
    out = torch.cat([out[:, cols], out[:, 5:]], 1).contiguous()
    tp = torch.full((400, 1), 7, dtype=torch.uint8, device=DEV)
    conf, pcls = torch.zeros(400, device=DEV), torch.zeros(400, device=DEV)
    state = torch.zeros(2, dtype=torch.int64, device=DEV)
    need = hip._Z()
    hip.call("ryolo_scene_match_workspace_bytes", MAX_DET, len(order), need)
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    hip.call("ryolo_scene_match", hip.ptr(out), hip.ptr(num), MAX_DET, hip.ptr(lab), hip.ptr(cls_off), len(order), nc, hip.ptr(raw.iouv), 1, hip.ptr(tp),
             hip.ptr(conf), hip.ptr(pcls), 400, state.data_ptr(), state.data_ptr() + 8, hip.ptr(ws), ws.numel(), hip.stream())
    assert int(state[0].item()) == 360
    assert torch.equal(tp[:360], (raw.status[:360] == 1).to(torch.uint8)) and int(tp[:360].sum()) >= 100


# ---------------------------------------------------------------------------------------------- AP
def _ap_gpu(status, conf, pcls, npos, nc, metric):
    from ryolov4_amd import hip
    status = np.ascontiguousarray(status, np.uint8)
    n, T = status.shape
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                   # noqa: E731
    st, cf, pc, npd, grid = d(status), d(np.asarray(conf, np.float32)), d(np.asarray(pcls, np.float32)), d(np.asarray(npos, np.int64)), d(R.GRID11)
    ap = torch.full((nc, T), -7.0, dtype=torch.float64, device=DEV)
    n_pred = torch.full((nc,), -7, dtype=torch.int64, device=DEV)
    need = hip._Z()
    hip.call("ryolo_ap_voc_workspace_bytes", n, T, nc, need)
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    hip.call("ryolo_ap_voc", hip.ptr(st) if n else None, hip.ptr(cf) if n else None, hip.ptr(pc) if n else None, n, hip.ptr(npd), nc, T,
             {"voc07": 0, "voc12": 1}[metric], hip.ptr(grid), hip.ptr(ws), ws.numel(), hip.ptr(ap), hip.ptr(n_pred), hip.stream())
    return ap.cpu().numpy(), n_pred.cpu().numpy()


def _assert_ap(status, conf, pcls, npos, nc):
    out = {}
    for metric in ("voc07", "voc12"):
        exp, exp_n = R.ap_voc(status, conf, pcls, npos, nc, metric)
        got, got_n = _ap_gpu(status, conf, pcls, npos, nc, metric)
        assert np.array_equal(got_n, exp_n)
        assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(np.isnan(exp).all(1), np.asarray(npos) <= 0)
        dev = np.nanmax(np.abs(got - exp)) if not np.isnan(exp).all() else 0.0
        print(f"{metric}: max |ap - restatement| {dev:.3e}")
        assert dev <= TOL
        out[metric] = exp
    return out


def test_ap_voc_on_the_matched_scene(scene):
    sc, iouv, m = scene
    ap = _assert_ap(m["status"], sc["dets"][:, 5], sc["dets"][:, 6], m["npos"], NC)
    assert np.isnan(ap["voc07"][1]).all() and (ap["voc07"][[0, 3, 4], 0] > 0.2).all() and (ap["voc07"] != ap["voc12"])[[0, 3, 4]].any()


def test_ap_voc_on_random_rows():
    rs = np.random.RandomState(21)
    n, nc = 20000, 16
    status = rs.choice(np.array([0, 1, 2], np.uint8), size=(n, 3), p=[0.45, 0.4, 0.15])
    conf = (np.round(rs.uniform(0.05, 1.0, n) * 256) / 256).astype(np.float32)         # 244 values for 20 000 rows: ties in every class
    pcls = rs.randint(0, nc, n).astype(np.float32)
    pcls[pcls == 7] = 8                                               # class 7: positives and no detection -> 0
    pcls[::97], pcls[5::89] = np.nan, nc
    npos = rs.randint(600, 3000, nc).astype(np.int64)
    npos[3], npos[11] = 0, -2                                         # no positives -> NaN
    ap = _assert_ap(status, conf, pcls, npos, nc)
    assert (ap["voc07"][7] == 0).all() and (ap["voc12"][7] == 0).all() and np.isnan(ap["voc07"][[3, 11]]).all()
    for metric in ("voc07", "voc12"):
        assert np.array_equal(_ap_gpu(status[:0], conf[:0], pcls[:0], npos, nc, metric)[0], R.ap_voc(status[:0], conf[:0], pcls[:0], npos, nc, metric)[0],
                              equal_nan=True), "no rows at all"


# ---------------------------------------------------------------------------------------------- the evaluator
def _num(n):
    return torch.tensor([n], dtype=torch.int32, device=DEV)


def test_evaluator_host_and_device_labels(scene):
    from ryolov4_amd.lib.dota_eval import DotaEvaluator
    sc, iouv, m = scene
    dets, quads, classes, hard = sc["dets"], sc["quads"], sc["classes"], sc["difficult"]
    ev = DotaEvaluator(NC, iouv=iouv, metric="voc12", capacity=1000, device=DEV)
    assert ev.result()["npos"].tolist() == [0] * NC and np.isnan(ev.result()["map"]).all()
    ev.add(_padded(dets), _num(65), quads, classes, hard)
    ev.add(_padded(dets, seed=1), _num(0), np.zeros((0, 8), np.float32), np.zeros(0, np.float32))      # neither detections nor labels
    ev.add(_padded(dets, seed=3), _num(360), torch.from_numpy(quads).to(DEV), torch.from_numpy(classes).to(DEV), torch.from_numpy(hard).to(DEV))
    status, conf, pcls, npos = ev.stats()
    exp_status = np.concatenate([m["status"][:65], m["status"]])
    exp_conf, exp_pcls = np.concatenate([dets[:65, 5], dets[:, 5]]), np.concatenate([dets[:65, 6], dets[:, 6]])
    assert np.array_equal(status, exp_status) and np.array_equal(_bits(conf), _bits(exp_conf)) and np.array_equal(_bits(pcls), _bits(exp_pcls))
    assert np.array_equal(npos, 2 * m["npos"])
    res = ev.result()
    exp_ap, exp_n = R.ap_voc(exp_status, exp_conf, exp_pcls, 2 * m["npos"], NC, "voc12")
    assert np.nanmax(np.abs(res["ap"] - exp_ap)) <= TOL and np.array_equal(np.isnan(res["ap"]), np.isnan(exp_ap))
    assert np.array_equal(res["n_pred"], exp_n) and res["classes"].tolist() == [0, 2, 3, 4]
    assert np.abs(res["map"] - R.mean_ap(exp_ap, npos)).max() <= TOL and res["map"].shape == (3,) and res["map"][0] > res["map"][2] > 0
    ev.reset()
    status, _, _, npos = ev.stats()
    assert status.shape == (0, 3) and not npos.any()
    with pytest.raises(ValueError):
        ev.add(_padded(dets), _num(1), quads, classes, hard[:-1])
    with pytest.raises(ValueError):
        ev.add(_padded(dets), _num(1), quads[:, :6], classes)
    with pytest.raises(ValueError):
        DotaEvaluator(NC, metric="coco")


def test_evaluator_overflow_raises(scene):
    from ryolov4_amd.lib.dota_eval import DotaEvaluator
    sc, iouv, m = scene
    ev = DotaEvaluator(NC, iouv=iouv, capacity=65 + 360 - 1, device=DEV)
    ev.add(_padded(sc["dets"]), _num(65), sc["quads"], sc["classes"], sc["difficult"])
    ev.add(_padded(sc["dets"]), _num(360), sc["quads"], sc["classes"], sc["difficult"])
    with pytest.raises(RuntimeError, match="capacity"):
        ev.stats()
    with pytest.raises(RuntimeError, match="capacity"):
        ev.result()
    ev.reset()
    ev.add(_padded(sc["dets"]), _num(360), sc["quads"], sc["classes"], sc["difficult"])
    assert np.array_equal(ev.stats()[0], m["status"])


def test_interleaved_with_the_scene_evaluator_equals_each_alone(scene):
    """The two rules run through one skeleton on the host and on the device: scene, dota, scene, dota on one device and stream (n = 65, 65,
    1, 1: across a workgroup of waves and the 64 lanes, then a single row) must leave each evaluator with exactly the bytes it has after the
    same two scenes alone — no state of one rule reaches the other.  The alone runs are held to the oracles by the tests above and by
    tests/test_gpu_scene_eval.py."""
    from ryolov4_amd.lib.dota_eval import DotaEvaluator
    from ryolov4_amd.lib.scene_eval import SceneEvaluator
    from tests import scene_eval_ref as S
    sc, iouv, _ = scene
    sdets, sboxes, sclasses = S.case("mixed")

    def run(which):
        evs = {"scene": SceneEvaluator(NC, capacity=100, device=DEV), "dota": DotaEvaluator(NC, iouv=iouv, capacity=100, device=DEV)}
        for n in (65, 1):
            if "scene" in which:
                evs["scene"].add(_padded(sdets), _num(n), sboxes, sclasses)
            if "dota" in which:
                evs["dota"].add(_padded(sc["dets"]), _num(n), sc["quads"], sc["classes"], sc["difficult"])
        return {k: evs[k].stats() for k in which}

    both, alone = run(("scene", "dota")), {**run(("scene",)), **run(("dota",))}
    for k in ("scene", "dota"):
        assert len(both[k]) == len(alone[k]) == 4 and both[k][0].shape[0] == 66 and both[k][0][:, 0].sum() >= 10
        for a, b in zip(both[k], alone[k]):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


# ---------------------------------------------------------------------------------------------- end to end with a detector
def test_scenes_through_a_detector_equal_the_restatement():
    from ryolov4_amd.datasets.scene_dataset import SceneDataset
    from ryolov4_amd.lib import general
    from ryolov4_amd.lib.dota_eval import DotaEvaluator, evaluate_scenes_dota
    from ryolov4_amd.lib.tiled import TiledDetector
    from ryolov4_amd.model.yolo import Yolo
    net = Yolo(3, CFG, "kfiou", "yolov5")
    net.load_state_dict(fill_state(net.state_dict()))
    det = TiledDetector(net.to(DEV).eval(), size=256, overlap=64, batch=4, conf_thres=0.05)
    rs = np.random.RandomState(5)
    scenes = [rs.randint(0, 256, (520, 700, 3)).astype(np.uint8) for _ in range(2)]
    iouv = (0.5, 0.75)
    ev = DotaEvaluator(3, iouv=iouv, metric="voc07", device=DEV)
    polys, labels, hard, ref, rows = [], [], [], [], []
    for sc in scenes:
        d = det(sc)
        assert len(d) > 10
        sub = d[::3, :5].clone()                                      # labels: a subset of the scene's own detections, jittered
        sub[:, :2] += torch.from_numpy(rs.normal(0, 1.0, (len(sub), 2)).astype(np.float32)).to(DEV)
        sub[:, 2:4] *= torch.from_numpy(rs.uniform(0.9, 1.1, (len(sub), 2)).astype(np.float32)).to(DEV)
        p = general.xywha2xyxyxyxy(sub).reshape(-1, 8).cpu().numpy()
        c = d[::3, 6].cpu().numpy().copy()
        c[::5] = (c[::5] + 1) % 3                                     # some labels of another class
        h = (np.arange(len(c)) % 4 == 1).astype(np.uint8)             # a quarter of them difficult
        polys.append(p), labels.append(c), hard.append(h)
        ev.add_scene(det, sc, p, c, h)
        dn = d.cpu().numpy()
        m = R.match(dn, p, _rects(p), c, h, 3, iouv)                  # the restatement on the detector's own output
        assert m["gap_thr"] >= 1e-9 and m["gap_top2"] >= 1e-9, "the detector's output came too close to a decision: change the scene seed"
        ref.append(m), rows.append(dn)
    status, conf, pcls = np.concatenate([m["status"] for m in ref]), np.concatenate([r[:, 5] for r in rows]), np.concatenate([r[:, 6] for r in rows])
    npos = sum(m["npos"] for m in ref)
    got = ev.stats()
    assert (status == 1).sum() > 5 and (status == 2).sum() > 0, "true positives and ignored detections exist"
    assert np.array_equal(got[0], status) and np.array_equal(_bits(got[1]), _bits(conf)) and np.array_equal(_bits(got[2]), _bits(pcls))
    assert np.array_equal(got[3], npos)
    ds = SceneDataset(HYP, 256, False, False, device=DEV, overlap=64, keep_empty=True)
    ds.set_arrays(scenes, polys, labels, difficult=hard)
    for metric in ("voc07", "voc12"):
        exp_ap, exp_n = R.ap_voc(status, conf, pcls, npos, 3, metric)
        for res in (evaluate_scenes_dota(det, ds, metric=metric, iouv=iouv), evaluate_scenes_dota(det, ds, metric=metric, iouv=iouv, overlap=False)):
            assert np.array_equal(np.isnan(res["ap"]), np.isnan(exp_ap)) and np.nanmax(np.abs(res["ap"] - exp_ap)) <= TOL
            assert np.array_equal(res["n_pred"], exp_n) and np.array_equal(res["npos"], npos)
            assert np.abs(res["map"] - R.mean_ap(exp_ap, npos)).max() <= TOL and res["map"][0] > 0
    assert np.nanmax(np.abs(ev.result()["ap"] - R.ap_voc(status, conf, pcls, npos, 3, "voc07")[0])) <= TOL
