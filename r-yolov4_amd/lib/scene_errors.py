"""Why a full-scene mAP is what it is: an error breakdown in the manner of TIDE (Bolya et al., 2020) next to lib/scene_eval.py, computed on
the device scene after scene.  Every detection gets one code, every label one status (include/ryolo.h: ryolo_scene_errors states the rule
operation by operation; tests/scene_errors_ref.py restates it in numpy):

  codes     BELOW  under conf_thres               TP    owns its best label of its own class (IoU > fg): SceneEvaluator's true positive
            DUP    that label has an earlier owner      CLS   a label of ANOTHER class lies under it (IoU > fg)
            ANG    IoU with its best label in (bg, fg], and turned to that label's angle it is above fg: only the angle is wrong
            LOC    IoU with its best label in (bg, fg]  BOTH  a label of another class in (bg, fg]        BKG   nothing under it
  statuses  FOUND  a detection owns it            CONFUSED  a CLS detection lies on it       MISLOCATED  an ANG / LOC detection names it
            MISSED otherwise

    an = SceneErrorAnalyzer(num_classes, fg=0.5, bg=0.1, conf_thres=0.0, size_edges=(32.0 ** 2, 96.0 ** 2), capacity=1 << 20, device=None)
    an.add(out, num, boxes, classes)          as SceneEvaluator.add: boxes [nl, 5] or polygons [nl, 8], host arrays or device tensors
    an.add_scene(det, scene, polys, classes)  det.run_async(scene) + add; nothing is read back
    an.result()                               {"det_hist" [nc + 1, 8], "confusion" [nc + 1, nc + 1], "label_hist" [nc, 3, 4]} int64, and what
                                              follows from them: "per_class" counts, "recall_by_size"; reads the cursor and the histograms
    an.rows()                                 the accumulated rows as a structured array (code, conf, pred_cls, other_cls, iou, other_iou,
                                              aligned_iou): the one larger read
    an.reset()
    analyze_scenes(det, dataset, ...)         every scene of a SceneDataset -> result()
    format_report(res, class_names)           plain text: codes per class, label statuses per class and size, the top confusions

The matcher looks at the labels of every class, so per detection it scans num_classes times the rows ryolo_scene_match scans; the shared
parts — validation, label grouping, the cursor, the overflow flag — are scene_eval._Evaluator.  Labels are rectangles, as for
SceneEvaluator: difficult flags and the annotated quadrilaterals of the DOTA protocol are not read."""
import numpy as np
import torch

from .. import hip
from . import general
from .scene_eval import _Evaluator, _scene_rows

CODES = ("BELOW", "TP", "DUP", "CLS", "ANG", "LOC", "BOTH", "BKG")
STATUSES = ("FOUND", "CONFUSED", "MISLOCATED", "MISSED")
SIZES = ("small", "medium", "large")
ROW_DTYPE = np.dtype([("code", np.uint8), ("conf", np.float32), ("pred_cls", np.float32), ("other_cls", np.float32), ("iou", np.float32),
                      ("other_iou", np.float32), ("aligned_iou", np.float32)])


class SceneErrorAnalyzer(_Evaluator):
    """Accumulates the code rows and the three histograms over full scenes (see the module docstring).  `capacity` is the number of
    detection rows the device accumulators hold (25 bytes per row, allocated at the first add); a scene that does not fit sets a device
    flag, moves nothing — no row, no histogram — and result() / rows() raise."""

    _LABELS = ("boxes", "boxes must be")

    def __init__(self, num_classes, fg=0.5, bg=0.1, conf_thres=0.0, size_edges=(32.0 ** 2, 96.0 ** 2), capacity=1 << 20, device=None):
        self._args = (fg, bg, conf_thres, size_edges)
        super().__init__(num_classes, (fg,), capacity, device)       # _check_more has judged fg by the time the base class reads it

    def _check_more(self):
        fg, bg, conf_thres, edges = self._args
        try:
            th = np.array([fg, bg, conf_thres], dtype=np.float32)
            e = np.array(edges, dtype=np.float32).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"{self._name}: fg, bg, conf_thres must be numbers and size_edges two numbers") from None
        if th.shape != (3,) or not np.all(np.isfinite(th)) or np.any(th < 0):
            raise ValueError(f"{self._name}: fg, bg and conf_thres must be finite and non-negative, got {fg!r}, {bg!r}, {conf_thres!r}")
        if not th[1] < th[0]:
            raise ValueError(f"{self._name}: bg must lie below fg (as float32), got bg={bg!r}, fg={fg!r}")
        if e.shape != (2,) or not np.all(np.isfinite(e)) or e[0] < 0 or e[1] < e[0]:
            raise ValueError(f"{self._name}: size_edges must be two finite non-negative ascending areas, got {edges!r}")
        self.fg, self.bg, self.conf_thres = (float(v) for v in th)
        self.size_edges = (float(e[0]), float(e[1]))

    def _more_buffers(self):                 # _buf = (code, conf, pcls, state, ocls, s_iou, o_iou, a_iou, det_hist, cm, lab_hist, iouv)
        nc, dev = self.num_classes, self.device
        rows = [torch.empty(self.capacity, dtype=torch.float32, device=dev) for _ in range(4)]
        return (*rows, torch.zeros((nc + 1, 8), dtype=torch.int64, device=dev), torch.zeros((nc + 1, nc + 1), dtype=torch.int64, device=dev),
                torch.zeros((nc, 3, 4), dtype=torch.int64, device=dev))

    def add(self, out, num, boxes, classes):
        """One scene.  out [max_det, 7] float32 (x, y, w, h, theta_rad, score, cls) score-descending and num [1] int32, on the device
        (rows from num on are ignored; `out` is only read).  Nothing is read back."""
        code, conf, pcls, state, ocls, s_iou, o_iou, a_iou, det_hist, cm, lab_hist, _ = self._begin(out, num)
        head, geo, cls_off, nl, _ = self._group(boxes, classes)
        lab = None
        if nl:                               # label rows [nl, 6] = (cls, x, y, w, h, theta_rad): a polygon is its rectangle
            lab = torch.cat([head, general.xyxyxyxy2xywha(geo.contiguous()) if geo.shape[1] == 8 else geo], 1).contiguous()
        max_det = int(out.shape[0])
        ws = self._workspace("ryolo_scene_errors_workspace_bytes", max_det, nl)
        hip.call("ryolo_scene_errors", hip.ptr(out) if max_det else None, hip.ptr(num), max_det, hip.ptr(lab) if nl else None, hip.ptr(cls_off), nl,
                 self.num_classes, self.fg, self.bg, self.conf_thres, *self.size_edges, hip.ptr(code), hip.ptr(conf), hip.ptr(pcls), hip.ptr(ocls),
                 hip.ptr(s_iou), hip.ptr(o_iou), hip.ptr(a_iou), hip.ptr(det_hist), hip.ptr(cm), hip.ptr(lab_hist), self.capacity,
                 state.data_ptr(), state.data_ptr() + 8, hip.ptr(ws), ws.numel(), hip.stream())

    def result(self):
        """{"det_hist" int64 [nc + 1, 8] (predicted class, row nc: an invalid class; code), "confusion" int64 [nc + 1, nc + 1] ([true][pred],
        index nc: none), "label_hist" int64 [nc, 3, 4] (class, size bucket, status), "rows": the detections seen, and derived from those:
        "per_class" {name: int64 [nc]} — labels, the four statuses, detections at or above conf_thres, the seven codes — and
        "recall_by_size" float64 [3] = FOUND / labels per size bucket (NaN for an empty bucket), "labels_by_size" int64 [3]}."""
        nc = self.num_classes
        n = self._count()
        if self._buf is None:
            det_hist, cm, lab_hist = np.zeros((nc + 1, 8), np.int64), np.zeros((nc + 1, nc + 1), np.int64), np.zeros((nc, 3, 4), np.int64)
        else:
            det_hist, cm, lab_hist = (t.cpu().numpy() for t in self._buf[8:11])
        return summarize(det_hist, cm, lab_hist, n, self)

    def rows(self):
        """The accumulated rows, scene after scene, as a structured numpy array of ROW_DTYPE."""
        n = self._count()
        out = np.zeros(n, ROW_DTYPE)
        if n:
            code, conf, pcls, _, ocls, s_iou, o_iou, a_iou = self._buf[:8]
            out["code"] = code[:n, 0].cpu().numpy()
            for name, t in zip(ROW_DTYPE.names[1:], (conf, pcls, ocls, s_iou, o_iou, a_iou)):
                out[name] = t[:n].cpu().numpy()
        return out

    def reset(self):
        super().reset()
        if self._buf is not None:
            for t in self._buf[8:11]:
                t.zero_()


def summarize(det_hist, cm, lab_hist, rows, an):
    """The result dictionary from the three histograms (numpy int64) and the analyzer's settings."""
    per_class = {"labels": lab_hist.sum((1, 2))}
    for s, name in enumerate(STATUSES):
        per_class[name.lower()] = lab_hist[:, :, s].sum(1)
    nc = lab_hist.shape[0]
    per_class["detections"] = det_hist[:nc, 1:].sum(1)
    for c, name in enumerate(CODES[1:], 1):
        per_class[name.lower()] = det_hist[:nc, c].copy()
    by_size = lab_hist.sum((0, 2))
    with np.errstate(invalid="ignore", divide="ignore"):
        recall = lab_hist[:, :, 0].sum(0) / by_size.astype(np.float64)
    return {"det_hist": det_hist, "confusion": cm, "label_hist": lab_hist, "rows": int(rows), "per_class": per_class, "recall_by_size": recall,
            "labels_by_size": by_size, "fg": an.fg, "bg": an.bg, "conf_thres": an.conf_thres, "size_edges": an.size_edges}


def analyze_scenes(det, dataset, fg=0.5, bg=0.1, conf_thres=0.0, size_edges=(32.0 ** 2, 96.0 ** 2), imread=None, overlap=True, capacity=1 << 20):
    """Every scene of a SceneDataset (`scene_files`, `scene_labels(scene)`) through the TiledDetector `det` -> SceneErrorAnalyzer.result().
    Per scene the host only enqueues (scene_eval._scene_rows, which also takes imread and overlap)."""
    an = SceneErrorAnalyzer(det.nc, fg=fg, bg=bg, conf_thres=conf_thres, size_edges=size_edges, capacity=capacity, device=det.device)
    for s, out, num in _scene_rows(det, dataset, imread, overlap):
        an.add(out, num, *dataset.scene_labels(s))
    return an.result()


def format_report(res, class_names=None, top=10):
    """A result() dictionary as plain text: detections per class and code, labels per class and status, recall per size bucket, and the
    `top` largest off-diagonal cells of the confusion matrix."""
    det_hist, cm, lab_hist = res["det_hist"], res["confusion"], res["label_hist"]
    nc = lab_hist.shape[0]
    names = [str(class_names[c]) if class_names is not None and c < len(class_names) else str(c) for c in range(nc)]
    w = max([len(s) for s in names] + [9])
    lines = [f"{res['rows']} detections, {int(lab_hist.sum())} labels; IoU above {res['fg']:g} matches, above {res['bg']:g} is near; "
             f"conf_thres {res['conf_thres']:g}", "", "detections by code"]
    lines.append(" ".join([f"{'class':<{w}}"] + [f"{c:>7}" for c in CODES]))
    for r, name in enumerate(names + ["(invalid)"]):
        if r < nc or det_hist[r].any():
            lines.append(" ".join([f"{name:<{w}}"] + [f"{int(v):>7}" for v in det_hist[r]]))
    lines.append(" ".join([f"{'all':<{w}}"] + [f"{int(v):>7}" for v in det_hist.sum(0)]))
    lines += ["", "labels by status"]
    lines.append(" ".join([f"{'class':<{w}}"] + [f"{s:>10}" for s in STATUSES] + [f"{'recall':>7}"]))
    for c, name in enumerate(names):
        st = lab_hist[c].sum(0)
        rec = f"{st[0] / st.sum():7.3f}" if st.sum() else f"{'-':>7}"
        lines.append(" ".join([f"{name:<{w}}"] + [f"{int(v):>10}" for v in st] + [rec]))
    lines += ["", f"labels by size (area edges {res['size_edges'][0]:g}, {res['size_edges'][1]:g} px^2)"]
    lines.append(" ".join([f"{'size':<{w}}"] + [f"{s:>10}" for s in STATUSES] + [f"{'recall':>7}"]))
    for b, name in enumerate(SIZES):
        st = lab_hist[:, b].sum(0)
        rec = f"{st[0] / st.sum():7.3f}" if st.sum() else f"{'-':>7}"
        lines.append(" ".join([f"{name:<{w}}"] + [f"{int(v):>10}" for v in st] + [rec]))
    off = cm[:nc, :nc].copy()
    np.fill_diagonal(off, 0)
    lines += ["", "top confusions (label class <- predicted class)"]
    flat = np.argsort(-off, axis=None, kind="stable")[:top]
    shown = 0
    for k in flat:
        t, p = divmod(int(k), nc)
        if off[t, p] > 0:
            lines.append(f"{names[t]:<{w}} <- {names[p]:<{w}} {int(off[t, p]):>7}")
            shown += 1
    if not shown:
        lines.append("none")
    return "\n".join(lines)
