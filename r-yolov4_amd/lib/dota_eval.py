"""mAP on full scenes in the DOTA / VOC protocol — the rule the dataset's numbers are published under — next to lib/scene_eval.py, which
scores by the reference's rule.  Three things differ (include/ryolo.h: ryolo_dota_match, ryolo_ap_voc state them in full):

  difficult   a label flagged "difficult" counts toward no class's positives, and a detection whose best label is difficult is ignored:
              neither a true nor a false positive;
  geometry    the detection's rectangle is intersected with the ANNOTATED quadrilateral in float64 (its xyxyxyxy2xywha rectangle only
              when the quad is not strictly convex or not finite);
  AP          the 11-point VOC07 mean or the all-point VOC12 area, every IoU threshold a run of its own.

    ev = DotaEvaluator(num_classes, iouv=(0.5,), metric="voc07", capacity=1 << 20, device=None)
    ev.add(out, num, polys_or_boxes, classes, difficult=None)    out / num as TiledDetector.run_async returns them; polygons [nl, 8] or
                                                                 boxes [nl, 5] (x, y, w, h, theta_rad), classes [nl], difficult [nl]
                                                                 (nonzero: difficult); host arrays or device tensors
    ev.add_scene(det, scene, polys, classes, difficult=None)     det.run_async(scene) + add; nothing is read back
    status, conf, pcls, npos = ev.stats()                        the accumulated rows (numpy); status 1 TP, 2 ignored, 0 FP
    ev.result()                                                  {"ap" [nc, niou], "npos" [nc], "n_pred" [nc], "map" [niou], "classes"}
    ev.reset()
    evaluate_scenes_dota(det, dataset, metric=..., iouv=...)     every scene of a SceneDataset (scene_labels, scene_difficult) -> result()

Per scene the host uploads the labels grouped by class and enqueues; rows, cursor, overflow flag and the positives per class live on the
device.  result() reads the cursor once, computes the AP on the device (the rows are not brought over) and reads nc x niou numbers.
Everything the two evaluators share is scene_eval._Evaluator; this module holds the difficult column, the label rows, npos and the VOC AP.
tests/dota_eval_ref.py restates all of it in float64 numpy.  Not checked anywhere: agreement with the DOTA devkit's own numbers on real
label files (the devkit is not part of this repository), and the header lines of raw DOTA label files, which the parser does not take."""
import numpy as np
import torch

from .. import hip
from . import general
from .scene_eval import _Evaluator, _h2d, _scene_rows

METRICS = {"voc07": 0, "voc12": 1}
GRID11 = np.arange(0., 1.1, 0.1)


class DotaEvaluator(_Evaluator):
    """Accumulates (status, conf, pred_cls) rows and the positives per class over full scenes (see the module docstring).  `capacity` is
    the number of detection rows the device accumulators hold ((niou + 8) bytes per row, allocated at the first add); a scene that does
    not fit sets a device flag, writes nothing, and stats() / result() raise."""

    def __init__(self, num_classes, iouv=(0.5,), metric="voc07", capacity=1 << 20, device=None):
        self.metric = metric
        super().__init__(num_classes, iouv, capacity, device, nonnegative=True)

    def _check_more(self):
        if self.metric not in METRICS:
            raise ValueError(f"DotaEvaluator: metric must be one of {sorted(METRICS)}, got {self.metric!r}")

    def _more_buffers(self):                 # _buf = (status, conf, pcls, state, npos, iouv)
        return (torch.zeros(self.num_classes, dtype=torch.int64, device=self.device),)

    def _rows(self, head, geo):
        """head [nl, 2] = (cls, difficult), geo [nl, 5 | 8], both on the device and already grouped -> rows [nl, 15] = (cls, difficult,
        quad[8], rect[5])."""
        if geo.shape[1] == 8:
            quad, rect = geo, general.xyxyxyxy2xywha(geo.contiguous())
        else:
            quad, rect = torch.full((geo.shape[0], 8), float("nan"), dtype=torch.float32, device=geo.device), geo     # no quad: the box is the label
        return torch.cat([head, quad, rect], 1).contiguous()

    def add(self, out, num, polys_or_boxes, classes, difficult=None):
        """One scene.  out [max_det, 7] float32 (x, y, w, h, theta_rad, score, cls) score-descending and num [1] int32, on the device
        (rows from num on are ignored; `out` is only read).  Nothing is read back."""
        status, conf, pcls, state, npos, iouv = self._begin(out, num)
        head, geo, cls_off, nl, _ = self._group(polys_or_boxes, classes, difficult=difficult)
        lab = self._rows(head, geo) if nl else None
        max_det = int(out.shape[0])
        ws = self._workspace("ryolo_dota_match_workspace_bytes", max_det, nl, self.niou)
        hip.call("ryolo_dota_match", hip.ptr(out) if max_det else None, hip.ptr(num), max_det, hip.ptr(lab) if nl else None, hip.ptr(cls_off), nl,
                 self.num_classes, hip.ptr(iouv), self.niou, hip.ptr(status), hip.ptr(conf), hip.ptr(pcls), self.capacity, state.data_ptr(),
                 state.data_ptr() + 8, hip.ptr(npos), hip.ptr(ws), ws.numel(), hip.stream())

    def add_scene(self, det, scene, polys, classes, difficult=None):
        """det.run_async(scene) and add: the scene's detections never leave the device."""
        out, num = det.run_async(scene)
        self.add(out, num, polys, classes, difficult)

    def stats(self):
        """(status uint8 [n, niou] (1 TP, 2 ignored, 0 FP), conf float32 [n], pred_cls float32 [n], npos int64 [nc]), scene after scene."""
        npos = self._buf[4].cpu().numpy() if self._buf is not None else np.zeros(self.num_classes, np.int64)
        return (*self._read_rows(), npos)

    def result(self):
        """{"ap": float64 [nc, niou] (NaN: a class without positives), "npos": int64 [nc], "n_pred": int64 [nc], "map": float64 [niou] (the
        mean over the classes with positives; NaN when there is none), "classes": their indices, "metric", "iouv"} over everything added."""
        nc, T = self.num_classes, self.niou
        n = self._count()
        if self._buf is None:
            ap, npos, n_pred = np.full((nc, T), np.nan), np.zeros(nc, np.int64), np.zeros(nc, np.int64)
        else:
            status, conf, pcls, _, npos_d, _ = self._buf
            ap_d = torch.empty((nc, T), dtype=torch.float64, device=self.device)
            n_pred_d = torch.empty(nc, dtype=torch.int64, device=self.device)
            grid = torch.empty(11, dtype=torch.float64, device=self.device)
            _h2d(grid, GRID11)
            ws = hip.workspace("ryolo_ap_voc_workspace_bytes", n, T, nc, device=self.device)
            hip.call("ryolo_ap_voc", hip.ptr(status), hip.ptr(conf), hip.ptr(pcls), n, hip.ptr(npos_d), nc, T, METRICS[self.metric], hip.ptr(grid),
                     hip.ptr(ws), ws.numel(), hip.ptr(ap_d), hip.ptr(n_pred_d), hip.stream())
            ap, npos, n_pred = ap_d.cpu().numpy(), npos_d.cpu().numpy(), n_pred_d.cpu().numpy()
        keep = npos > 0
        return {"ap": ap, "npos": npos, "n_pred": n_pred, "map": ap[keep].mean(0) if keep.any() else np.full(T, np.nan),
                "classes": np.nonzero(keep)[0], "metric": self.metric, "iouv": self.iouv.copy()}

    def reset(self):
        super().reset()
        if self._buf is not None:
            self._buf[4].zero_()


def evaluate_scenes_dota(det, dataset, metric="voc07", iouv=(0.5,), imread=None, overlap=True, capacity=1 << 20):
    """Every scene of a SceneDataset (`scene_files`, `scene_labels(scene)`, `scene_difficult(scene)`) through the TiledDetector `det` ->
    DotaEvaluator.result().  Per scene the host only enqueues (scene_eval._scene_rows, which also takes imread and overlap)."""
    ev = DotaEvaluator(det.nc, iouv=iouv, metric=metric, capacity=capacity, device=det.device)
    for s, out, num in _scene_rows(det, dataset, imread, overlap):
        ev.add(out, num, *dataset.scene_labels(s), dataset.scene_difficult(s))
    return ev.result()
