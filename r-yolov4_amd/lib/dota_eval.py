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
tests/dota_eval_ref.py restates all of it in float64 numpy.  Not checked anywhere: agreement with the DOTA devkit's own numbers on real
label files (the devkit is not part of this repository), and the header lines of raw DOTA label files, which the parser does not take."""
import numpy as np
import torch

from .. import hip
from . import general
from .scene_eval import MAX_CLASSES, MAX_THRESHOLDS, group_labels
from .tiled import _h2d

METRICS = {"voc07": 0, "voc12": 1}
GRID11 = np.arange(0., 1.1, 0.1)


def _check_iouv(iouv):
    v = np.asarray(iouv.detach().cpu() if isinstance(iouv, torch.Tensor) else iouv, dtype=np.float32).reshape(-1)
    if not 1 <= v.size <= MAX_THRESHOLDS:
        raise ValueError(f"DotaEvaluator: between 1 and {MAX_THRESHOLDS} IoU thresholds, got {v.size}")
    if not np.all(np.isfinite(v)) or np.any(np.diff(v) < 0) or v[0] < 0:
        raise ValueError("DotaEvaluator: iouv must be finite, non-negative and ascending")
    return v


class DotaEvaluator:
    """Accumulates (status, conf, pred_cls) rows and the positives per class over full scenes (see the module docstring).  `capacity` is
    the number of detection rows the device accumulators hold ((niou + 8) bytes per row, allocated at the first add); a scene that does
    not fit sets a device flag, writes nothing, and stats() / result() raise."""

    def __init__(self, num_classes, iouv=(0.5,), metric="voc07", capacity=1 << 20, device=None):
        if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or not 1 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError(f"DotaEvaluator: num_classes must be an integer in [1, {MAX_CLASSES}], got {num_classes!r}")
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or int(capacity) < 1:
            raise ValueError(f"DotaEvaluator: capacity must be a positive integer, got {capacity!r}")
        if metric not in METRICS:
            raise ValueError(f"DotaEvaluator: metric must be one of {sorted(METRICS)}, got {metric!r}")
        self.num_classes, self.capacity, self.metric = int(num_classes), int(capacity), metric
        self.iouv = _check_iouv(iouv)
        self.niou = int(self.iouv.size)
        self.device = None if device is None else torch.device(device)
        self._buf = None                     # (status, conf, pcls, state, npos, iouv) on the device
        self._ws = None

    # ---- device buffers
    def _buffers(self, dev):
        if self._buf is None:
            if self.device is None:
                self.device = dev
            cap, T = self.capacity, self.niou
            status = torch.empty((cap, T), dtype=torch.uint8, device=self.device)
            conf = torch.empty(cap, dtype=torch.float32, device=self.device)
            pcls = torch.empty(cap, dtype=torch.float32, device=self.device)
            state = torch.zeros(2, dtype=torch.int64, device=self.device)       # [0] the cursor, [1] (its first four bytes) the overflow flag
            npos = torch.zeros(self.num_classes, dtype=torch.int64, device=self.device)
            iouv = torch.empty(T, dtype=torch.float32, device=self.device)
            _h2d(iouv, self.iouv)
            self._buf = (status, conf, pcls, state, npos, iouv)
        if dev != self.device:
            raise RuntimeError(f"DotaEvaluator: detections on {dev}, the evaluator lives on {self.device}")
        return self._buf

    def _workspace(self, max_det, nl):
        need = hip._Z()
        hip.call("ryolo_dota_match_workspace_bytes", max_det, nl, self.niou, need)
        if self._ws is None or self._ws.numel() < need.value:
            self._ws = torch.empty(need.value, dtype=torch.uint8, device=self.device)     # the old one is released in stream order
        return self._ws

    # ---- labels of one scene -> (rows [nl, 15] = (cls, difficult, quad[8], rect[5]) grouped by class, cls_off [nc + 1]) on the device
    def _rows(self, head, geo):
        """head [nl, 2] = (cls, difficult), geo [nl, 5 | 8], both on the device and already grouped."""
        if geo.shape[1] == 8:
            quad, rect = geo, general.xyxyxyxy2xywha(geo.contiguous())
        else:
            quad, rect = torch.full((geo.shape[0], 8), float("nan"), dtype=torch.float32, device=geo.device), geo     # no quad: the box is the label
        return torch.cat([head, quad, rect], 1).contiguous()

    def _labels(self, boxes, classes, difficult):
        nc, dev = self.num_classes, self.device
        if isinstance(boxes, torch.Tensor) != isinstance(classes, torch.Tensor):
            raise ValueError("DotaEvaluator.add: labels and classes must both be host arrays or both be tensors")
        if isinstance(boxes, torch.Tensor) and boxes.is_cuda:
            # labels that already live on the device are grouped there; their classes cannot be validated without a read, so a class that
            # is not an integer in [0, nc) is a label nothing can match and that counts toward no class
            hip.require_device(classes, "DotaEvaluator.add")
            cls = classes.reshape(-1).float()
            nl = int(cls.shape[0])
            b = boxes.reshape(nl, -1).float() if nl else boxes.new_zeros((0, 5), dtype=torch.float32)
            if b.shape[1] not in (5, 8):
                raise ValueError(f"DotaEvaluator.add: labels must be boxes [nl, 5] or polygons [nl, 8], got {tuple(boxes.shape)}")
            if difficult is None:
                hard = torch.zeros(nl, dtype=torch.float32, device=dev)
            else:
                hard = (difficult if isinstance(difficult, torch.Tensor) else torch.as_tensor(np.asarray(difficult))).to(dev).reshape(-1)
                if int(hard.shape[0]) != nl:
                    raise ValueError(f"DotaEvaluator.add: {int(hard.shape[0])} difficult flags for {nl} labels")
                hard = (hard != 0).float()
            if nl == 0:
                return None, torch.zeros(nc + 1, dtype=torch.int32, device=dev), 0
            order = torch.argsort(cls, stable=True)
            scls = cls[order]
            cls_off = torch.searchsorted(scls, torch.arange(nc + 1, dtype=torch.float32, device=dev)).to(torch.int32)
            return self._rows(torch.stack([scls, hard[order]], 1), b[order]), cls_off, nl
        if isinstance(boxes, torch.Tensor):
            boxes, classes = boxes.numpy(), classes.numpy()
        if isinstance(difficult, torch.Tensor):
            difficult = difficult.detach().cpu().numpy()
        cls = np.asarray(classes, dtype=np.float32).reshape(-1)
        nl = int(cls.size)
        b = np.asarray(boxes, dtype=np.float32).reshape(nl, -1) if nl else np.zeros((0, 5), np.float32)
        if b.shape[1] not in (5, 8):
            raise ValueError(f"DotaEvaluator.add: labels must be boxes [nl, 5] or polygons [nl, 8], got {np.asarray(boxes).shape}")
        hard = np.zeros(nl, np.float32) if difficult is None else (np.asarray(difficult).reshape(-1) != 0).astype(np.float32)
        if hard.size != nl:
            raise ValueError(f"DotaEvaluator.add: {hard.size} difficult flags for {nl} labels")
        order, off = group_labels(cls, nc)
        cls_off = torch.empty(nc + 1, dtype=torch.int32, device=dev)
        _h2d(cls_off, off)
        if nl == 0:
            return None, cls_off, 0
        up = torch.empty((nl, 2 + b.shape[1]), dtype=torch.float32, device=dev)
        _h2d(up, np.concatenate([cls[order, None], hard[order, None], b[order]], 1))
        return self._rows(up[:, :2], up[:, 2:]), cls_off, nl

    # ---- public
    def add(self, out, num, polys_or_boxes, classes, difficult=None):
        """One scene.  out [max_det, 7] float32 (x, y, w, h, theta_rad, score, cls) score-descending and num [1] int32, on the device
        (rows from num on are ignored; `out` is only read).  Nothing is read back."""
        hip.require_device(out, "DotaEvaluator.add")
        hip.require_device(num, "DotaEvaluator.add")
        if out.dim() != 2 or out.shape[1] != 7 or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("DotaEvaluator.add: out must be a contiguous float32 [max_det, 7] tensor")
        if num.dtype != torch.int32 or num.numel() != 1:
            raise ValueError("DotaEvaluator.add: num must be an int32 tensor of one element")
        status, conf, pcls, state, npos, iouv = self._buffers(out.device)
        lab, cls_off, nl = self._labels(polys_or_boxes, classes, difficult)
        max_det = int(out.shape[0])
        ws = self._workspace(max_det, nl)
        hip.call("ryolo_dota_match", hip.ptr(out) if max_det else None, hip.ptr(num), max_det, hip.ptr(lab) if nl else None, hip.ptr(cls_off), nl,
                 self.num_classes, hip.ptr(iouv), self.niou, hip.ptr(status), hip.ptr(conf), hip.ptr(pcls), self.capacity, state.data_ptr(),
                 state.data_ptr() + 8, hip.ptr(npos), hip.ptr(ws), ws.numel(), hip.stream())

    def add_scene(self, det, scene, polys, classes, difficult=None):
        """det.run_async(scene) and add: the scene's detections never leave the device."""
        out, num = det.run_async(scene)
        self.add(out, num, polys, classes, difficult)

    def _count(self):
        if self._buf is None:
            return 0
        state = self._buf[3].cpu().numpy()
        if state.view(np.int32)[2]:
            raise RuntimeError(f"DotaEvaluator: more detection rows than capacity={self.capacity}; the scenes that did not fit were "
                               "dropped — use a larger capacity")
        return int(state[0])

    def stats(self):
        """(status uint8 [n, niou] (1 TP, 2 ignored, 0 FP), conf float32 [n], pred_cls float32 [n], npos int64 [nc]), scene after scene."""
        n = self._count()
        if n:
            status, conf, pcls = (t[:n].cpu().numpy() for t in self._buf[:3])
        else:
            status, conf, pcls = np.zeros((0, self.niou), np.uint8), np.zeros(0, np.float32), np.zeros(0, np.float32)
        npos = self._buf[4].cpu().numpy() if self._buf is not None else np.zeros(self.num_classes, np.int64)
        return status, conf, pcls, npos

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
            need = hip._Z()
            hip.call("ryolo_ap_voc_workspace_bytes", n, T, nc, need)
            ws = torch.empty(need.value, dtype=torch.uint8, device=self.device)
            hip.call("ryolo_ap_voc", hip.ptr(status), hip.ptr(conf), hip.ptr(pcls), n, hip.ptr(npos_d), nc, T, METRICS[self.metric], hip.ptr(grid),
                     hip.ptr(ws), ws.numel(), hip.ptr(ap_d), hip.ptr(n_pred_d), hip.stream())
            ap, npos, n_pred = ap_d.cpu().numpy(), npos_d.cpu().numpy(), n_pred_d.cpu().numpy()
        keep = npos > 0
        return {"ap": ap, "npos": npos, "n_pred": n_pred, "map": ap[keep].mean(0) if keep.any() else np.full(T, np.nan),
                "classes": np.nonzero(keep)[0], "metric": self.metric, "iouv": self.iouv.copy()}

    def reset(self):
        if self._buf is not None:
            self._buf[3].zero_()
            self._buf[4].zero_()


def evaluate_scenes_dota(det, dataset, metric="voc07", iouv=(0.5,), imread=None, overlap=True, capacity=1 << 20):
    """Every scene of a SceneDataset (`scene_files`, `scene_labels(scene)`, `scene_difficult(scene)`) through the TiledDetector `det` ->
    DotaEvaluator.result().  Scene i + 1 is decoded and uploaded on a side stream while scene i runs (TiledDetector.iter_async); per scene
    the host only enqueues.  imread: callable(path) -> uint8 HWC BGR; default: the dataset's own decoder."""
    ev = DotaEvaluator(det.nc, iouv=iouv, metric=metric, capacity=capacity, device=det.device)
    files = list(dataset.scene_files)
    if imread is None:
        pool, index = dataset.cache(), {p: i for i, p in enumerate(files)}
        imread = lambda path: pool.host_image(index[path])             # noqa: E731
    for s, (_, out, num) in enumerate(det.iter_async(files, imread=imread, overlap=overlap)):
        polys, classes = dataset.scene_labels(s)
        ev.add(out, num, polys, classes, dataset.scene_difficult(s))
    return ev.result()
