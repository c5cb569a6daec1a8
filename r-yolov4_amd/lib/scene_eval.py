"""mAP on full scenes: the detections of a merged scene (lib/tiled.py: up to max_det = 5 000 rows) are matched to the scene's labels (a few
thousand) on the device, scene after scene, and the statistics of the reference's test.py stay on the device until they are asked for.

    ev = SceneEvaluator(num_classes, iouv=torch.linspace(0.5, 0.95, 10), capacity=1 << 20, device=None)
    ev.add(out, num, boxes, classes)          out / num as TiledDetector.run_async returns them; boxes [nl, 5] (x, y, w, h, theta_rad) or
                                              polygons [nl, 8], classes [nl]; host arrays or device tensors
    ev.add_scene(det, scene, polys, classes)  det.run_async(scene) + add; nothing is read back
    tp, conf, pcls, tcls = ev.stats()         the reference's concatenated statistics (numpy); THE device -> host read
    ev.result(host=False)                     evaluate.calculate_eval_stats(ev.stats(), num_classes, host): the reference's 11-tuple
    ev.reset()
    evaluate_scenes(det, dataset)             every scene of a SceneDataset -> ev.result()
    group_labels(classes, nc)                 (stable ascending class order, [nc + 1] int32 offsets) — numpy

The rule is the reference's (test.py:130-145), the one `evaluate.get_batch_statistics` applies per window: a detection is a candidate iff
its best-IoU label of its own class (first maximum) has IoU > iouv[0]; in score order a candidate is a true positive iff its best label is
not yet claimed, and one whose label is taken stays a false positive.  There is no fallback to a second-best label, so the owner of a
label is simply the first candidate that names it — which csrc/evaluate.hip (ryolo_scene_match; include/ryolo.h states the rule and its
ties) computes with one wave per detection and one atomicMin per candidate instead of a serial walk on one compute unit.  Per scene the
host uploads the labels grouped by class (one small pinned copy) and enqueues; counts, cursor and overflow flag live on the device.
DOTA's "difficult" flags are not read (DOTADataset ignores them too): lib/dota_eval.py scores by the dataset's own protocol.  Both
evaluators are _Evaluator below — validation, device accumulators, label grouping, the cursor — plus their own label rows and statistics,
as both matchers in csrc/evaluate.hip are one skeleton with a rule each.
"""
import numpy as np
import torch

from .. import hip
from . import evaluate, general
from .tiled import _h2d

MAX_CLASSES = evaluate.MAP_MAX_CLASSES
MAX_THRESHOLDS = 16           # csrc/evaluate.hip (AP_MAX_T)


def group_labels(classes, nc):
    """classes [nl] (any real dtype), nc -> (order int64 [nl]: the stable ascending class order, cls_off int32 [nc + 1]: class c owns
    positions [cls_off[c], cls_off[c + 1]) of classes[order]).  ValueError for a class that is not an integer in [0, nc) and for
    nc > 256."""
    nc = int(nc)
    if not 1 <= nc <= MAX_CLASSES:
        raise ValueError(f"group_labels: the number of classes must lie in [1, {MAX_CLASSES}], got {nc}")
    cls = np.asarray(classes, dtype=np.float64).reshape(-1)
    bad = ~((cls >= 0) & (cls < nc) & (cls == np.floor(cls)))         # NaN fails the comparisons
    if bad.any():
        raise ValueError(f"group_labels: class {cls[bad][0]} is not an integer in [0, {nc})")
    ids = cls.astype(np.int64)
    order = np.argsort(ids, kind="stable")
    cls_off = np.zeros(nc + 1, dtype=np.int32)
    cls_off[1:] = np.cumsum(np.bincount(ids, minlength=nc))
    return order, cls_off


class _Evaluator:
    """What the full-scene evaluators share: argument validation, the device accumulators `_buf` = (rows [capacity, niou] uint8, conf,
    pcls, state, *_more_buffers(), iouv) allocated at the first add, the grow-only workspace, the labels of a scene grouped by class on
    the host or on the device, and the cursor with its overflow flag.  Messages name the class the caller used."""

    _LABELS = ("labels", "labels must be boxes")      # how add's messages call the label argument

    def __init__(self, num_classes, iouv, capacity, device, nonnegative=False):
        self._name = type(self).__name__
        if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or not 1 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError(f"{self._name}: num_classes must be an integer in [1, {MAX_CLASSES}], got {num_classes!r}")
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or int(capacity) < 1:
            raise ValueError(f"{self._name}: capacity must be a positive integer, got {capacity!r}")
        self.num_classes, self.capacity = int(num_classes), int(capacity)
        self._check_more()
        v = np.asarray(iouv.detach().cpu() if isinstance(iouv, torch.Tensor) else iouv, dtype=np.float32).reshape(-1)
        if not 1 <= v.size <= MAX_THRESHOLDS:
            raise ValueError(f"{self._name}: between 1 and {MAX_THRESHOLDS} IoU thresholds, got {v.size}")
        if not np.all(np.isfinite(v)) or np.any(np.diff(v) < 0) or (nonnegative and v[0] < 0):
            raise ValueError(f"{self._name}: iouv must be finite{', non-negative' if nonnegative else ''} and ascending")
        self.iouv, self.niou = v, int(v.size)
        self.device = None if device is None else torch.device(device)
        self._buf = None
        self._ws = None

    def _check_more(self):
        """A subclass's own constructor checks, in their place between capacity and iouv."""

    # ---- device buffers
    def _more_buffers(self):
        return ()

    def _buffers(self, dev):
        if self._buf is None:
            if self.device is None:
                self.device = dev
            cap, T = self.capacity, self.niou
            rows = torch.empty((cap, T), dtype=torch.uint8, device=self.device)
            conf = torch.empty(cap, dtype=torch.float32, device=self.device)
            pcls = torch.empty(cap, dtype=torch.float32, device=self.device)
            state = torch.zeros(2, dtype=torch.int64, device=self.device)       # [0] the cursor, [1] (its first four bytes) the overflow flag
            iouv = torch.empty(T, dtype=torch.float32, device=self.device)
            _h2d(iouv, self.iouv)
            self._buf = (rows, conf, pcls, state, *self._more_buffers(), iouv)
        if dev != self.device:
            raise RuntimeError(f"{self._name}: detections on {dev}, the evaluator lives on {self.device}")
        return self._buf

    def _workspace(self, entry, *sizes):
        need = hip.workspace_bytes(entry, *sizes)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)     # the old one is released in stream order
        return self._ws

    def _begin(self, out, num):
        """The checks of add's `out` / `num` -> the device buffers."""
        hip.require_device(out, f"{self._name}.add")
        hip.require_device(num, f"{self._name}.add")
        if out.dim() != 2 or out.shape[1] != 7 or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"{self._name}.add: out must be a contiguous float32 [max_det, 7] tensor")
        if num.dtype != torch.int32 or num.numel() != 1:
            raise ValueError(f"{self._name}.add: num must be an int32 tensor of one element")
        return self._buffers(out.device)

    # ---- labels of one scene, grouped by class
    def _flag(self, name, values, nl, dev):
        """One per-label flag column (None: all clear) -> float32 [nl], 1 where nonzero; a numpy array when dev is None."""
        if values is None:
            return np.zeros(nl, np.float32) if dev is None else torch.zeros(nl, dtype=torch.float32, device=dev)
        if dev is None:
            col = np.asarray(values.detach().cpu() if isinstance(values, torch.Tensor) else values).reshape(-1)
        else:
            col = (values if isinstance(values, torch.Tensor) else torch.as_tensor(np.asarray(values))).to(dev).reshape(-1)
        if len(col) != nl:
            raise ValueError(f"{self._name}.add: {len(col)} {name} flags for {nl} labels")
        return (col != 0).astype(np.float32) if dev is None else (col != 0).float()

    def _group(self, boxes, classes, **flags):
        """-> (head [nl, 1 + len(flags)] = (cls, *flags), geo [nl, 5 | 8], cls_off int32 [nc + 1], nl, classes in the caller's order); head and
        geo on the device in class order (None without labels), cls_off on the device."""
        nc, dev, where = self.num_classes, self.device, f"{self._name}.add"
        if isinstance(boxes, torch.Tensor) != isinstance(classes, torch.Tensor):
            raise ValueError(f"{where}: {self._LABELS[0]} and classes must both be host arrays or both be tensors")
        if isinstance(boxes, torch.Tensor) and boxes.is_cuda:
            # labels that already live on the device are grouped there; their classes cannot be validated without a read, so a class that
            # is not an integer in [0, nc) is a label nothing can match and that counts toward no class
            hip.require_device(classes, where)
            cls = classes.reshape(-1).float()
            nl = int(cls.shape[0])
            b = boxes.reshape(nl, -1).float() if nl else boxes.new_zeros((0, 5), dtype=torch.float32)
            if b.shape[1] not in (5, 8):
                raise ValueError(f"{where}: {self._LABELS[1]} [nl, 5] or polygons [nl, 8], got {tuple(boxes.shape)}")
            cols = [self._flag(k, v, nl, dev) for k, v in flags.items()]
            if nl == 0:
                return None, None, torch.zeros(nc + 1, dtype=torch.int32, device=dev), 0, None
            order = torch.argsort(cls, stable=True)
            scls = cls[order]
            cls_off = torch.searchsorted(scls, torch.arange(nc + 1, dtype=torch.float32, device=dev)).to(torch.int32)
            return torch.stack([scls] + [c[order] for c in cols], 1), b[order], cls_off, nl, cls
        if isinstance(boxes, torch.Tensor):
            boxes, classes = boxes.numpy(), classes.numpy()
        cls = np.asarray(classes, dtype=np.float32).reshape(-1)
        nl = int(cls.size)
        b = np.asarray(boxes, dtype=np.float32).reshape(nl, -1) if nl else np.zeros((0, 5), np.float32)
        if b.shape[1] not in (5, 8):
            raise ValueError(f"{where}: {self._LABELS[1]} [nl, 5] or polygons [nl, 8], got {np.asarray(boxes).shape}")
        cols = [self._flag(k, v, nl, None) for k, v in flags.items()]
        order, off = group_labels(cls, nc)
        cls_off = torch.empty(nc + 1, dtype=torch.int32, device=dev)
        _h2d(cls_off, off)
        if nl == 0:
            return None, None, cls_off, 0, cls
        h = 1 + len(cols)
        up = torch.empty((nl, h + b.shape[1]), dtype=torch.float32, device=dev)
        _h2d(up, np.concatenate([cls[order, None]] + [c[order, None] for c in cols] + [b[order]], 1))
        return up[:, :h], up[:, h:], cls_off, nl, cls

    # ---- public
    def add_scene(self, det, scene, polys, classes):
        """det.run_async(scene) and add: the scene's detections never leave the device."""
        out, num = det.run_async(scene)
        self.add(out, num, polys, classes)

    def _count(self):
        """The rows accumulated so far: reads the cursor and the overflow flag once."""
        if self._buf is None:
            return 0
        state = self._buf[3].cpu().numpy()
        if state.view(np.int32)[2]:
            raise RuntimeError(f"{self._name}: more detection rows than capacity={self.capacity}; the scenes that did not fit were "
                               "dropped — use a larger capacity")
        return int(state[0])

    def _read_rows(self):
        """(rows uint8 [n, niou], conf float32 [n], pred_cls float32 [n]) as numpy: the device -> host read."""
        n = self._count()
        if n:
            return tuple(t[:n].cpu().numpy() for t in self._buf[:3])
        return np.zeros((0, self.niou), np.uint8), np.zeros(0, np.float32), np.zeros(0, np.float32)

    def reset(self):
        if self._buf is not None:
            self._buf[3].zero_()


class SceneEvaluator(_Evaluator):
    """Accumulates the reference's (tp, conf, pred_cls, target_cls) over full scenes (see the module docstring).  `capacity` is the number
    of detection rows the device accumulators hold ((niou + 8) bytes per row, allocated at the first add); a scene that does not fit
    sets a device flag, writes nothing, and stats() raises.  Target classes stay on the host, in the caller's label order."""

    _LABELS = ("boxes", "boxes must be")

    def __init__(self, num_classes, iouv=None, capacity=1 << 20, device=None):
        super().__init__(num_classes, torch.linspace(0.5, 0.95, 10) if iouv is None else iouv, capacity, device)
        self._tcls = []                      # per scene: numpy array, or a device tensor that stats() brings over

    def add(self, out, num, boxes, classes):
        """One scene.  out [max_det, 7] float32 (x, y, w, h, theta_rad, score, cls) score-descending and num [1] int32, on the device
        (rows from num on are ignored; `out` is only read).  Nothing is read back."""
        tp, conf, pcls, state, iouv = self._begin(out, num)
        head, geo, cls_off, nl, tcls = self._group(boxes, classes)
        lab = None
        if nl:                               # label rows [nl, 6] = (cls, x, y, w, h, theta_rad): a polygon is its rectangle
            self._tcls.append(tcls)
            lab = torch.cat([head, general.xyxyxyxy2xywha(geo.contiguous()) if geo.shape[1] == 8 else geo], 1).contiguous()
        max_det = int(out.shape[0])
        if max_det == 0:
            return
        ws = self._workspace("ryolo_scene_match_workspace_bytes", max_det, nl)
        hip.call("ryolo_scene_match", hip.ptr(out), hip.ptr(num), max_det, hip.ptr(lab) if nl else None, hip.ptr(cls_off), nl, self.num_classes,
                 hip.ptr(iouv), self.niou, hip.ptr(tp), hip.ptr(conf), hip.ptr(pcls), self.capacity, state.data_ptr(), state.data_ptr() + 8,
                 hip.ptr(ws), ws.numel(), hip.stream())

    def stats(self):
        """(tp bool [n, niou], conf float32 [n], pred_cls float32 [n], target_cls float64 [nt]) — np.concatenate of the reference's per-image
        statistics, scene after scene.  Reads the cursor and the overflow flag once, then the n rows."""
        tp, conf, pcls = self._read_rows()
        tcls = [t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in self._tcls]
        tcls = np.concatenate(tcls).astype(np.float64) if tcls else np.zeros(0, np.float64)
        return tp.astype(bool), conf, pcls, tcls

    def result(self, host=False):
        """(nt, p, r, ap50, ap, f1, ap_class, mp, mr, map50, map) of test.py:152-164 over everything added so far."""
        return evaluate.calculate_eval_stats(self.stats(), self.num_classes, host)

    def reset(self):
        self._tcls = []
        super().reset()


def _scene_rows(det, dataset, imread, overlap):
    """(s, out, num) for every scene s of a SceneDataset through the TiledDetector `det`.  Scene s + 1 is decoded and uploaded on a side
    stream while scene s runs (TiledDetector.iter_async).  imread: callable(path) -> uint8 HWC BGR; default: the dataset's own decoder (the
    arrays themselves after set_arrays)."""
    files = list(dataset.scene_files)
    if imread is None:
        pool, index = dataset.cache(), {p: i for i, p in enumerate(files)}
        imread = lambda path: pool.host_image(index[path])             # noqa: E731
    for s, (_, out, num) in enumerate(det.iter_async(files, imread=imread, overlap=overlap)):
        yield s, out, num


def evaluate_scenes(det, dataset, imread=None, overlap=True, iouv=None, capacity=1 << 20, host=False):
    """Every scene of a SceneDataset (`scene_files`, `scene_labels(scene)`) through the TiledDetector `det` -> SceneEvaluator.result().
    Per scene the host only enqueues (_scene_rows), and the statistics are read once at the end."""
    ev = SceneEvaluator(det.nc, iouv=iouv, capacity=capacity, device=det.device)
    for s, out, num in _scene_rows(det, dataset, imread, overlap):
        ev.add(out, num, *dataset.scene_labels(s))
    return ev.result(host)
