"""Full-scene detection: a scene far larger than the network input (DOTA scenes run to thousands of pixels per side) is cut into overlapping
windows at the network size, every group of windows runs through ONE captured graph (Yolo.capture_inference(batch, size, post=...): the
forward, the decode and post_process), and the per-window detections are mapped back to scene pixels and merged with class-wise rotated
NMS — the workflow users of the reference rebuild by hand around detect.py, which only letterboxes a whole file to img_size.

    tile_plan(H, W, size, overlap, rates=(1.0,)) -> [(rate_index, x0, y0)]        the window table (host, pure Python)
    tile_entries(H, W, size, overlap, rates, views) -> [(rate_index, x0, y0, view)]  windows x views, window-major
    TiledDetector(model, size, overlap, batch, ...)(scene) -> Tensor[n, 7]          (x, y, w, h, theta_rad, score, cls) in scene pixels
    TiledDetector(..., views=("id", "hflip", "rot90"))                              every window also seen flipped / turned by 90 degrees (VIEWS)
    TiledDetector(..., fuse="box" | "wbf")                                          kept boxes absorb the boxes they suppressed (FUSE)
    TiledDetector(..., seam=Seam(margin=2.0, cover=0.7, whole=True))                window-cut fragments seen whole elsewhere are dropped (Seam)
    TiledDetector.run_async(scene) -> (out [max_det, 7], num [1] int32)             the same with the count left on the device
    TiledDetector.detect_files(paths) -> iterator of (path, Tensor[n, 7])           scene i + 1 decoded / uploaded while scene i runs
    TiledDetector.iter_async(paths) -> iterator of (path, out, num)                 the same with the counts left on the device (lib/scene_eval.py)
    write_dota_task1({name: dets}, out_dir, class_names)                            DOTA Task1 files (Task1_<class>.txt)

Device side (csrc/tiled.hip): a scene's entries are windows x views, window-major (entry e = window_index * len(views) + view_index;
with the default views=("id",) the entries are the windows).  Per group of `batch` entries ryolo_tile_cut_views (scene -> the graph's
static input, every entry's window in its view), the graph replay, ryolo_tile_collect_views (the view's boxes back in the window, then
scene rows at the fixed slot e * mk + j, per-class keys); then per scene ryolo_topk_desc over the nc class rows, ryolo_tile_merge_gather,
ryolo_nms_rotated_batched with batch = nc (no cls * 4096 offset: post_process's class separation collides on scenes wider than 4096 px),
ryolo_tile_mark, ryolo_topk_desc over the kept entries (score desc, slot asc) and ryolo_tile_emit.  No allocation and no host read after the
scene's upload; __call__ reads one count per scene.

Views (test-time orientation ensembling; an overhead scene has no preferred orientation): the views of one window are cut back to
back.  The cut writes an entry's window in its view (flips by index arithmetic, the transposing views through LDS) and the collect maps
the view's boxes back to the window (point, theta wrapped into [-pi/2, pi/2)) in front of the shift; "id" is the view that changes
neither a pixel's place nor a bit of a box.  The merge does not know about views: it keeps the best-scoring box of a cluster.
The definition of the eight views is in include/ryolo.h.

Fusion (fuse="box" | "wbf", default None = the merge above, bit for bit): what makes the extra replays of rates x views pay beyond
recall.  After the NMS, ryolo_nms_owner reads from the NMS's own suppression mask which kept box removed each suppressed one (no second
IoU), and ryolo_tile_fuse, in place of ryolo_tile_mark, lets every kept box absorb its cluster: score-weighted centre, size and angle,
with theta taken modulo pi and (w, h, theta) ~ (h, w, theta +- pi/2) resolved against the kept box; "wbf" also replaces the score by the
mean member score scaled by min(members, n) / n, n = len(rates) * len(views), so a box seen by one view of eight no longer keeps its
full score.  The fused rows go to their own buffer (the candidates are only read) and the final order is taken over the fused scores.
Two more launches per scene, no host read, and no allocation after a plan's first fused merge (which allocates the two buffers).  The arithmetic is defined in include/ryolo.h.

Seams (seam=Seam(...), default None = the merge above, bit for bit, not one launch more; csrc/seam.hip): a window border cuts an object
into a fragment that ends at the border, and the overlapping neighbour sees it whole; the NMS then lets a better-scoring fragment
suppress the whole box, or keeps both.  ryolo_tile_seam_flags, in front of the selection, marks every candidate whose extent touches an
interior border of its own window (within `margin` px) and, rule 1, takes those out of the selection's keys that another window of the
same rate holds whole; ryolo_tile_seam_cover, behind ryolo_tile_mark / ryolo_tile_fuse, rule 2, drops kept cut boxes that a larger kept
box of their class covers by at least `cover` of their area.  The NMS itself, the candidates and `key` are untouched; the buffers are
allocated by a plan's first seam merge; `seam_counts` holds the two drop counts on the device.  The rules are defined in include/ryolo.h.
"""
import math
from collections import OrderedDict

import numpy as np
import torch

from .. import hip
from ..datasets import augment as A
from . import general

_SORT_MAX = 16384            # ryolo_topk_desc selects at most this many entries per row
# the eight flip / 90-degree views of a window; a view's code in the device tables is its index here (include/ryolo.h)
VIEWS = ("id", "hflip", "vflip", "rot180", "transpose", "rot90", "rot270", "antitranspose")


def check_views(views):
    """-> the tuple of view names, validated: known names, no duplicates, not empty."""
    if isinstance(views, str):
        raise ValueError(f"views must be a sequence of names from {VIEWS}, got the string {views!r}")
    views = tuple(views)
    if not views:
        raise ValueError("views must name at least one view")
    for v in views:
        if v not in VIEWS:
            raise ValueError(f"unknown view {v!r}: choose from {VIEWS}")
    if len(set(views)) != len(views):
        raise ValueError(f"views must not repeat, got {views}")
    return views


# cluster fusion of the merge; a mode's code for ryolo_tile_fuse is its index here (include/ryolo.h)
FUSE = ("box", "wbf")


def check_fuse(fuse):
    """-> None, "box" or "wbf", validated."""
    if fuse is None or (isinstance(fuse, str) and fuse in FUSE):
        return fuse
    raise ValueError(f"fuse must be None or one of {FUSE}, got {fuse!r}")


class Seam:
    """Seam handling of the merge (include/ryolo.h states the rules).  margin: a box side within `margin` window pixels of an interior
    border of its own window counts as cut by it.  whole (rule 1): a cut box is left out of the merge when another window of the same
    rate holds it clear of its own borders.  cover (rule 2; None = off): a kept cut box is dropped when a larger kept box of its class
    covers at least this share of its area."""
    __slots__ = ("margin", "cover", "whole")

    def __init__(self, margin=2.0, cover=0.7, whole=True):
        if isinstance(margin, bool) or not isinstance(margin, (int, float, np.integer, np.floating)) or not math.isfinite(margin) or margin < 0:
            raise ValueError(f"Seam: margin must be a finite number >= 0 (window pixels), got {margin!r}")
        if cover is not None and (isinstance(cover, bool) or not isinstance(cover, (int, float, np.integer, np.floating))
                                  or not 0.05 <= cover <= 1):
            raise ValueError(f"Seam: cover must be None or lie in [0.05, 1], got {cover!r}")
        if not isinstance(whole, (bool, np.bool_)):
            raise ValueError(f"Seam: whole must be a bool, got {whole!r}")
        if not whole and cover is None:
            raise ValueError("Seam: whole=False with cover=None leaves no rule; pass seam=None instead")
        self.margin, self.cover, self.whole = float(margin), None if cover is None else float(cover), bool(whole)

    def __repr__(self):
        return f"Seam(margin={self.margin}, cover={self.cover}, whole={self.whole})"

    def __eq__(self, other):
        return isinstance(other, Seam) and (self.margin, self.cover, self.whole) == (other.margin, other.cover, other.whole)

    def __hash__(self):
        return hash((self.margin, self.cover, self.whole))


def check_seam(seam):
    """-> None or a Seam, validated; a dict of Seam's arguments is accepted."""
    if seam is None:
        return None
    if isinstance(seam, dict):
        try:
            return Seam(**seam)
        except TypeError as e:
            raise ValueError(f"seam: {e}") from None
    if isinstance(seam, Seam):
        return Seam(seam.margin, seam.cover, seam.whole)                 # attributes set after construction are checked again
    raise ValueError(f"seam must be None, a Seam or a dict of its arguments, got {seam!r}")


# ------------------------------------------------------------------------------------------ window plan
def resized_extent(H, W, rate):
    """(h, w) of the scene resized by `rate`."""
    return int(H * rate + 0.5), int(W * rate + 0.5)


def axis_starts(L, size, stride):
    """Window starts along an axis of length L (tile_plan states the rule)."""
    if L <= size:
        return [0]
    out, x = [], 0
    while x + size < L:
        out.append(x)
        x += stride
    out.append(L - size)
    return out


def tile_plan(H, W, size, overlap, rates=(1.0,)):
    """Windows of an H x W scene: [(rate_index, x0, y0)], row-major by rate, then y0, then x0 (this order fixes the tie-breaks of the
    merge).  Per rate the scene is resized to resized_extent(H, W, rate); along an axis of length L the starts are 0, stride, 2 * stride,
    ... (stride = size - overlap) up to the first start x with x + size >= L, which becomes L - size; an axis no longer than `size` has
    the single start 0 (the window reaches past the scene and is filled with 114 grey)."""
    if not isinstance(size, (int, np.integer)) or size <= 0 or size % 32:
        raise ValueError(f"tile_plan: size must be a positive multiple of 32 (the largest head stride), got {size}")
    if not isinstance(overlap, (int, np.integer)) or not 0 <= overlap < size:
        raise ValueError(f"tile_plan: overlap must satisfy 0 <= overlap < size, got {overlap}")
    rates = tuple(rates)
    if not rates or any(not (float(r) > 0) or not math.isfinite(float(r)) for r in rates):
        raise ValueError(f"tile_plan: rates must be positive, got {rates}")
    if int(H) <= 0 or int(W) <= 0:
        raise ValueError(f"tile_plan: empty scene {H} x {W}")
    stride = size - overlap
    out = []
    for ri, r in enumerate(rates):
        h, w = resized_extent(H, W, float(r))
        if h <= 0 or w <= 0:
            raise ValueError(f"tile_plan: rate {r} leaves nothing of a {H} x {W} scene")
        xs = axis_starts(w, size, stride)
        for y0 in axis_starts(h, size, stride):
            out.extend((ri, x0, y0) for x0 in xs)
    return out


def tile_entries(H, W, size, overlap, rates=(1.0,), views=("id",)):
    """Entries of a scene: [(rate_index, x0, y0, view name)], every window of tile_plan once per view, window-major: entry
    e = window_index * len(views) + view_index.  Detection j of entry e takes candidate slot e * mk + j."""
    views = check_views(views)
    return [(ri, x0, y0, v) for ri, x0, y0 in tile_plan(H, W, size, overlap, rates) for v in views]


# ------------------------------------------------------------------------------------------ per-scene-shape buffers
def _h2d(dst, arr):
    """Small host table -> existing device tensor through pinned memory, non-blocking on the current stream."""
    stage = torch.empty(dst.shape, dtype=dst.dtype, pin_memory=True)
    stage.numpy()[...] = arr
    dst.copy_(stage, non_blocking=True)


class ScenePlan:
    """Static buffers of one (H, W, rates, views): entry table, candidate rows, class keys, merge and final-order buffers, resized copies.
    `det` supplies device, batch, mk (detection rows per window), nc, size, overlap, rates, max_nms and max_det (a TiledDetector) and
    optionally views (default ("id",)).  An entry is a window seen through a view: entries = windows x views, window-major; T counts
    entries, and groups of `batch` entries share one replay.  The tables carry every entry's view code (its index in VIEWS, 0 for "id")
    for ryolo_tile_cut_views / ryolo_tile_collect_views."""

    def __init__(self, det, H, W):
        dev, B, mk, nc, S = det.device, det.batch, det.mk, det.nc, det.size
        self.H, self.W = H, W
        self.batch, self.mk, self.nc, self.max_det = B, mk, nc, det.max_det
        self.size = S
        self.views = check_views(getattr(det, "views", ("id",)))
        self.windows = tile_plan(H, W, S, det.overlap, det.rates)
        self.entries = tile_entries(H, W, S, det.overlap, det.rates, self.views)
        self.extents = [resized_extent(H, W, r) for r in det.rates]
        T = self.T = len(self.entries)
        self.groups = (T + B - 1) // B
        ld = self.ld = self.groups * B * mk
        f32, i32, i64 = torch.float32, torch.int32, torch.int64
        wa = np.asarray([e[:3] for e in self.entries], dtype=np.int64).reshape(-1, 3)
        code = np.asarray([VIEWS.index(e[3]) for e in self.entries], dtype=np.int64)
        ext = np.asarray(self.extents, dtype=np.int64)
        # win rows (src_off, set per scene; source height, width; x0, y0; view code) and geom rows (x0, y0, rate, view code)
        self.rows = np.stack([np.zeros(T, np.int64), ext[wa[:, 0], 0], ext[wa[:, 0], 1], wa[:, 1], wa[:, 2], code], 1)
        self.rate_of = wa[:, 0]
        self.win = torch.empty((T, 6), dtype=i64, device=dev)
        self.geom = torch.empty((T, 4), dtype=f32, device=dev)
        _h2d(self.geom, np.stack([wa[:, 1], wa[:, 2], np.asarray(det.rates, np.float32)[wa[:, 0]], code], 1).astype(np.float32))
        # resized copies of the scene (rates != 1), one staging buffer
        self.stage_off, total = [], 0
        for r, (h, w) in zip(det.rates, self.extents):
            self.stage_off.append(total if r != 1.0 else None)
            if r != 1.0:
                total += ((h * w * 3 + 15) // 16) * 16
        self.stage = torch.empty(max(total, 16), dtype=torch.uint8, device=dev)
        self.resize_items = [(ri, h, w) for ri, (r, (h, w)) in enumerate(zip(det.rates, self.extents)) if r != 1.0]
        # candidates and keys: every slot is written by ryolo_tile_collect_views
        self.cand = torch.empty((ld, 7), dtype=f32, device=dev)
        self.key = torch.empty((nc, ld), dtype=f32, device=dev)
        self.fkey = torch.empty(ld, dtype=f32, device=dev)
        self.Kc, self.Kf = min(det.max_nms, ld), min(det.max_det, ld)
        # one sort workspace for both selections: the per-class one and the final one
        sort_bytes = max(hip.workspace_bytes("ryolo_sort_workspace_bytes", nc, self.Kc), hip.workspace_bytes("ryolo_sort_workspace_bytes", 1, self.Kf))
        self.sort_ws = torch.empty(max(sort_bytes, 16), dtype=torch.uint8, device=dev)
        self.skey = torch.empty((nc, self.Kc), dtype=f32, device=dev)
        self.order = torch.empty((nc, self.Kc), dtype=i64, device=dev)
        self.nsel = torch.empty(nc, dtype=i32, device=dev)
        self.rboxes = torch.empty((nc, self.Kc, 5), dtype=f32, device=dev)
        self.nms_ws = hip.workspace("ryolo_nms_workspace_bytes", nc, self.Kc, device=dev)
        self.keep = torch.empty((nc, self.Kc), dtype=i64, device=dev)
        self.nkeep = torch.empty(nc, dtype=i32, device=dev)
        self.fskey = torch.empty((1, self.Kf), dtype=f32, device=dev)
        self.forder = torch.empty((1, self.Kf), dtype=i64, device=dev)
        self.num = torch.empty(1, dtype=i32, device=dev)
        self.out = torch.empty((self.max_det, 7), dtype=f32, device=dev)
        # cluster fusion (merge(..., fuse=...)): the owner of every sorted position and the fused rows, by candidate slot.  Allocated by
        # the first fused merge of the plan, so a detector that never fuses holds exactly the buffers it always held
        self.n_ens = len(det.rates) * len(self.views)
        self.owner = self.fused = None
        # seam handling (merge_seam(..., seam=...)): cut / redundant bits by slot, the keys the first selection reads under rule 1 plus one
        # row for the seam merge's own final key, the two drop counts and rule 2's workspace.  Allocated by the first seam merge of the plan, like the fusion buffers
        self.nviews = len(self.views)
        self.flags = self.key2 = self.seam_counts = self.seam_ws = None

    def cut(self, scene, g, dst):
        """Group g's entries of the scene at device address `scene` -> dst [batch, 3, size, size] (slots past the last entry untouched)."""
        e0 = g * self.batch
        hip.call("ryolo_tile_cut_views", scene, hip.ptr(self.win), e0, min(self.batch, self.T - e0), self.size, hip.ptr(dst), hip.stream())

    def collect(self, dets, num, g):
        """Group g's post_process output dets [batch, mk, 7] / num [batch] -> candidate rows and class keys of its slots."""
        B = self.batch
        hip.call("ryolo_tile_collect_views", hip.ptr(dets), hip.ptr(num), B, self.mk, hip.ptr(self.geom), g * B, self.T, self.nc, self.ld,
                 self.size, hip.ptr(self.cand), hip.ptr(self.key), hip.ptr(self.fkey), hip.stream())

    def merge(self, merge_iou, gt_only=True, fuse=None):
        """Class-wise rotated NMS over every collected candidate, then the final order -> (out [max_det, 7], num [1]) on the device.
        fuse None: a kept box is emitted as it is.  "box" / "wbf": it absorbs the boxes it suppressed (ryolo_nms_owner + ryolo_tile_fuse
        in place of ryolo_tile_mark, the rows emitted from `fused`); the candidates are only read, so the modes can follow each other on
        the same collected scene.  This is merge_seam without a seam: the launches it always issued, and no other."""
        return self.merge_seam(merge_iou, gt_only, fuse, None)

    def merge_seam(self, merge_iou, gt_only=True, fuse=None, seam=None):
        """merge with the seam rules (merge's own parameter list is pinned by tests/test_tiled_fusion_cpu.py, so seam has a method of its
        own).  seam None: merge, nothing more is launched.  A Seam (or a dict of its arguments): ryolo_tile_seam_flags in front of the selection, which
        under rule 1 reads `key2` (the keys without the cut rows another window holds whole), and under rule 2 ryolo_tile_seam_cover behind
        ryolo_tile_mark / ryolo_tile_fuse (kept cut rows that a larger kept box covers leave the final order).  `seam_counts` int32 [2]
        holds the rows the two rules dropped in this merge, on the device.  A seam merge marks its kept slots in a key of its own (the
        last row of `key2`, reset per merge), not in `fkey`: merges with and without seam can follow each other on the same collected
        scene, and seam=None afterwards is the plain result bit for bit.  The window table `win` must hold the scene's rows
        (TiledDetector uploads it per scene); the candidates and `key` are only read."""
        fuse, seam = check_fuse(fuse), check_seam(seam)
        nc, Kc, Kf, st = self.nc, self.Kc, self.Kf, hip.stream()
        key, fkey = self.key, self.fkey
        if seam is not None:
            if self.flags is None:
                dev = self.cand.device
                self.flags = torch.empty(self.ld, dtype=torch.uint8, device=dev)
                self.seam_counts = torch.empty(2, dtype=torch.int32, device=dev)
                self.seam_ws = hip.workspace("ryolo_tile_seam_workspace_bytes", nc, Kc, device=dev)
                self.key2 = torch.empty((nc + 1, self.ld), dtype=torch.float32, device=dev)
            hip.call("ryolo_tile_seam_flags", hip.ptr(self.cand), hip.ptr(self.key), hip.ptr(self.win), hip.ptr(self.geom), self.T, self.nviews,
                     self.mk, self.ld, nc, self.size, seam.margin, 1 if seam.whole else 0, hip.ptr(self.flags),
                     hip.ptr(self.key2), hip.ptr(self.seam_counts), st)
            if seam.whole:
                key = self.key2
            fkey = self.key2[nc]                                         # the seam merge's own final key (include/ryolo.h)
        hip.call("ryolo_topk_desc", hip.ptr(key), nc, self.ld, Kc, hip.ptr(self.skey), hip.ptr(self.order), hip.ptr(self.nsel), hip.ptr(self.sort_ws),
                 self.sort_ws.numel(), st)
        hip.call("ryolo_tile_merge_gather", hip.ptr(self.cand), hip.ptr(self.skey), hip.ptr(self.order), nc, Kc, hip.ptr(self.rboxes), st)
        hip.call("ryolo_nms_rotated_batched", hip.ptr(self.rboxes), hip.ptr(self.nsel), nc, Kc, merge_iou, 1 if gt_only else 0, Kc,
                 hip.ptr(self.nms_ws), self.nms_ws.numel(), hip.ptr(self.keep), Kc, hip.ptr(self.nkeep), st)
        if fuse is None:
            hip.call("ryolo_tile_mark", hip.ptr(self.skey), hip.ptr(self.order), hip.ptr(self.keep), hip.ptr(self.nkeep), nc, Kc, Kc, hip.ptr(fkey), st)
            rows = self.cand
        else:
            if self.fused is None:
                self.owner = torch.empty((nc, Kc), dtype=torch.int32, device=self.cand.device)
                self.fused = torch.empty((self.ld, 7), dtype=torch.float32, device=self.cand.device)
            hip.call("ryolo_nms_owner", hip.ptr(self.nsel), nc, Kc, hip.ptr(self.nms_ws), self.nms_ws.numel(), hip.ptr(self.keep), Kc,
                     hip.ptr(self.nkeep), hip.ptr(self.owner), st)
            hip.call("ryolo_tile_fuse", hip.ptr(self.cand), hip.ptr(self.order), hip.ptr(self.nsel), hip.ptr(self.keep), hip.ptr(self.nkeep),
                     hip.ptr(self.owner), nc, Kc, Kc, self.ld, FUSE.index(fuse), self.n_ens, hip.ptr(self.fused), hip.ptr(fkey), st)
            rows = self.fused
        if seam is not None and seam.cover is not None:
            hip.call("ryolo_tile_seam_cover", hip.ptr(self.rboxes), hip.ptr(self.order), hip.ptr(self.nsel), hip.ptr(self.keep), hip.ptr(self.nkeep),
                     nc, Kc, Kc, hip.ptr(self.flags), self.ld, seam.cover, hip.ptr(fkey), hip.ptr(self.seam_counts), hip.ptr(self.seam_ws),
                     self.seam_ws.numel(), st)
        hip.call("ryolo_topk_desc", hip.ptr(fkey), 1, self.ld, Kf, hip.ptr(self.fskey), hip.ptr(self.forder), hip.ptr(self.num), hip.ptr(self.sort_ws),
                 self.sort_ws.numel(), st)
        hip.call("ryolo_tile_emit", hip.ptr(rows), hip.ptr(self.forder), hip.ptr(self.num), self.max_det, hip.ptr(self.out), st)
        return self.out, self.num


class _Placed:
    """A scene resident on the device: `base` tensor + byte offset (what the table-driven kernels take), and the object that owns it."""

    def __init__(self, base, off, H, W, owner):
        self.base, self.off, self.H, self.W, self.owner = base, off, H, W, owner

    @property
    def addr(self):
        return self.base.data_ptr() + self.off


# ------------------------------------------------------------------------------------------ detector
class TiledDetector:
    """Detect on full scenes with one captured graph of an eval-mode Yolo (see the module docstring).

    conf_thres / iou_thres: post_process of every window (captured with the graph).  merge_iou (default iou_thres) and gt_only: the
    class-wise rotated NMS of the merge.  rates: the scene is resized once per rate (INTER_AREA below 1, INTER_LINEAR above; rate 1 is cut
    straight from the scene) and every resized copy is tiled; boxes are mapped back to the original scene.  max_nms: candidates per class
    entering the merge; max_det: detections per scene.  views: names from VIEWS, in the order their entries take inside a window; every
    window runs once per view and all views' boxes enter the one merge, which keeps the best-scoring box of a cluster.  fuse: None
    emits that box as it is; "box" replaces its geometry by the score-weighted rotated mean of the cluster it suppressed (box voting),
    score unchanged; "wbf" does the same and sets the score to the mean member score times min(members, n) / n, n = len(rates) *
    len(views) (weighted box fusion).  The arithmetic is defined in include/ryolo.h (ryolo_tile_fuse)."""

    def __init__(self, model, size=1024, overlap=200, batch=8, conf_thres=0.1, iou_thres=0.4, merge_iou=None, rates=(1.0,), max_nms=5000,
                 max_det=5000, gt_only=True, views=("id",), fuse=None, seam=None):
        rates = tuple(float(r) for r in rates)
        views = check_views(views)
        self.fuse = check_fuse(fuse)                                     # read per scene, like views and rates
        self.seam = check_seam(seam)                                     # read per scene too
        tile_plan(size, size, size, overlap, rates)                      # argument validation
        if int(batch) < 1:
            raise ValueError(f"TiledDetector: batch must be >= 1, got {batch}")
        for name, v in (("max_nms", max_nms), ("max_det", max_det)):
            if not 1 <= int(v) <= _SORT_MAX:
                raise ValueError(f"TiledDetector: {name} must lie in [1, {_SORT_MAX}], got {v}")
        if model.training:
            raise RuntimeError("TiledDetector: call model.eval() first")
        self.size, self.overlap, self.batch, self.rates, self.views = int(size), int(overlap), int(batch), rates, views
        self.conf_thres, self.iou_thres = float(conf_thres), float(iou_thres)
        self.merge_iou = self.iou_thres if merge_iou is None else float(merge_iou)
        self.max_nms, self.max_det, self.gt_only = int(max_nms), int(max_det), bool(gt_only)
        # the graph replays into the model's runtime buffers (weights, activations): the detector keeps the model alive with it
        self.model = model
        self.run = model.capture_inference(self.batch, self.size, post=(self.conf_thres, self.iou_thres))
        self.device = self.run.static_input.device
        self.nc, self.mk = self.run.post_plan.nc, self.run.post_plan.mk
        self._plans = OrderedDict()          # (H, W, rates, views) -> ScenePlan, least recently used first
        self._plans_max = 4
        self._side = None

    # ---- buffers
    def plan(self, H, W):
        key = (int(H), int(W), self.rates, tuple(self.views))
        p = self._plans.pop(key, None)
        if p is None:
            while len(self._plans) >= self._plans_max:
                torch.cuda.synchronize(self.device)                   # launches still reading the evicted buffers finish first
                self._plans.popitem(last=False)
            p = ScenePlan(self, int(H), int(W))
        self._plans[key] = p
        return p

    # ---- scene placement
    def _place(self, scene):
        if isinstance(scene, torch.Tensor):
            hip.require_device(scene, "TiledDetector")
            if scene.dtype != torch.uint8 or scene.dim() != 3 or scene.shape[2] != 3 or not scene.is_contiguous():
                raise RuntimeError("TiledDetector: a device scene must be a contiguous uint8 [H, W, 3] (BGR) tensor")
            return _Placed(scene, 0, scene.shape[0], scene.shape[1], scene)
        img = np.asarray(scene)
        if img.dtype != np.uint8 or img.ndim not in (2, 3):
            raise RuntimeError("TiledDetector: a host scene must be a uint8 H x W x 3 (BGR) array")
        pool = A.ImagePool([img], self.device)                           # pinned staging + non-blocking upload (grey -> 3 channels)
        H, W = pool.shape(0)
        return _Placed(pool.buf, pool.offset(0), H, W, pool)

    # ---- the device pipeline of one scene
    def _enqueue(self, placed):
        fuse = check_fuse(self.fuse)                                     # a bad mode set on the detector fails before anything is launched
        seam = check_seam(self.seam)
        H, W = placed.H, placed.W
        p = self.plan(H, W)
        st = hip.stream()
        scene = placed.addr
        src = []
        if p.resize_items:
            A._check_layouts()
            arr = (A._ResizeItem * len(p.resize_items))()
            for k, (ri, h, w) in enumerate(p.resize_items):
                arr[k] = A._ResizeItem(0, p.stage_off[ri], H, W, h, w, A.INTERP_AREA if self.rates[ri] < 1 else A.INTERP_LINEAR, -1)
            items = A._to_device(arr, self.device)
            hip.call("ryolo_resize_hsv_batch", scene, hip.ptr(items), len(p.resize_items), max(h * w for _, h, w in p.resize_items), None,
                     hip.ptr(p.stage), st)
        for ri, r in enumerate(self.rates):
            src.append(0 if p.stage_off[ri] is None else p.stage.data_ptr() + p.stage_off[ri] - scene)
        rows = p.rows.copy()
        rows[:, 0] = np.asarray(src, dtype=np.int64)[p.rate_of]
        _h2d(p.win, rows)
        run = self.run
        for g in range(p.groups):
            p.cut(scene, g, run.static_input)
            run.graph.replay()
            p.collect(run.post_plan.out, run.post_plan.num, g)
        return p.merge_seam(self.merge_iou, self.gt_only, fuse, seam)

    # ---- public
    def run_async(self, scene):
        """-> (out [max_det, 7] zero padded, num [1] int32), both on the device and owned by the detector (valid until the next scene of the
        same size).  Nothing is read back."""
        placed = self._place(scene)
        out, num = self._enqueue(placed)
        self._last = placed                  # the scene's memory stays referenced while its launches may be pending
        return out, num

    def __call__(self, scene):
        """HxWx3 uint8 BGR numpy array (cv2.imread) or device tensor -> Tensor[n, 7] (x, y, w, h, theta_rad, score, cls) in scene pixels,
        score descending (ties: window order, then the order of `views`, then the entry's own order)."""
        out, num = self.run_async(scene)
        n = int(num.item())                  # the one device -> host read of the scene
        return out[:n].clone()

    def detect_files(self, paths, imread=None, overlap=True):
        """Iterate (path, Tensor[n, 7]) over image files: iter_async plus the count read and a copy of the rows.  overlap=True: scene
        i + 1 is decoded on the host and uploaded on a side stream while scene i runs, since iter_async issues both before it hands
        scene i over, and only then does the host block here on scene i's count; the compute stream waits for the upload's event
        (DeviceLoader's pattern).  Scene i's memory follows iter_async's rule: it is released behind an event recorded after scene i's
        launches (one record and one wait per scene), not behind this count read."""
        for path, out, num in self.iter_async(paths, imread, overlap):
            yield path, out[:int(num.item())].clone()

    def iter_async(self, paths, imread=None, overlap=True):
        """The prefetch loop over image files: iterate (path, out [max_det, 7], num [1] int32), both on the device and owned by the
        detector as run_async returns them — valid until the consumer asks for the next scene, and whatever it launches on them must go
        to the current stream.  Nothing is read back and nothing waits for the device.  overlap=True: scene i + 1 is decoded and uploaded
        on a side stream while scene i runs; its memory is released to that stream only behind an event recorded after scene i's
        launches, since no host read says that they are done."""
        from ..datasets.base_dataset import _default_imread
        imread = imread or _default_imread
        paths = list(paths)
        main = torch.cuda.current_stream(self.device)
        if overlap and self._side is None:
            self._side = torch.cuda.Stream(device=self.device)

        def load(path):
            if not overlap:
                return self._place(imread(path)), None
            with torch.cuda.stream(self._side):
                placed = self._place(imread(path))
                return placed, self._side.record_event()

        nxt = load(paths[0]) if paths else None
        for i, path in enumerate(paths):
            placed, ev = nxt
            if ev is not None:
                main.wait_event(ev)
            out, num = self._enqueue(placed)
            if overlap:
                done = main.record_event()
                nxt = load(paths[i + 1]) if i + 1 < len(paths) else None
                self._side.wait_event(done)   # a later upload may take scene i's memory: it starts after scene i's launches
            else:
                self._last = placed           # one stream: reuse is ordered by it (run_async's rule)
            del placed
            yield path, out, num
            if not overlap and i + 1 < len(paths):
                nxt = load(paths[i + 1])


# ------------------------------------------------------------------------------------------ DOTA Task1 output
def write_dota_task1(results, out_dir, class_names):
    """results {image name: Tensor[n, 7] (x, y, w, h, theta_rad, score, cls) on the device} -> out_dir/Task1_<class>.txt for every class
    (DOTA's submission format): one line per detection, "name score x1 y1 x2 y2 x3 y3 x4 y4", vertices from xywha2xyxyxyxy on the device;
    images in the order of `results`, detections in their order.  Returns the list of files written."""
    import os
    os.makedirs(out_dir, exist_ok=True)
    lines = [[] for _ in class_names]
    for name, dets in results.items():
        if dets is None or dets.shape[0] == 0:
            continue
        d = dets if dets.is_cuda else dets.to(torch.device("cuda", torch.cuda.current_device()))
        polys = general.xywha2xyxyxyxy(d[:, :5].contiguous()).reshape(-1, 8).cpu().numpy()
        sc = d[:, 5].cpu().numpy()
        cl = d[:, 6].cpu().numpy().astype(np.int64)
        for k in range(len(sc)):
            if not 0 <= cl[k] < len(class_names):
                raise ValueError(f"write_dota_task1: class {cl[k]} of {name} has no name")
            lines[cl[k]].append(f"{name} {sc[k]:.6f} " + " ".join(f"{v:.1f}" for v in polys[k]))
    files = []
    for c, cname in enumerate(class_names):
        path = os.path.join(out_dir, f"Task1_{cname}.txt")
        with open(path, "w") as f:
            f.write("".join(line + "\n" for line in lines[c]))
        files.append(path)
    return files
