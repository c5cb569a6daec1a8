"""Training and validation on full-size labelled scenes: the windows are cut on the device, batch by batch.

The reference trains on windows that an external devkit cut offline (data/DOTA.yaml: data/DOTA/split/train); it has no code for this
stage, as it has none for tiled detection (lib/tiled.py).  Here a dataset ITEM is a planned window of a scene; the ImagePool holds the
scenes, and the first stage of BaseDataset.assemble_batch — the source image of a use and the labels that belong to it — reads through
the window (csrc/scene.hip):

    ryolo_resize_hsv_windows   load_image's resize + hsv of the window, bit-identical to ryolo_resize_hsv_batch on the c x c cut
                               (114 where the window lies outside the scene), without a cut pass;
    ryolo_scene_label_rows     shift by the window origin, keep a label when intersection-over-foreground with the window reaches
                               `iof_thr`; dropped rows become NaN rows, which the rest of the chain already removes in order.

Everything downstream (mosaic / mixup / warp / hsv, the draws from `rng` in the reference's order, label_stage, encode_labels) is
BaseDataset's, unchanged.  With `jitter` every use of an item redraws its window origin from a private random.Random(window_seed), so
the crop positions are not fixed for the run as an offline split fixes them.  tests/scene_ref.py restates the semantics in numpy.
"""
import glob
import math
import os
import random as _py_random

import numpy as np
import torch

from . import augment as A
from .base_dataset import BaseDataset
from .copy_paste import CopyPaste, strictly_convex
from .DOTA_dataset import DOTADataset
from ..lib.tiled import axis_starts


def scene_windows(H, W, size, overlap, rates=(1.0,)):
    """Planned windows of an H x W scene in SCENE pixels: [(rate_index, x0, y0, c)], ordered by rate, then y0, then x0.  At rate r a
    window has side c = int(size / r + 0.5) (it is resized to size x size by the pixel stage) and the stride is c - int(overlap / r +
    0.5); starts along an axis as lib/tiled.py places them (an axis no longer than c: the single start 0, the window hangs over the
    scene).  rates=(1.0,) gives tiled.tile_plan's windows with c = size."""
    if not isinstance(size, (int, np.integer)) or size <= 0 or size % 32:
        raise ValueError(f"scene_windows: size must be a positive multiple of 32 (the largest head stride), got {size}")
    if not isinstance(overlap, (int, np.integer)) or not 0 <= overlap < size:
        raise ValueError(f"scene_windows: overlap must satisfy 0 <= overlap < size, got {overlap}")
    rates = tuple(rates)
    if not rates or any(not (float(r) > 0) or not math.isfinite(float(r)) for r in rates):
        raise ValueError(f"scene_windows: rates must be positive, got {rates}")
    if int(H) <= 0 or int(W) <= 0:
        raise ValueError(f"scene_windows: empty scene {H} x {W}")
    out = []
    for ri, r in enumerate(rates):
        c = int(size / float(r) + 0.5)
        stride = c - int(overlap / float(r) + 0.5)
        if c <= 0 or stride <= 0 or c >= A.WINDOW_COORD_MAX:
            raise ValueError(f"scene_windows: rate {r} gives a window of {c} pixels with stride {stride}")
        xs = axis_starts(int(W), c, stride)
        for y0 in axis_starts(int(H), c, stride):
            out.extend((ri, x0, y0, c) for x0 in xs)
    return out


def jitter_window(wrng, H, W, c, polys, p_object):
    """One redraw of a window origin in an H x W scene: per axis randint(min(0, L - c), max(0, L - c)) (a scene smaller than the window
    floats inside it: negative origins).  With probability p_object, if the scene has labels, one label is drawn and the range of each
    axis is intersected with [ceil(m) - c + 1, floor(m)], m the label's mean vertex (an empty intersection: the whole range).  Draw
    order: the coin, the label index if drawn, x, y."""
    rx, ry = (min(0, W - c), max(0, W - c)), (min(0, H - c), max(0, H - c))
    if wrng.random() < p_object and len(polys):
        p = polys[wrng.randrange(len(polys))]
        mx = (float(p[0]) + float(p[2]) + float(p[4]) + float(p[6])) / 4.0
        my = (float(p[1]) + float(p[3]) + float(p[5]) + float(p[7])) / 4.0
        ax, bx = max(rx[0], math.ceil(mx) - c + 1), min(rx[1], math.floor(mx))
        ay, by = max(ry[0], math.ceil(my) - c + 1), min(ry[1], math.floor(my))
        if ax <= bx:
            rx = (ax, bx)
        if ay <= by:
            ry = (ay, by)
    x0 = wrng.randint(*rx)
    return x0, wrng.randint(*ry)


def label_boxes(polys):
    """(min x, max x, min y, max y) per label, float32 [4, n]."""
    polys = np.asarray(polys, dtype=np.float32).reshape(-1, 8)
    xs, ys = polys[:, 0::2], polys[:, 1::2]
    if not len(polys):
        return np.zeros((4, 0), dtype=np.float32)
    return np.stack([xs.min(1), xs.max(1), ys.min(1), ys.max(1)])


def cull_labels(polys, x0, y0, c, boxes=None):
    """Indices (file order) of the labels whose axis-aligned bounding box overlaps the window with positive extent; every other label has
    intersection-over-foreground 0 with it, so leaving it out of the table cannot change a result."""
    b = label_boxes(polys) if boxes is None else boxes
    return np.nonzero((b[1] > x0) & (b[0] < x0 + c) & (b[3] > y0) & (b[2] < y0 + c))[0]


class Ignore:
    """Ignore regions of window training (SceneDataset(ignore=...)).  A label of which the window holds less than `iof_thr` of the area is
    no target, yet its pixels are in the window; with this option every such label that keeps at least the share `iof_lo` becomes an IGNORE
    ROW of the batch (`dataset.last_ignore`), under which the criterion's objectness term neither rewards nor punishes a prediction
    (include/ryolo.h, ryolo_loss).  difficult=True: labels the DOTA / VOC protocol calls difficult are ignore rows too, and no targets —
    what DotaEvaluator does with detections on them.  Off by default; the effect on DOTA mAP has not been measured."""
    __slots__ = ("iof_lo", "difficult")

    def __init__(self, iof_lo=0.1, difficult=True):
        if isinstance(iof_lo, bool) or not isinstance(iof_lo, (int, float, np.integer, np.floating)) or not math.isfinite(iof_lo) or not 0 < iof_lo < 1:
            raise ValueError(f"Ignore: iof_lo must be a number in (0, 1), below the dataset's iof_thr, got {iof_lo!r}")
        if not isinstance(difficult, (bool, np.bool_)):
            raise ValueError(f"Ignore: difficult must be a bool, got {difficult!r}")
        self.iof_lo, self.difficult = float(iof_lo), bool(difficult)

    def __repr__(self):
        return f"Ignore(iof_lo={self.iof_lo}, difficult={self.difficult})"

    def __eq__(self, other):
        return isinstance(other, Ignore) and (self.iof_lo, self.difficult) == (other.iof_lo, other.difficult)

    def __hash__(self):
        return hash((self.iof_lo, self.difficult))


def check_ignore(ignore, iof_thr):
    """-> None or an Ignore, validated against the dataset's iof_thr (0 < iof_lo < iof_thr); a dict of Ignore's arguments is accepted."""
    if ignore is None:
        return None
    if isinstance(ignore, dict):
        try:
            ignore = Ignore(**ignore)
        except TypeError as e:
            raise ValueError(f"ignore: {e}") from None
    elif isinstance(ignore, Ignore):
        ignore = Ignore(ignore.iof_lo, ignore.difficult)              # attributes set after construction are checked again
    else:
        raise ValueError(f"ignore must be None, an Ignore or a dict of its arguments, got {ignore!r}")
    if not ignore.iof_lo < float(iof_thr):
        raise ValueError(f"ignore: iof_lo must satisfy 0 < iof_lo < iof_thr = {iof_thr}, got {ignore.iof_lo}")
    return ignore


class Rotate:
    """Rotation augmentation of window training (SceneDataset(rotate=...)): a use's window is read from the scene at a random angle about its
    centre pixel (INTERP_ROT of ryolo_resize_hsv_windows), so the corners of the result hold scene pixels — and the scene's labels under
    the same map — instead of the fill that hyp["rotate"] leaves when it turns a finished canvas.  Per use one coin from a private
    random.Random(seed); under `p` one angle uniform in [-degrees, degrees]; with step > 0 it becomes k * step, k the nearest integer to
    angle / step (Python's round: halves to even) clamped to |k| <= floor(degrees / step), so a snapped angle never leaves the range.
    Off by default; the effect on DOTA mAP has not been measured."""
    __slots__ = ("degrees", "p", "step", "seed", "_rng")

    def __init__(self, degrees=180.0, p=0.5, step=0.0, seed=0):
        for name, v in (("degrees", degrees), ("p", p), ("step", step)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"Rotate: {name} must be a finite number >= 0, got {v!r}")
        if p > 1:
            raise ValueError(f"Rotate: p is a probability, got {p!r}")
        self.degrees, self.p, self.step, self.seed = float(degrees), float(p), float(step), seed
        self._rng = _py_random.Random(seed)

    def draw(self):
        """The angle of one use in degrees, or None for an unrotated use.  Draw order: the coin, then the angle if the coin is under p."""
        if not self._rng.random() < self.p:
            return None
        a = self._rng.uniform(-self.degrees, self.degrees)
        if self.step > 0:
            kmax = math.floor(self.degrees / self.step)
            a = max(-kmax, min(kmax, round(a / self.step))) * self.step
        return a

    def __repr__(self):
        return f"Rotate(degrees={self.degrees}, p={self.p}, step={self.step}, seed={self.seed!r})"


def check_rotate(rotate, augment):
    """-> None or a Rotate with a generator of its own at the start of its seed; a dict of Rotate's arguments is accepted."""
    if rotate is None:
        return None
    if isinstance(rotate, dict):
        try:
            rotate = Rotate(**rotate)
        except TypeError as e:
            raise ValueError(f"rotate: {e}") from None
    elif isinstance(rotate, Rotate):
        rotate = Rotate(rotate.degrees, rotate.p, rotate.step, rotate.seed)
    else:
        raise ValueError(f"rotate must be None, a Rotate or a dict of its arguments, got {rotate!r}")
    if not augment:
        raise ValueError("SceneDataset: rotate is an augmentation (augment=True); validation and label_table() read the planned windows")
    return rotate


def rot_window_box(x0, y0, c, phi_deg):
    """(xlo, xhi, ylo, yhi): the axis-aligned bounding box, in scene coordinates, of the window frame [0, c]^2 of a use rotated by phi_deg
    (the corners through the inverse of rot_window_maps' fwd)."""
    _, f = A.rot_window_maps(x0, y0, c, c, phi_deg)
    k = (c - 1) / 2.0
    xs, ys = [], []
    for u in (0.0, float(c)):
        for v in (0.0, float(c)):
            xs.append(x0 + k + f[0] * (u - k) - f[1] * (v - k))                 # q + R (corner - k), R = fwd's rotation transposed
            ys.append(y0 + k + f[1] * (u - k) + f[0] * (v - k))
    return min(xs), max(xs), min(ys), max(ys)


class SceneDataset(BaseDataset):
    """BaseDataset whose items are windows of scenes.  Subclasses fill `scene_files` / `scene_label_files`, implement `load_files` and call
    `plan_windows()`; `set_arrays(scenes, polys, labels)` does the same from decoded scenes.  `img_files` / `label_files` / `len()` are per
    ITEM ("<scene path>#x0,y0,c"), so the mosaic partner draws range over windows.

    overlap, rates: the window plan (scene_windows, window side = img_size / rate).  iof_thr: a label belongs to a window when that share
    of its area lies inside.  keep_empty=False: planned windows that keep no label are not items (one launch of ryolo_scene_label_rows over
    all scenes at construction, label files only — no pixels are decoded).  jitter (default: augment): every USE of an item, mosaic
    partners included, redraws the window origin (jitter_window) from random.Random(window_seed) — never from `rng`, whose draws stay in
    the reference's order.  `last_windows`: (item, scene, x0, y0, c) per row of the last batch's resize table.

    copy_paste (a CopyPaste or a dict of its arguments; default None: off): with augment, labelled objects of the scenes the batch reads
    are pasted onto the finished canvases and their labels appended behind the batch's rows (datasets/copy_paste.py); `last_pastes`:
    (slot, scene, label index, angle, scale, (cx, cy)) per pasted object of the last batch.  label_table() never pastes.

    ignore (an Ignore or a dict of its arguments; default None: off, not one launch more): per batch a SHADOW table of every label the host
    cull hands to a use goes through ryolo_scene_label_rows with the threshold iof_lo and through ryolo_label_stage with the batch's own
    matrices; a shadow row that is finite after the stage becomes an ignore row when its IoF is below iof_thr, or when `difficult` is on and
    its label is difficult (those labels are then left out of the targets on the host).  `last_ignore`: float32 [ni, 9] on the device =
    (slot, x1, y1, ..., x4, y4) with the flips of the slot applied and divided by the canvas side like the targets — the `ignore` argument
    of the criterion; [0, 9] without rows, None when the option is off; valid until the next batch is requested.  Two extra launches, six
    small uploads, a few element-wise torch operations and one host read (the row count) per batch.  The windows, every draw from `rng`,
    copy-paste (pastes neither bury ignore rows nor count them for occ_thr), keep_empty and label_table() are what they are without it.
    Not covered: rows that the centre filter of ryolo_encode_labels drops on the plain DOTADataset path, and ignore rows of a mixup
    partner beyond carrying its slot.

    rotate (a Rotate or a dict of its arguments; default None: off, not one draw or launch more; augment only): after the jitter draw every
    use draws a coin and, under p, an angle from Rotate's private generator; a rotated use is read from the scene through
    augment.rot_window_maps' pixel map (INTERP_ROT, the same row of the same table; about the window's centre pixel, 114 beyond the
    scene), and its labels are the scene's under the label map: the polygons the cull against the rotated window's bounding box keeps are
    mapped on the host in float64 and tested by ryolo_scene_label_rows against the window (0, 0, c) — in the main table and in the shadow
    table of `ignore` alike.  `last_angles`: degrees, or None for an unrotated use, per row of `last_windows`.  Unrotated uses, `rng`, the
    jitter generator, copy-paste, keep_empty and label_table() (planned, unrotated windows) are what they are without it.  Not built:
    keeping the rotated window inside the scene, keeping the p_object label inside the rotated window, area filtering for c > img_size
    (rotated cuts are bilinear, as load_image's resizes under augment are).  tests/scene_rotate_ref.py restates it."""

    def __init__(self, hyp, img_size, augment, csl, normalized_labels=False, overlap=200, rates=(1.0,), iof_thr=0.7, keep_empty=False,
                 jitter=None, p_object=0.5, window_seed=0, copy_paste=None, ignore=None, rotate=None, **device_kw):
        super().__init__(hyp, img_size, augment, csl, normalized_labels, **device_kw)
        if normalized_labels:
            raise ValueError("SceneDataset: scene labels are in scene pixels (normalized_labels=False)")
        if not (0.0 < float(iof_thr) <= 1.0):
            raise ValueError(f"SceneDataset: iof_thr must satisfy 0 < iof_thr <= 1, got {iof_thr}")
        if not (0.0 <= float(p_object) <= 1.0):
            raise ValueError(f"SceneDataset: p_object is a probability, got {p_object}")
        scene_windows(1, 1, img_size, overlap, rates)               # argument errors now, not at the first scene
        self.ignore = check_ignore(ignore, iof_thr)
        self.rotate = check_rotate(rotate, augment)
        self.last_ignore = self._ignore_pending = None
        self._shadow = {}                                          # resize-table row -> (polys, classes, difficult flags) the cull handed to that use
        self.overlap, self.rates, self.iof_thr, self.keep_empty = overlap, tuple(rates), float(iof_thr), bool(keep_empty)
        self.jitter = bool(augment) if jitter is None else bool(jitter)
        self.p_object = float(p_object)
        self._wrng = _py_random.Random(window_seed)
        self.scene_files, self.scene_label_files = [], []
        self.items = []                                            # (scene, rate index, x0, y0, c)
        self.last_windows, self._row_wins = [], []
        self.last_angles, self._maps = [], {}                      # degrees or None per resize-table row; row -> (minv, fwd) of a rotated use
        self._rotating = True                                      # (off while label_table() reads the planned windows)
        self._boxes = {}                                           # scene -> label_boxes of its labels (the cull of every use)
        self._difficult = {}                                       # scene -> uint8 [n] "difficult" flags (scene_difficult)
        if copy_paste is not None and not isinstance(copy_paste, CopyPaste):
            copy_paste = CopyPaste(**dict(copy_paste))
        self.copy_paste = copy_paste
        self.last_pastes = []
        self._paste_sources = {}                                   # scene -> indices of its labels that can be pasted
        self._class_counts = None                                  # class -> label count over all scenes

    # ------------------------------------------------------------------ the item table
    def _pool_files(self):
        return self.scene_files, self.scene_label_files

    def scene_labels(self, scene):
        """(polys float32 [n, 8] in scene pixels, classes float32 [n]) of a scene, parsed on first use."""
        got = self._labels.get(scene)
        if got is None:
            got = self._labels[scene] = self._parse_label_file(self.scene_label_files[scene])
        return got

    def scene_difficult(self, scene):
        """uint8 [n] aligned with scene_labels(scene): nonzero marks a label the DOTA / VOC protocol calls difficult (lib/dota_eval.py).
        Here: the flags given to set_arrays, else zeros; a dataset that reads them from its label files overrides _parse_difficult."""
        got = self._difficult.get(scene)
        if got is None:
            n = len(self.scene_labels(scene)[1])
            got = self._parse_difficult(scene)
            got = np.zeros(n, dtype=np.uint8) if got is None else (np.asarray(got).reshape(-1) != 0).astype(np.uint8)
            if len(got) != n:
                raise ValueError(f"SceneDataset: {len(got)} difficult flags for the {n} labels of scene {scene}")
            self._difficult[scene] = got
        return got

    def _parse_difficult(self, scene):
        return None

    def _window_cull(self, scene, x0, y0, c):
        polys, _ = self.scene_labels(scene)
        boxes = self._boxes.get(scene)
        if boxes is None:
            boxes = self._boxes[scene] = label_boxes(polys)
        return cull_labels(polys, x0, y0, c, boxes)

    def _window_labels(self, scene, x0, y0, c):
        polys, cls = self.scene_labels(scene)
        keep = self._window_cull(scene, x0, y0, c)
        return polys[keep], cls[keep]

    def plan_windows(self):
        """(Re)build the item table from the scenes: every planned window, minus — without keep_empty — those that keep no label."""
        pool = self.cache()
        items = []
        for s in range(len(self.scene_files)):
            H, W = pool.shapes[s]
            items += [(s, ri, x0, y0, c) for ri, x0, y0, c in scene_windows(H, W, self.img_size, self.overlap, self.rates)]
        if not self.keep_empty and items:
            kept = self._windows_with_labels(items)
            items = [it for it, k in zip(items, kept) if k]
        self._set_items(items)
        return self

    def _windows_with_labels(self, items):
        rows, win_of_row = [], []
        for wi, (s, _, x0, y0, c) in enumerate(items):
            polys, cls = self._window_labels(s, x0, y0, c)
            if len(cls):
                r = np.zeros(len(cls), dtype=A.LABEL_ROW_DTYPE)
                r["poly"], r["cls"] = polys, cls
                rows.append(r)
                win_of_row.append(np.full(len(cls), wi, dtype=np.int32))
        kept = np.zeros(len(items), dtype=bool)
        if rows:
            rows, win_of_row = np.concatenate(rows), np.concatenate(win_of_row)
            table = A.upload_label_rows(rows, self.device)
            iof = A.scene_label_rows(table, len(rows), win_of_row, [(x0, y0, c) for _, _, x0, y0, c in items], self.iof_thr, want_iof=True)
            kept[win_of_row[iof.cpu().numpy() >= self.iof_thr]] = True      # (a zero-area label reports 0)
        return kept

    def _set_items(self, items):
        self.items = list(items)
        self.img_files = ["{}#{},{},{}".format(self.scene_files[s], x0, y0, c) for s, _, x0, y0, c in self.items]
        self.label_files = [self.scene_label_files[s] for s, _, _, _, _ in self.items]

    def set_arrays(self, images, polys, labels, difficult=None):
        """Decoded scenes (uint8 HWC BGR) and their parsed labels (scene pixels) instead of files; plans the windows.  difficult: per scene
        the flags scene_difficult returns (default: none is difficult)."""
        self.img_files, self.label_files = [], []
        super().set_arrays(images, polys, labels)
        self._difficult, self._paste_sources, self._class_counts = {}, {}, None
        if difficult is not None:
            difficult = list(difficult)
            if len(difficult) != len(self._labels):
                raise ValueError(f"SceneDataset.set_arrays: difficult flags for {len(difficult)} scenes, {len(self._labels)} scenes")
            for i, d in enumerate(difficult):
                d = (np.asarray(d).reshape(-1) != 0).astype(np.uint8)
                if len(d) != len(self._labels[i][1]):
                    raise ValueError(f"SceneDataset.set_arrays: {len(d)} difficult flags for the {len(self._labels[i][1])} labels of scene {i}")
                self._difficult[i] = d
        self.scene_files, self.scene_label_files = list(self.img_files), list(self.img_files)
        self.plan_windows()

    def shard(self, rank, world_size, pad=None):
        """BaseDataset.shard over the ITEM table (same padding rules); the pool keeps holding whole scenes, filled on demand."""
        self._set_items([self.items[i] for i in self._shard_indices(len(self.items), rank, world_size, self.augment if pad is None else pad)])
        return self

    # ------------------------------------------------------------------ the first stage of assemble_batch, through the window
    def _use_shape(self, index, row):
        s, _, x0, y0, c = self.items[index]
        if self.jitter:
            H, W = self._pool.shapes[s]
            x0, y0 = jitter_window(self._wrng, H, W, c, self.scene_labels(s)[0], self.p_object)
        if row != len(self.last_windows):
            raise RuntimeError("SceneDataset: resize table and window table out of step")
        self.last_windows.append((index, s, x0, y0, c))
        self.last_angles.append(self.rotate.draw() if self.rotate is not None and self._rotating else None)
        return c, c

    def _label_wins(self):
        """The windows ryolo_scene_label_rows tests the rows of each use against: (x0, y0, c), and (0, 0, c) for a rotated use, whose
        polygons the host has already mapped into the window frame."""
        return [(0, 0, w[4]) if a is not None else w[2:] for w, a in zip(self.last_windows, self.last_angles)]

    def _use_cull(self, row):
        """(indices the host cull keeps, their polygons, their classes) for the use `row`, in file order.  Unrotated: bounding boxes against
        the window, polygons in scene pixels.  Rotated: bounding boxes against the bounding box of the rotated window (a superset of what
        can have a share inside it), polygons mapped into the window frame by rot_window_maps' fwd in float64."""
        _, s, x0, y0, c = self.last_windows[row]
        polys, cls = self.scene_labels(s)
        if self.last_angles[row] is None:
            keep = self._window_cull(s, x0, y0, c)
            return keep, polys[keep], cls[keep]
        boxes = self._boxes.get(s)
        if boxes is None:
            boxes = self._boxes[s] = label_boxes(polys)
        xlo, xhi, ylo, yhi = rot_window_box(x0, y0, c, self.last_angles[row])
        keep = np.nonzero((boxes[1] > xlo - 1e-3) & (boxes[0] < xhi + 1e-3) & (boxes[3] > ylo - 1e-3) & (boxes[2] < yhi + 1e-3))[0]
        return keep, A.map_polys(polys[keep], self._use_maps(row)[1]), cls[keep]

    def _use_maps(self, row):
        got = self._maps.get(row)
        if got is None:
            _, _, x0, y0, c = self.last_windows[row]
            _, (n, _) = self._resized(c, c)
            got = self._maps[row] = A.rot_window_maps(x0, y0, c, n, self.last_angles[row])
        return got

    def _use_labels(self, index, row):
        s = self.last_windows[row][1]
        keep, polys, cls = self._use_cull(row)
        if self.ignore is not None:
            # the shadow of this use: everything the cull kept, difficult labels included; with Ignore.difficult those are no targets
            diff = self.scene_difficult(s)[keep]
            self._shadow[row] = (polys, cls, diff)
            if self.ignore.difficult:
                polys, cls = polys[diff == 0], cls[diff == 0]
        self._row_wins.append(np.full(len(cls), row, dtype=np.int32))
        return polys, cls

    def _pixel_stage(self, pool, items, luts):
        pool.ensure(w[1] for w in self.last_windows)
        table = [(s, (x0, y0, c), hw, interp, lut) for (_, s, x0, y0, c), (_, hw, interp, lut) in zip(self.last_windows, items)]
        for row, a in enumerate(self.last_angles):
            if a is not None:                                       # a rotated use: the same row of the same table, read through its map
                table[row] = table[row][:3] + (A.INTERP_ROT, table[row][4], self._use_maps(row)[0])
        return A.resize_hsv_windows(pool, table, luts)

    def _label_table(self, rows):
        table = super()._label_table(rows)
        A.scene_label_rows(table, len(rows), np.concatenate(self._row_wins), self._label_wins(), self.iof_thr)
        return table

    def assemble_batch(self, indices):
        self.last_windows, self._row_wins, self._shadow = [], [], {}
        self.last_angles, self._maps = [], {}
        self.last_ignore = self._ignore_pending = None
        batch = super().assemble_batch(indices)
        if self._ignore_pending is not None:
            # the rows were chosen on the device in _label_side_stage; the compaction needs their count on the host, and here — behind
            # finalize_batch's own read — that wait is over work that has already finished
            out, sel = self._ignore_pending
            self.last_ignore, self._ignore_pending = out[sel], None
        return batch

    def _label_side_stage(self, uses, mats, flags):
        """The ignore rows of the batch (class docstring; restated by tests/ignore_ref.py): the shadow table through the window test at iof_lo
        and the stage with the batch's matrices, the choice of rows, then the coordinate maps ryolo_encode_labels applies to labels — the
        division by the canvas side and the flips of the slot, the same fp32 operations."""
        ig = self.ignore
        if ig is None:
            return
        dev, S = self.device, self.img_size
        rows, wins, hard = [], [], []
        for row, slot, hw0, hw, u, mat in uses:
            polys, cls, diff = self._shadow[row]
            rows.append(A.label_rows(polys, cls, slot, hw0, hw, u, mat, self.normalized_labels))
            wins.append(np.full(len(cls), row, dtype=np.int32))
            hard.append(diff)
        rows = np.concatenate(rows) if rows else np.zeros(0, dtype=A.LABEL_ROW_DTYPE)
        n = len(rows)
        if not n:
            self.last_ignore = torch.empty((0, 9), dtype=torch.float32, device=dev)
            return
        table = A.upload_label_rows(rows, dev)
        iof = A.scene_label_rows(table, n, np.concatenate(wins), self._label_wins(), ig.iof_lo, want_iof=True)
        t10 = A.label_stage_table(table, n, mats, dev)              # (slot, class, 8 vertices in canvas pixels; NaN: below iof_lo or filtered)
        quad = t10[:, 2:10]
        sel = iof < self.iof_thr
        if ig.difficult:
            sel = sel | (A._to_device(np.concatenate(hard).astype(np.uint8), dev) != 0)
        sel = sel & torch.isfinite(quad).all(dim=1)
        f = A._to_device(np.asarray(flags, dtype=np.uint8), dev)[t10[:, 0].long()]
        x, y = quad[:, 0::2] / float(S), quad[:, 1::2] / float(S)
        x = torch.where((f & 1).bool()[:, None], 1.0 - x, x)
        y = torch.where((f & 2).bool()[:, None], 1.0 - y, y)
        out = torch.empty((n, 9), dtype=torch.float32, device=dev)
        out[:, 0], out[:, 1::2], out[:, 2::2] = t10[:, 0], x, y
        self._ignore_pending = (out, sel)                            # (compacted at the end of assemble_batch)

    # ------------------------------------------------------------------ copy-paste on the finished canvases
    def class_counts(self):
        """{class: number of labels over ALL scenes}, from the label files, once."""
        if self._class_counts is None:
            counts = {}
            for s in range(len(self.scene_files)):
                for c in self.scene_labels(s)[1].tolist():
                    counts[c] = counts.get(c, 0) + 1
            self._class_counts = counts
        return self._class_counts

    def paste_bank(self, scenes):
        """{class: [(scene, label index, quad)]} over `scenes` ascending, labels in file order, strictly convex finite quads only."""
        bank = {}
        for s in sorted(set(int(v) for v in scenes)):
            polys, cls = self.scene_labels(s)
            src = self._paste_sources.get(s)
            if src is None:
                src = self._paste_sources[s] = [i for i in range(len(cls)) if strictly_convex(polys[i])]
            for i in src:
                bank.setdefault(float(cls[i]), []).append((s, i, polys[i]))
        return bank

    def _canvas_stage(self, final, targets10, indices):
        self.last_pastes = []
        cp = self.copy_paste
        if cp is None or not self.augment:
            return final, targets10
        S = self.img_size
        drawn = cp.draw(len(indices), S, self.paste_bank(w[1] for w in self.last_windows), self.class_counts(),
                        [S / self.items[i][4] for i in indices])
        self.last_pastes = [(slot, scene, label, angle, sc, (cx, cy)) for slot, scene, label, _, _, angle, sc, cx, cy in drawn]
        if not drawn:
            return final, targets10
        final, targets10, _ = A.paste_objects(self._pool, final, targets10, cp.items(drawn, self._pool), cp.occ_thr)
        return final, targets10

    def _label_chunk(self, indices):
        """BaseDataset._label_chunk over the PLANNED windows: jitter is off for its duration (the window generator is not touched) and the
        window tables of the last batch are put back afterwards."""
        saved = self.jitter, self.last_windows, self._row_wins, self.ignore, self.last_angles, self._maps, self._rotating
        self.jitter, self.last_windows, self._row_wins, self.ignore = False, [], [], None       # (the table holds every target: no ignore rows here)
        self.last_angles, self._maps, self._rotating = [], {}, False                            # (nor a rotated use: no angle is drawn)
        try:
            return super()._label_chunk(indices)
        finally:
            self.jitter, self.last_windows, self._row_wins, self.ignore, self.last_angles, self._maps, self._rotating = saved


class DOTASceneDataset(SceneDataset):
    """Full-size DOTA scenes in DOTADataset's layout: `images/*.png` with `annfiles/*.txt` (datasets/DOTA_dataset.py)."""

    def __init__(self, data_dir, class_names, hyp, augment, img_size, csl, normalized_labels=False, **kw):
        super().__init__(hyp, img_size, augment, csl, normalized_labels, **kw)
        self.scene_files = sorted(glob.glob(os.path.join(data_dir, "images", "*.png")))
        self.scene_label_files = [p.replace("images", "annfiles").replace(".png", ".txt") for p in self.scene_files]
        self.category = {name.replace(" ", "-"): i for i, name in enumerate(class_names)}
        self.plan_windows()

    load_files = DOTADataset.load_files

    def _parse_difficult(self, scene):
        """Field 9 of every label line (the field after the category name): nonzero means difficult, an absent field 0."""
        with open(self.scene_label_files[scene].rstrip(), "r") as fh:
            fields = [line.split(" ") for line in fh.readlines()]
        return np.array([1 if len(f) > 9 and f[9].strip() and float(f[9]) != 0 else 0 for f in fields], dtype=np.uint8)
