"""Object-level copy-paste for scene training: the host half (the draws and the item table); the device half is csrc/copypaste.hip.

Aerial data is class-imbalanced: a few classes carry most labels, others appear a few hundred times.  With the scenes of a batch already
resident in HBM next to the canvases being assembled, a labelled object can be taken out of a scene, rotated and scaled, dropped onto a
finished canvas with its label, and the labels it buries removed — three launches per batch (datasets/augment.py: paste_objects).

CopyPaste owns a private random.Random(seed): the assembler's `rng` is never touched, so the reference's draw order stands (the rule
SceneDataset's window_seed follows).  Per slot, in slot order, the draws are

    1. a coin: random() < p, else the slot gets nothing;
    2. n = randint(1, max_objects);
    3. per object  class   x = random() * sum(w), the first class (ascending) whose running sum of w exceeds x, w_c = n_c ** -alpha, among the
                           classes present in the batch's bank; n_c = the dataset-wide label count of the class;
                   object  randrange(len(bank[class]));
                   angle   uniform(-rotate, rotate) degrees;
                   scale   uniform(scale[0], scale[1]) * img_size / c, c the window side of the slot's item;
                   centre  cx = r + (S - 2 r) * random(), then cy likewise, r = scale * the largest distance of a vertex from the mean vertex.

An object is skipped AFTER its draws when 2 r > S or when its shortest scaled side is below min_side.  The bank holds the labels of the
scenes named in the batch's window table, scene ascending, label in file order, and only strictly convex finite quads (the four edge
cross products all of one non-zero sign: the test of ryolo_dota_match).  An empty bank draws nothing at all.

The map is M = T(centre) . scale . R(angle) . T(-mean vertex) with R = [[cos, sin], [-sin, cos]] (datasets/augment.py: affine); Minv is its
closed form; both in double on the host.  No reflection, so the vertex order ryolo_encode_labels expects is kept.

Whether copy-paste improves mAP on DOTA is NOT measured here (no real data or weights in this repository).  Not built: blending or
feathering of the paste edge, a context margin around the quad, hsv gains on the pasted pixels, sources from scenes outside the batch,
BaseDataset (non-scene) sources.  tests/copy_paste_ref.py restates the draws and the three kernels."""
import math
import random as _py_random

import numpy as np

from . import augment as A


def strictly_convex(quad):
    """Finite, and the four turns (e -> e + 1 -> e + 2) all of one non-zero sign — in double, as ryolo_dota_match decides it."""
    q = [float(v) for v in quad]
    if not all(math.isfinite(v) for v in q):
        return False
    x, y = q[0::2], q[1::2]
    cr = []
    for e in range(4):
        f, g = (e + 1) & 3, (e + 2) & 3
        cr.append((x[f] - x[e]) * (y[g] - y[f]) - (y[f] - y[e]) * (x[g] - x[f]))
    return all(c > 0 for c in cr) or all(c < 0 for c in cr)


def paste_matrices(quad, angle, scale, cx, cy):
    """(M, Minv) as 6 doubles each (row major 2 x 3): scene -> canvas and back, for a source quad whose mean vertex goes to (cx, cy)."""
    q = [float(v) for v in quad]
    mx = (q[0] + q[2] + q[4] + q[6]) / 4.0
    my = (q[1] + q[3] + q[5] + q[7]) / 4.0
    ang = angle * math.pi / 180.0
    a, b = scale * math.cos(ang), scale * math.sin(ang)
    ia, ib = a / (scale * scale), b / (scale * scale)
    M = (a, b, cx - a * mx - b * my, -b, a, cy + b * mx - a * my)
    Minv = (ia, -ib, mx - ia * cx + ib * cy, ib, ia, my - ib * cx - ia * cy)
    return M, Minv


def quad_extent(quad):
    """(largest distance of a vertex from the mean vertex, shortest side) of a quad, in double."""
    q = [float(v) for v in quad]
    mx = (q[0] + q[2] + q[4] + q[6]) / 4.0
    my = (q[1] + q[3] + q[5] + q[7]) / 4.0
    rad = max(math.hypot(q[2 * k] - mx, q[2 * k + 1] - my) for k in range(4))
    side = min(math.hypot(q[2 * ((k + 1) & 3)] - q[2 * k], q[2 * ((k + 1) & 3) + 1] - q[2 * k + 1]) for k in range(4))
    return rad, side


class CopyPaste:
    """p: chance that a slot receives pastes; max_objects: at most that many per slot; alpha: class weights n_c ** -alpha (0: uniform over
    classes, 1: inverse frequency); scale: range of the object scale (times img_size / window side); rotate: the angle is uniform in
    [-rotate, rotate) degrees; occ_thr: covered share at which a label is removed; min_side: scaled objects with a shorter side are not
    pasted; seed: of the private generator."""

    def __init__(self, p=0.5, max_objects=8, alpha=0.5, scale=(0.75, 1.25), rotate=180.0, occ_thr=0.5, min_side=4.0, seed=0):
        scale = tuple(float(v) for v in scale)
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError(f"CopyPaste: p is a probability, got {p}")
        if int(max_objects) < 1:
            raise ValueError(f"CopyPaste: max_objects must be >= 1, got {max_objects}")
        if len(scale) != 2 or not 0.0 < scale[0] <= scale[1] or not math.isfinite(scale[1]):
            raise ValueError(f"CopyPaste: scale must be a positive range (lo, hi), got {scale}")
        if not 0.0 < float(occ_thr) <= 1.0:
            raise ValueError(f"CopyPaste: occ_thr must satisfy 0 < occ_thr <= 1, got {occ_thr}")
        if not (float(rotate) >= 0.0 and float(min_side) >= 0.0 and math.isfinite(float(alpha))):
            raise ValueError("CopyPaste: rotate and min_side must be >= 0, alpha finite")
        self.p, self.max_objects, self.alpha, self.scale = float(p), int(max_objects), float(alpha), scale
        self.rotate, self.occ_thr, self.min_side = float(rotate), float(occ_thr), float(min_side)
        self.rng = _py_random.Random(seed)

    def draw_class(self, classes, counts):
        """One class among `classes` (ascending) with probability proportional to counts[c] ** -alpha: one random()."""
        w = [float(counts[c]) ** -self.alpha for c in classes]
        total = 0.0
        for v in w:
            total += v
        x = self.rng.random() * total
        acc = 0.0
        for c, v in zip(classes, w):
            acc += v
            if x < acc:
                return c
        return classes[-1]

    def draw(self, B, S, bank, counts, unit_scale):
        """bank {class: [(scene, label index, quad float32 [8])]}, counts {class: n_c}, unit_scale [B] (img_size / window side per slot) ->
        [(slot, scene, label index, class, quad, angle, scale, cx, cy)] of the objects that are pasted, slot by slot in paste order."""
        classes = sorted(c for c in bank if len(bank[c]))
        out = []
        if not classes:
            return out
        rng = self.rng
        for slot in range(B):
            if not rng.random() < self.p:
                continue
            for _ in range(rng.randint(1, self.max_objects)):
                c = self.draw_class(classes, counts)
                scene, label, quad = bank[c][rng.randrange(len(bank[c]))]
                angle = rng.uniform(-self.rotate, self.rotate)
                sc = rng.uniform(self.scale[0], self.scale[1]) * unit_scale[slot]
                rad, side = quad_extent(quad)
                r = sc * rad
                cx = r + (S - 2.0 * r) * rng.random()
                cy = r + (S - 2.0 * r) * rng.random()
                if 2.0 * r > S or sc * side < self.min_side:
                    continue
                out.append((slot, scene, label, c, quad, angle, sc, cx, cy))
        return out

    def items(self, drawn, pool):
        """The PASTE_ITEM_DTYPE table of draw()'s result; the scenes must be resident in `pool` (they are: the batch's windows read them)."""
        items = np.zeros(len(drawn), dtype=A.PASTE_ITEM_DTYPE)
        for k, (slot, scene, _, c, quad, angle, sc, cx, cy) in enumerate(drawn):
            H, W = pool.shapes[scene]
            M, Minv = paste_matrices(quad, angle, sc, cx, cy)
            items[k] = (pool.offsets[scene], H, W, slot, c, quad, M, Minv)
        return items
