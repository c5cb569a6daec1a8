"""Inputs of the ignore-region tests of the fused loss, shared by tests/test_gpu_loss_ignore.py (the kernels) and
tests/test_ignore_ref_cpu.py (which checks on the CPU that these quads leave no test vacuous).  Not a test module.

B = 2, nc = 3, grids (12, 6, 3).  kfiou (na 18): scale 0 is 2 * 18 * 144 = 5184 cells = exactly 81 full 64-cell runs of the objectness
pass; csl (na 3): 864 cells = 13 runs and a 32-cell tail; scale 2 of csl is one 54-cell tail.  Vertices are multiples of 1/8, so every
grid coordinate (coordinate * 12, * 6, * 3) is exact and some edges pass exactly through cell centres: x = 1/8 at gs 12 is 1.5, the
centre of column 1, which is inside."""
import numpy as np
import torch

from oracle import ref_ops
from ryolov4_amd.synth import CFG, synth_targets

B, NC, GS = 2, 3, (12, 6, 3)
NA = {"csl": 3, "kfiou": 18}
ATTRS = {"csl": NC + 185, "kfiou": NC + 6}
OCH = {"csl": 4, "kfiou": 5}
NAN = float("nan")

DIAMOND = [3 / 8, 4 / 8, 5 / 8, 2 / 8, 7 / 8, 4 / 8, 5 / 8, 6 / 8]           # a square turned by 45 degrees, centre (5/8, 4/8)


def _rect(x0, y0, x1, y1):
    return [x0, y0, x1, y0, x1, y1, x0, y1]


def _rev(q):
    return [v for k in (0, 3, 2, 1) for v in q[2 * k:2 * k + 2]]


# (what, image, quad)
QUADS = [
    ("axis-aligned, left edge through the centres of column 1 at gs 12", 0, _rect(1 / 8, 2 / 8, 4 / 8, 5 / 8)),
    ("45 degrees", 1, DIAMOND),
    ("45 degrees, the other vertex order", 0, _rev(DIAMOND)),
    ("overlapping pair, first", 0, _rect(4 / 8, 6 / 8, 6 / 8, 8 / 8)),
    ("overlapping pair, second", 0, _rect(5 / 8, 6 / 8, 7 / 8, 7 / 8)),
    ("the whole image", 1, _rect(0.0, 0.0, 1.0, 1.0)),
    ("wholly outside", 0, _rect(9 / 8, 1 / 8, 11 / 8, 3 / 8)),
    ("zero area", 0, [2 / 8, 1 / 8] * 4),
    ("a NaN coordinate", 0, [0.0, 0.0, 1.0, 0.0, 1.0, NAN, 0.0, 1.0]),
    ("image -1", -1, _rect(0.0, 0.0, 1.0, 1.0)),
    ("image B", B, _rect(0.0, 0.0, 1.0, 1.0)),
    # synth_targets(edge_cases=True) puts target 0 of image 0 at (0.5625, 0.3125): cell (gj 3, gi 6) of scale 0 and its neighbours
    ("over a target's own cell", 0, _rect(4 / 8, 2 / 8, 6 / 8, 4 / 8)),
]
DEAD = ("wholly outside", "zero area", "a NaN coordinate", "image -1", "image B")        # rows that must cover nothing


def ignore_table():
    return torch.tensor([[float(img)] + [float(v) for v in q] for _, img, q in QUADS], dtype=torch.float32)


class Model:
    def __init__(self, mode):
        self.anchors, self.nc = ref_ops.make_anchors(CFG, mode), NC


def targets(mode, empty=False):
    """A dozen rows (six per image) on a 96-pixel image, or none."""
    if empty:
        return torch.zeros((0, 187 if mode == "csl" else 7))
    return synth_targets(B, 6, NC, mode == "csl", seed=3, img_size=96, edge_cases=True)


def heads(mode, seed=11):
    """Random head maps [B, na, gs, gs, attrs], logits uniform in [-4, 4]."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, NA[mode], gs, gs, ATTRS[mode], generator=g) * 8.0 - 4.0) for gs in GS]


def cpu_matches(mode, tg):
    """Match records per scale as criterion.debug_matches() lays them out (columns b, a, gj, gi), from the oracle's build_targets on the CPU."""
    out = []
    for m in ref_ops.build_targets([(gs, gs) for gs in GS], tg, Model(mode).anchors, mode):
        rec = np.zeros((int(m["b"].numel()), 8), dtype=np.int64)
        for k, name in enumerate(("b", "a", "gj", "gi")):
            rec[:, k] = m[name].numpy()
        out.append(rec)
    return out
