"""Shared cases of the rotated-cut tests (tests/test_scene_rotate_cpu.py, tests/test_gpu_scene_rotate.py; not a test module): the scenes,
the dataset configurations, and a planner that runs the host half of a batch without a device, so that the CPU tests can check the very
windows and angles the GPU tests will see."""
import random

import numpy as np

S = 64
IOF_THR, IOF_LO = 0.7, 0.1
SCENE_SHAPES = ((97, 131), (150, 120))                               # H x W
PLAIN = dict(mosaic=0.0, mixup=0.0, hsv_h=0.0, hsv_s=0.0, hsv_v=0.0, rotate=0.0, scale=0.0, translate=0.0, fliplr=0.0, flipud=0.0)
FULL = dict(mosaic=1.0, mixup=0.5, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, rotate=10.0, scale=0.3, translate=0.1, fliplr=0.5, flipud=0.3)
ROT = dict(degrees=180.0, p=0.6, step=0.0, seed=4)
# name -> (hyp, rates, csl, Rotate arguments, ignore, batch indices)
DATASET_CASES = {
    "plain": (PLAIN, (1.0,), False, ROT, False, [0, 1, 2, 3, 4, 5, 1, 1]),
    "plain_rates": (PLAIN, (1.0, 2.0), False, dict(ROT, step=15.0), False, [0, 3, 7, 11, 20, 30, 40, 2]),
    "full_kfiou": (FULL, (1.0, 2.0), False, ROT, False, [0, 9, 25, 41]),
    "full_csl": (FULL, (1.0,), True, dict(ROT, p=1.0), False, [5, 2, 2]),
    "ignore": (PLAIN, (1.0, 2.0), False, dict(ROT, p=0.8), True, [0, 3, 7, 11, 20, 30, 40, 2]),
    "loss": (FULL, (1.0,), False, ROT, False, [0, 1, 2, 3]),
}


def rot_rects(rs, n, W, H, lo, hi, margin):
    """n rotated rectangles with sides lo .. hi px around an H x W scene, both orientations, float32 [n, 8]."""
    cx, cy = rs.uniform(-margin, W + margin, n), rs.uniform(-margin, H + margin, n)
    w, h, a = rs.uniform(lo, hi, n), rs.uniform(lo, hi, n), rs.uniform(0, np.pi, n)
    ux, uy = np.cos(a) * w / 2, np.sin(a) * w / 2
    vx, vy = -np.sin(a) * h / 2, np.cos(a) * h / 2
    q = np.stack([cx - ux - vx, cy - uy - vy, cx + ux - vx, cy + uy - vy, cx + ux + vx, cy + uy + vy, cx - ux + vx, cy - uy + vy], 1)
    flip = rs.rand(n) < 0.5
    q[flip] = q[flip].reshape(-1, 4, 2)[:, ::-1].reshape(-1, 8)
    return q.astype(np.float32)


def scenes():
    rs = np.random.RandomState(31)
    imgs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in SCENE_SHAPES]
    polys = [rot_rects(rs, 40, w, h, 4, 30, 5) for h, w in SCENE_SHAPES]
    labels = [rs.randint(0, 3, size=40).astype(np.float32) for _ in SCENE_SHAPES]
    difficult = [(rs.rand(40) < 0.2).astype(np.uint8) for _ in SCENE_SHAPES]
    return imgs, polys, labels, difficult


def dataset(name, device, base=None, rotate="case", seed=5):
    """The SceneDataset of a case (or a subclass `base` of it); rotate: "case" = the case's Rotate arguments, else what is given."""
    from ryolov4_amd.datasets.scene_dataset import Ignore, SceneDataset
    hyp, rates, csl, rot, ignore, _ = DATASET_CASES[name]
    imgs, polys, labels, difficult = scenes()
    ds = (base or SceneDataset)(hyp, S, True, csl, device=device, rng=(random.Random(seed), np.random.RandomState(seed)), overlap=16, rates=rates,
                                iof_thr=IOF_THR, keep_empty=True, window_seed=seed, rotate=rot if rotate == "case" else rotate,
                                ignore=Ignore(IOF_LO, True) if ignore else None)
    ds.set_arrays(imgs, polys, labels, difficult=difficult)
    return ds


class Planned(Exception):
    pass


def plan(name):
    """(last_windows, last_angles) of the case's batch, from the host half of assemble_batch alone (device "cpu", stopped at the pixel stage)."""
    from ryolov4_amd.datasets.scene_dataset import SceneDataset

    class Planner(SceneDataset):
        def _pixel_stage(self, pool, items, luts):
            raise Planned()

    ds = dataset(name, "cpu", Planner)
    try:
        ds.assemble_batch(DATASET_CASES[name][5])
    except Planned:
        pass
    return list(ds.last_windows), list(ds.last_angles)
