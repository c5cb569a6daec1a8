"""CPU tests of training on full-size scenes (datasets/scene_dataset.py): the window plan, the label rule (shift, intersection over
foreground by Sutherland-Hodgman in fp64, keep) as tests/scene_ref.py restates it — by hand and against exact rational arithmetic —
and the jitter draws.  The device kernels are compared with the same restatement bit for bit in tests/test_gpu_scene.py.

test_iof_hand_cases and test_iof_fp64_against_exact_rationals run tests/scene_ref.py ALONE, no product code: they pin the restatement
(by hand, and against fractions.Fraction on this file's own lattice set, `_lattice_rects(20000, seed 5)`: max deviation 3.1e-15) that
the kernel is then held to bit for bit.  They are no coverage of the kernel's intersection over foreground; that is
tests/test_gpu_scene.py::test_label_rows_equal_the_restatement_bit_for_bit alone."""
import random
from fractions import Fraction

import numpy as np
import pytest

from tests import scene_ref as R


# ---------------------------------------------------------------------------------------------- 1. window plan
@pytest.mark.parametrize("H,W,size,overlap", [(100, 70, 32, 8), (4000, 4000, 800, 200), (64, 64, 64, 0), (65, 200, 64, 63), (31, 500, 96, 20)])
def test_window_plan_equals_tile_plan_at_rate_one(H, W, size, overlap):
    from ryolov4_amd.datasets.scene_dataset import scene_windows
    from ryolov4_amd.lib import tiled
    got = scene_windows(H, W, size, overlap)
    assert got == [(ri, x0, y0, size) for ri, x0, y0 in tiled.tile_plan(H, W, size, overlap)]
    assert got == R.scene_windows(H, W, size, overlap)


def test_window_plan_rates_by_hand():
    from ryolov4_amd.datasets.scene_dataset import scene_windows
    # 100 (H) x 70 (W), size 32, overlap 8.  rate 0.5: c = 64, stride 64 - 16 = 48: x: 70 > 64 -> 0, then 0 + 64 < 70 so 48 is not reached:
    # starts 0, 70 - 64 = 6; y: 0, 48 (48 + 64 >= 100) -> 0, 36.
    assert scene_windows(100, 70, 32, 8, (0.5,)) == [(0, 0, 0, 64), (0, 6, 0, 64), (0, 0, 36, 64), (0, 6, 36, 64)]
    # rate 2.0: c = 16, stride 16 - 4 = 12: x: 0, 12, ..., 48 (48 + 16 = 64 < 70), 60 + 16 >= 70 -> 54; y: 0 .. 72 (72 + 16 < 100), then 84
    xs, ys = [0, 12, 24, 36, 48, 54], [0, 12, 24, 36, 48, 60, 72, 84]
    assert scene_windows(100, 70, 32, 8, (2.0,)) == [(0, x, y, 16) for y in ys for x in xs]
    both = scene_windows(100, 70, 32, 8, (2.0, 0.5))
    assert both == [(0, x, y, 16) for y in ys for x in xs] + [(1, 0, 0, 64), (1, 6, 0, 64), (1, 0, 36, 64), (1, 6, 36, 64)]
    assert both == R.scene_windows(100, 70, 32, 8, (2.0, 0.5))
    # a scene smaller than the window: one window hanging over it
    assert scene_windows(40, 40, 64, 16, (1.0, 0.5)) == [(0, 0, 0, 64), (1, 0, 0, 128)]
    # rounding of the side: int(size / r + 0.5)
    assert scene_windows(10, 10, 32, 0, (1.5,))[0][3] == 21 and scene_windows(10, 10, 32, 0, (0.3,))[0][3] == 107


@pytest.mark.parametrize("args", [(100, 70, 33, 8), (100, 70, 0, 0), (100, 70, 32, 32), (100, 70, 32, -1), (100, 70, 32.0, 8), (100, 70, 32, 8, ()),
                                  (100, 70, 32, 8, (0.0,)), (100, 70, 32, 8, (float("nan"),)), (100, 70, 32, 8, (float("inf"),)), (0, 70, 32, 8),
                                  (100, 70, 32, 31, (40.0,))])
def test_window_plan_argument_errors(args):
    from ryolov4_amd.datasets.scene_dataset import scene_windows
    with pytest.raises(ValueError):
        scene_windows(*args)


# ---------------------------------------------------------------------------------------------- 2. IoF by hand
def _bits(v):
    return np.float64(v).tobytes()


def test_iof_hand_cases():
    c = 64
    sq = [(10.0, 10.0), (20.0, 10.0), (20.0, 20.0), (10.0, 20.0)]
    assert R.iof_quad(sq, c) == (1.0, 4)                                             # fully inside: exactly 1
    half = [(-10.0, 10.0), (10.0, 10.0), (10.0, 20.0), (-10.0, 20.0)]
    assert R.iof_quad(half, c) == (0.5, 4)                                           # half: exactly 0.5
    out = [(100.0, 100.0), (120.0, 100.0), (120.0, 130.0), (100.0, 130.0)]
    assert R.iof_quad(out, c)[0] == 0.0
    touching = [(64.0, 10.0), (80.0, 10.0), (80.0, 20.0), (64.0, 20.0)]             # shares the edge x = c only: no area inside
    assert R.iof_quad(touching, c)[0] == 0.0
    rot = [(-7.25, 30.5), (16.75, 12.5), (28.75, 28.5), (4.75, 46.5)]               # a (4, 3)-direction rectangle over the left border
    a, b = R.iof_quad(rot, c), R.iof_quad(rot[::-1], c)
    assert 0.0 < a[0] < 1.0 and _bits(a[0]) == _bits(b[0]) and a[1] == b[1]          # CW and CCW: same bits
    assert abs(a[0] - float(R.iof_quad(rot, c, Fraction)[0])) <= 1e-15
    for flat in ([(1.0, 1.0), (2.0, 2.0), (3.0, 3.0), (4.0, 4.0)], [(5.0, 5.0)] * 4, [(0.0, 0.0), (4.0, 0.0), (8.0, 0.0), (4.0, 0.0)]):
        assert R.iof_quad(flat, c) == (None, 0)                                      # zero area: dropped
    diamond = [(0.0, 10.0), (10.0, 0.0), (20.0, 10.0), (10.0, 20.0)]                # vertices ON x = 0 and y = 0: inside, nothing clipped
    assert R.iof_quad(diamond, c) == (1.0, 4)
    corner = [(-8.0, -8.0), (8.0, -8.0), (8.0, 8.0), (-8.0, 8.0)]                   # a quarter, through the window's corner
    assert R.iof_quad(corner, c) == (0.25, 4)
    big = [(32.0, -8.0), (72.0, 32.0), (32.0, 72.0), (-8.0, 32.0)]                  # every tip cut off: an octagon
    v, n = R.iof_quad(big, c)
    assert n == 8 and v == float(Fraction(3200 - 4 * 64, 3200)) == 0.92
    cover = [(-100.0, -100.0), (200.0, -100.0), (200.0, 200.0), (-100.0, 200.0)]     # the window inside the quad
    assert R.iof_quad(cover, c) == (64.0 * 64.0 / 90000.0, 4)


def test_label_rows_shift_keep_and_cull():
    polys = np.array([[110, 210, 120, 210, 120, 220, 110, 220],        # inside the window (100, 200, 64)
                      [90, 210, 110, 210, 110, 220, 90, 220],          # half
                      [95, 210, 125, 210, 125, 220, 95, 220],          # 5 of 30 outside: 0.8333
                      [300, 300, 310, 300, 310, 310, 300, 310],        # elsewhere: culled
                      [164, 210, 170, 210, 170, 220, 164, 220],        # touches x = x0 + c: culled (no positive overlap)
                      [130, 230, 130, 230, 130, 230, 130, 230]], dtype=np.float32)   # no area: dropped
    cls = np.arange(6, dtype=np.float32)
    assert R.cull(polys, 100, 200, 64).tolist() == [0, 1, 2, 5]        # (the label without area lies in the window: the kernel drops it)
    sh, iof, keep = R.label_rows(polys, 100, 200, 64, 0.7)
    assert sh.dtype == np.float32 and np.array_equal(sh[0], np.float32([10, 10, 20, 10, 20, 20, 10, 20]))
    assert iof[0] == 1.0 and iof[1] == 0.5 and abs(iof[2] - 25 / 30) < 1e-15 and iof[3] == 0.0 and iof[5] == 0.0
    assert keep.tolist() == [True, False, True, False, False, False]
    p, k = R.window_labels(polys, cls, 100, 200, 64, 0.7)
    assert k.tolist() == [0.0, 2.0] and np.array_equal(p, sh[[0, 2]])                # unclipped, file order
    from ryolov4_amd.datasets.scene_dataset import cull_labels
    for win in ((100, 200, 64), (0, 0, 64), (-30, 190, 128), (290, 290, 16)):
        assert np.array_equal(cull_labels(polys, *win), R.cull(polys, *win))


# ---------------------------------------------------------------------------------------------- 3. IoF against exact rationals
def _lattice_rects(n, seed):
    """Rotated rectangles on the 1/8-pixel lattice: edges k (a, b) / 8 and m (-b, a) / 8 with (a, b) a Pythagorean direction, 4-60 px long,
    around a 64 px window; either orientation.  Every coordinate is exact in fp32."""
    rs = random.Random(seed)
    dirs = [(3, 4, 5), (4, 3, 5), (5, 12, 13), (12, 5, 13), (8, 15, 17), (15, 8, 17), (-3, 4, 5), (-12, 5, 13), (1, 0, 1), (0, 1, 1), (7, 24, 25)]
    out = []
    for _ in range(n):
        a, b, h = rs.choice(dirs)
        k, m = rs.randint(-(-32 // h), 480 // h), rs.randint(-(-32 // h), 480 // h)
        x, y = rs.randint(-40 * 8, 100 * 8), rs.randint(-40 * 8, 100 * 8)
        q = [(x, y), (x + k * a, y + k * b), (x + k * a - m * b, y + k * b + m * a), (x - m * b, y + m * a)]
        if rs.random() < 0.5:
            q.reverse()
        out.append([(Fraction(px, 8), Fraction(py, 8)) for px, py in q])
    return out


def test_iof_fp64_against_exact_rationals():
    """fp64 Sutherland-Hodgman against fractions.Fraction on 20 000 lattice rectangles: |fp64 - exact| <= 1e-12, the kept sets agree
    except where the exact ratio is within 1e-12 of the threshold, and those are at most 0.5 % of the cases."""
    thr, c = 0.7, 64
    cases = _lattice_rects(20000, 5)
    worst, near, maxv, partial = 0.0, 0, 0, 0
    for q in cases:
        exact, _ = R.iof_quad(q, c, Fraction)
        got, nv = R.iof_quad([(float(x), float(y)) for x, y in q], c)
        assert exact is not None and got is not None
        worst = max(worst, abs(got - float(exact)), float(abs(Fraction(got) - exact)))
        maxv = max(maxv, nv)
        partial += 0 < exact < 1
        if abs(exact - Fraction(thr)) <= Fraction(1, 10 ** 12):
            near += 1
        else:
            assert (got >= thr) == (exact >= Fraction(thr)), (q, got, exact)
    print(f"max |fp64 - exact| = {worst:.3g}, max clip vertices = {maxv}, at the threshold = {near}, partly inside = {partial}")
    assert worst <= 1e-12
    assert maxv <= 8
    assert near <= len(cases) * 0.005
    assert partial > len(cases) // 5                                  # the set does exercise the clip


# ---------------------------------------------------------------------------------------------- 4. jitter
def test_jitter_ranges_negative_origins_and_object_constraint():
    from ryolov4_amd.datasets.scene_dataset import jitter_window
    polys = np.float32([[10, 10, 20, 10, 20, 20, 10, 20], [180.5, 90.25, 190.5, 90.25, 190.5, 99.25, 180.5, 99.25]])
    a, b = random.Random(3), random.Random(3)
    seen = set()
    for _ in range(400):                                                # no label constraint: the whole range, scene larger than the window
        x0, y0 = jitter_window(a, 120, 200, 64, polys, 0.0)
        assert (x0, y0) == R.jitter_window(b, 120, 200, 64, polys, 0.0)
        assert 0 <= x0 <= 200 - 64 and 0 <= y0 <= 120 - 64
        seen.add((x0 == 0, x0 == 136, y0 == 0, y0 == 56))
    assert a.random() == b.random()                                     # the same number of draws
    for _ in range(400):                                                # a scene smaller than the window floats inside it
        x0, y0 = jitter_window(a, 40, 50, 64, polys[:0], 0.5)
        assert (x0, y0) == R.jitter_window(b, 40, 50, 64, polys[:0], 0.5)
        assert 50 - 64 <= x0 <= 0 and 40 - 64 <= y0 <= 0
        seen.add(("neg", x0 < 0, y0 < 0))
    assert ("neg", True, True) in seen
    hits = [0, 0]
    for _ in range(400):                                                # p_object = 1: the drawn label's mean vertex lies in the window
        x0, y0 = jitter_window(a, 120, 200, 64, polys, 1.0)
        assert (x0, y0) == R.jitter_window(b, 120, 200, 64, polys, 1.0)
        assert 0 <= x0 <= 136 and 0 <= y0 <= 56
        inside = [x0 <= mx < x0 + 64 and y0 <= my < y0 + 64 for mx, my in ((15.0, 15.0), (185.5, 94.75))]
        assert any(inside)
        hits[0] += inside[0]
        hits[1] += inside[1]
    assert min(hits) > 100
    # mixed axes: in a 40 (H) x 200 (W) scene the y range is [-24, 0] whatever the label says, and the x range follows the label
    for _ in range(100):
        x0, y0 = jitter_window(a, 40, 200, 64, polys[1:], 1.0)
        assert (x0, y0) == R.jitter_window(b, 40, 200, 64, polys[1:], 1.0)
        assert 186 - 64 + 1 <= x0 <= 136 and -24 <= y0 <= 0
    assert a.random() == b.random()


class _CountingRng:
    """random / numpy.random stand-in that counts every attribute access: the scene hooks must not touch `rng`."""

    def __init__(self):
        self.calls = 0

    def __getattr__(self, name):
        self.calls += 1
        raise AssertionError(f"rng.{name} used by the window draws")


def _cpu_dataset(**kw):
    from ryolov4_amd.datasets.scene_dataset import SceneDataset
    rs = np.random.RandomState(1)
    scenes = [rs.randint(0, 256, size=s + (3,)).astype(np.uint8) for s in ((97, 131), (40, 40), (211, 53))]
    polys = [(rs.rand(5, 1, 2) * [im.shape[1], im.shape[0]] + (rs.rand(5, 4, 2) - 0.5) * 12).reshape(5, 8).astype(np.float32) for im in scenes]
    labels = [rs.randint(0, 3, size=5).astype(np.float32) for _ in scenes]
    stub = _CountingRng()
    ds = SceneDataset({}, 64, True, False, device="cpu", keep_empty=True, rng=(stub, stub), **kw)
    ds.set_arrays(scenes, polys, labels)
    return ds, scenes, polys, stub


def test_items_paths_and_shards_are_per_window():
    ds, scenes, _, _ = _cpu_dataset(overlap=16, rates=(1.0, 0.5))
    want = [(s, ri, x0, y0, c) for s, im in enumerate(scenes) for ri, x0, y0, c in R.scene_windows(im.shape[0], im.shape[1], 64, 16, (1.0, 0.5))]
    assert ds.items == want and len(ds) == len(want) == len(ds.img_files) == len(ds.label_files)
    assert ds.img_files[1] == "<array 0>#48,0,64" and ds.img_files[-1] == "<array 2>#0,83,128"
    n = len(want)
    from ryolov4_amd.datasets.scene_dataset import SceneDataset
    from ryolov4_amd.datasets.base_dataset import BaseDataset
    for pad in (True, False):
        for rank in range(3):
            d2, _, _, _ = _cpu_dataset(overlap=16, rates=(1.0, 0.5))
            d2.shard(rank, 3, pad=pad)
            assert d2.items == [want[i] for i in BaseDataset._shard_indices(n, rank, 3, pad)]
            assert len(d2) == (-(-n // 3) if pad else len(range(rank, n, 3))) and len(d2.img_files) == len(d2)
    assert issubclass(SceneDataset, BaseDataset)
    for bad in (dict(iof_thr=0.0), dict(iof_thr=1.5), dict(p_object=2.0), dict(overlap=64), dict(rates=())):
        with pytest.raises(ValueError):
            _cpu_dataset(**bad)


def test_jitter_draws_are_private_and_seeded():
    runs = []
    for seed in (7, 7, 8):
        ds, scenes, polys, stub = _cpu_dataset(overlap=16, jitter=True, p_object=0.5, window_seed=seed)
        ref = random.Random(seed)
        order = [3, 0, 5, 5, 1, len(ds) - 1, 2, 3]
        for row, item in enumerate(order):
            assert ds._use_shape(item, row) == (64, 64)
            s = ds.items[item][0]
            x0, y0 = R.jitter_window(ref, scenes[s].shape[0], scenes[s].shape[1], 64, polys[s], 0.5)
            assert ds.last_windows[row] == (item, s, x0, y0, 64)
        assert stub.calls == 0                                          # self.rng is not consumed
        runs.append(list(ds.last_windows))
    assert runs[0] == runs[1] != runs[2]
    ds, _, _, stub = _cpu_dataset(overlap=16, jitter=False)
    for row, item in enumerate([2, 2, 0]):
        ds._use_shape(item, row)
        assert ds.last_windows[row] == (item,) + tuple(np.take(ds.items[item], [0, 2, 3, 4]))
    assert stub.calls == 0
    assert _cpu_dataset(overlap=16)[0].jitter is True                             # default: augment
