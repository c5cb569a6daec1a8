"""Rotated window cuts without a device: the maps of datasets/augment.py against tests/scene_rotate_ref.py, right angles as exact pixel
permutations, the direction guard (pixels and labels turn the same way), the Rotate draws, and the decision gaps of the cases
tests/test_gpu_scene_rotate.py compares on the device."""
import random

import numpy as np
import pytest

from tests import scene_ref as SR
from tests import scene_rotate_cases as K
from tests import scene_rotate_ref as RR

ANGLES = (0.0, 90.0, 180.0, 270.0, 17.3, 45.0, -133.0)


# ---------------------------------------------------------------------------------------------- maps
def test_maps_equal_the_restatement_and_invert_each_other():
    from ryolov4_amd.datasets import augment as A
    assert A.INTERP_ROT == RR.INTERP_ROT == 3
    for x0, y0, c, N in ((5, 9, 64, 64), (-20, 33, 45, 32), (100, -7, 128, 96), (0, 0, 96, 64), (7, 7, 32, 64)):
        for phi in ANGLES + (-90.0, 360.0, 1e-3):
            minv, fwd = A.rot_window_maps(x0, y0, c, N, phi)
            rm, rf = RR.maps(x0, y0, c, N, phi)
            assert minv.dtype == fwd.dtype == np.float64 and minv.tobytes() == rm.tobytes() and fwd.tobytes() == rf.tobytes()
            # fwd(minv(u, v)) is the window-frame position of result pixel (u, v): (u + 0.5) s - 0.5; back in result pixels: (u, v)
            u, v = np.meshgrid(np.arange(N, dtype=np.float64), np.arange(N, dtype=np.float64))
            px, py = RR.apply(fwd, *RR.apply(minv, u, v))
            s = c / N
            assert np.abs((px + 0.5) / s - 0.5 - u).max() < 1e-12 and np.abs((py + 0.5) / s - 0.5 - v).max() < 1e-12
    for x0, y0, c in ((5, 9, 64), (-20, 33, 45), (3, -8, 96)):
        minv, fwd = A.rot_window_maps(x0, y0, c, c, 0.0)
        assert minv.tolist() == [1.0, 0.0, float(x0), 0.0, 1.0, float(y0)]           # (-0.0 == 0.0)
        assert fwd.tolist() == [1.0, 0.0, float(-x0), 0.0, 1.0, float(-y0)]
        p = np.random.RandomState(c).uniform(-50, 300, (20, 8)).astype(np.float32)
        assert A.map_polys(p, fwd).tobytes() == SR.shift_poly(p, x0, y0).tobytes() == RR.map_polys(p, fwd).tobytes()
    for bad in ((0, 0, 0, 64, 10.0), (0, 0, 64, 0, 10.0), (0, 0, 64, 64, float("nan"))):
        with pytest.raises(ValueError):
            A.rot_window_maps(*bad)


def _positions(H, W, c):
    return [((W - c) // 2, (H - c) // 2), (-(c // 3), H // 3), (W - c // 2, H // 4), (W // 3, -(c // 3)), (W // 4, H - c // 2), (-5, -7),
            (W + 2 * c, 3), (W - 1 - c // 2, H - 1 - c // 2), (W - c, H - c)]


def test_right_angles_are_pixel_permutations():
    """c = N: the cut at 90 / 180 / 270 degrees is np.rot90 of the plain cut (fill included), at 0 degrees the plain cut itself."""
    from ryolov4_amd.datasets import augment as A
    scene = np.random.RandomState(2).randint(0, 256, (61, 83, 3)).astype(np.uint8)
    for c in (32, 45):
        for x0, y0 in _positions(61, 83, c):
            plain = SR.cut_window(scene, x0, y0, c)
            for quarter, phi in enumerate((0.0, 90.0, 180.0, 270.0)):
                minv, _ = A.rot_window_maps(x0, y0, c, c, phi)                       # (the maps the loader uploads)
                assert np.array_equal(RR.rot_cut(scene, minv, c), np.rot90(plain, quarter)), (c, x0, y0, phi)
            assert np.array_equal(RR.rot_cut(scene, RR.maps(x0, y0, c, c, -90.0)[0], c), np.rot90(plain, 3))
    assert (RR.rot_cut(scene, RR.maps(83 + 90, 3, 45, 45, 17.3)[0], 45) == RR.FILL).all()


# ---------------------------------------------------------------------------------------------- direction guard
def _inside(quad, x, y):
    q = np.asarray(quad, dtype=np.float64).reshape(4, 2)
    sg = 1.0 if SR.shoelace([tuple(p) for p in q]) > 0 else -1.0
    ok = np.ones(x.shape, dtype=bool)
    for k in range(4):
        a, b = q[k], q[(k + 1) % 4]
        ok &= sg * ((b[0] - a[0]) * (y - a[1]) - (b[1] - a[1]) * (x - a[0])) >= 0
    return ok


@pytest.mark.parametrize("phi", [17.3, 45.0, -133.0])
@pytest.mark.parametrize("c", [64, 96])
def test_pixels_and_labels_turn_the_same_way(phi, c):
    """A dark scene with one bright filled rotated rectangle, off the window's centre, and its label: the centroid of the bright pixels of the
    cut lies within 0.5 px of the mean of the mapped label scaled by N / c, and the map keeps the label's area."""
    from ryolov4_amd.datasets import augment as A
    N, H, W = 64, 200, 260
    x0, y0 = 70, 40
    quad = np.zeros(8, dtype=np.float32)
    cx, cy, w, h, a = x0 + 0.5 * c + 0.18 * c, y0 + 0.5 * c - 0.12 * c, 0.3 * c, 0.14 * c, 0.4
    ux, uy, vx, vy = np.cos(a) * w / 2, np.sin(a) * w / 2, -np.sin(a) * h / 2, np.cos(a) * h / 2
    quad[:] = [cx - ux - vx, cy - uy - vy, cx + ux - vx, cy + uy - vy, cx + ux + vx, cy + uy + vy, cx - ux + vx, cy - uy + vy]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    scene = np.full((H, W, 3), 10, dtype=np.uint8)
    scene[_inside(quad, xx, yy)] = 250
    minv, fwd = A.rot_window_maps(x0, y0, c, N, phi)                                   # (the maps the loader uses for pixels and labels)
    cut = RR.rot_cut(scene, minv, N)
    bright = cut[..., 0] > 130
    assert bright.sum() > 40 and not bright[0].any() and not bright[-1].any() and not bright[:, 0].any() and not bright[:, -1].any()
    v, u = np.nonzero(bright)
    q = quad.astype(np.float64)
    mx, my = RR.apply(fwd, q[0::2], q[1::2])
    want = np.array([mx.mean(), my.mean()]) * N / c
    mapped = A.map_polys(quad, fwd).astype(np.float64)[0]                              # (and what the loader hands to the label stage)
    assert np.abs(mapped[0::2] - mx).max() < 1e-4 and np.abs(mapped[1::2] - my).max() < 1e-4
    got = np.array([u.mean(), v.mean()])
    assert np.abs(got - want).max() <= 0.5, (got, want)
    # a rotation the other way would put the centroid elsewhere: the mirrored position is far outside the bound
    other = RR.apply(RR.maps(x0, y0, c, N, -phi)[1], q[0::2], q[1::2])
    assert np.abs(np.array([other[0].mean(), other[1].mean()]) * N / c - got).max() > 3.0
    area = abs(SR.shoelace(list(zip(q[0::2], q[1::2]))))
    assert abs(abs(SR.shoelace(list(zip(mx, my)))) - area) <= 1e-9 * area


# ---------------------------------------------------------------------------------------------- Rotate
def test_rotate_draws_step_seed_and_errors():
    from ryolov4_amd.datasets.scene_dataset import Rotate, SceneDataset, check_rotate
    r, ref = Rotate(degrees=30.0, p=0.5, step=0.0, seed=7), random.Random(7)
    got = [r.draw() for _ in range(200)]
    want = []
    for _ in range(200):
        want.append(ref.uniform(-30.0, 30.0) if ref.random() < 0.5 else None)       # the coin first, the angle only under p
    assert got == want and 60 < sum(a is None for a in got) < 140 and all(a is None or -30.0 <= a <= 30.0 for a in got)
    twin = RR.Draws(30.0, 0.5, 0.0, 7)
    assert got == [twin.draw() for _ in range(200)]
    s, ref = Rotate(degrees=180.0, p=1.0, step=15.0, seed=3), RR.Draws(180.0, 1.0, 15.0, 3)
    snapped = [s.draw() for _ in range(100)]
    assert snapped == [ref.draw() for _ in range(100)] and all(a == 15.0 * round(a / 15.0) and -180.0 <= a <= 180.0 for a in snapped)
    assert len(set(snapped)) > 10
    odd = Rotate(degrees=100.0, p=1.0, step=15.0, seed=1)                              # 100 is no multiple of 15: the snap stays inside
    got = [odd.draw() for _ in range(400)]
    assert set(got) == {15.0 * k for k in range(-6, 7)} and max(abs(a) for a in got) == 90.0
    assert Rotate(degrees=10.0, p=1.0, step=15.0).draw() == 0.0
    assert [Rotate(seed=1).draw() for _ in range(3)] != [Rotate(seed=2).draw() for _ in range(3)]
    assert all(Rotate(p=0.0).draw() is None for _ in range(20)) and Rotate(degrees=0.0, p=1.0).draw() == 0.0
    for bad in (dict(p=1.5), dict(p=-0.1), dict(degrees=-1.0), dict(step=-5.0), dict(degrees=float("nan")), dict(p=True)):
        with pytest.raises(ValueError):
            Rotate(**bad)
    with pytest.raises(ValueError):
        SceneDataset({}, 64, False, False, device="cpu", overlap=16, rotate=Rotate())               # an augmentation: not with augment=False
    with pytest.raises(ValueError):
        SceneDataset({}, 64, True, False, device="cpu", overlap=16, rotate=dict(angle=3))
    with pytest.raises(ValueError):
        SceneDataset({}, 64, True, False, device="cpu", overlap=16, rotate=45.0)
    ds = SceneDataset({}, 64, True, False, device="cpu", overlap=16, rotate=dict(degrees=20.0, p=0.25, step=5.0, seed=9))
    assert (ds.rotate.degrees, ds.rotate.p, ds.rotate.step, ds.rotate.seed) == (20.0, 0.25, 5.0, 9)
    assert SceneDataset({}, 64, True, False, device="cpu", overlap=16).rotate is None and check_rotate(None, False) is None
    used = Rotate(seed=5)
    used.draw()
    assert check_rotate(used, True).draw() == Rotate(seed=5).draw()                   # a dataset starts its own generator at the seed


class _CountingRng:
    def __init__(self):
        self.calls = 0

    def __getattr__(self, name):
        self.calls += 1
        raise AssertionError(f"rng.{name} used by the window draws")


def test_rotate_leaves_rng_and_the_jitter_generator_alone():
    """The uses of a batch with and without rotate: the same windows, the jitter generator in the same state, `rng` untouched; the
    angles are the restatement's draws in use order, one per resize-table row."""
    from ryolov4_amd.datasets.scene_dataset import SceneDataset
    imgs, polys, labels, _ = K.scenes()
    made = []
    for rot in (None, dict(K.ROT)):
        stub = _CountingRng()
        ds = SceneDataset({}, K.S, True, False, device="cpu", keep_empty=True, rng=(stub, stub), overlap=16, rates=(1.0, 2.0), window_seed=3, rotate=rot)
        ds.set_arrays(imgs, polys, labels)
        for row, item in enumerate([3, 0, 5, 5, 1, len(ds) - 1, 2, 3, 40, 41]):
            assert ds._use_shape(item, row) == (ds.items[item][4],) * 2
        assert stub.calls == 0
        made.append(ds)
    off, on = made
    assert off.last_windows == on.last_windows and off._wrng.getstate() == on._wrng.getstate()
    ref = RR.Draws(**K.ROT)
    assert off.last_angles == [None] * 10 and on.last_angles == [ref.draw() for _ in range(10)]
    assert any(a is None for a in on.last_angles) and any(a is not None for a in on.last_angles)
    assert on._label_wins() == [(0, 0, w[4]) if a is not None else w[2:] for w, a in zip(on.last_windows, on.last_angles)]


# ---------------------------------------------------------------------------------------------- decision gaps of the GPU cases
@pytest.mark.parametrize("name", sorted(K.DATASET_CASES))
def test_decision_gaps_of_the_gpu_cases(name):
    """Every intersection-over-foreground the restatement computes for the batches tests/test_gpu_scene_rotate.py assembles is at least
    1e-9 away from iof_thr and iof_lo (or exactly 0 or 1), so a last-bit difference cannot move a label across a threshold; and the
    batches hold rotated and unrotated uses, labels kept and dropped."""
    imgs, polys, labels, _ = K.scenes()
    wins, angles = K.plan(name)
    assert len(wins) == len(angles) >= len(K.DATASET_CASES[name][5]) and any(a is not None for a in angles)
    kept = dropped = 0
    for (_, s, x0, y0, c), a in zip(wins, angles):
        if a is None:
            _, iof, keep = SR.label_rows(polys[s], x0, y0, c, K.IOF_THR)
        else:
            N = K.S
            _, iof, keep = RR.label_rows(polys[s], RR.maps(x0, y0, c, N, a)[1], c, K.IOF_THR)
        for thr in (K.IOF_THR, K.IOF_LO):
            assert np.abs(iof - thr).min() >= 1e-9, (name, s, x0, y0, c, a)
        kept, dropped = kept + int(keep.sum()), dropped + int((~keep & (iof > 0)).sum())
    assert kept > 0 and dropped > 0
