"""GPU tests of rotated window cuts (INTERP_ROT of ryolo_resize_hsv_windows, SceneDataset(rotate=...)).

  table    A.resize_hsv_windows with rotated items bit for bit against tests/scene_rotate_ref.py (warp_perspective_numpy of the whole scene
           under the item's map, border 114, then the hsv restatement): two scenes (the second at an odd pool offset), result sides 32 / 64 /
           96, window sides N / 45 / 128, every one of seven angles at every one of nine window positions, with and without tables; single-item launches; a mixed table
           against the same table without its rotated items and against ryolo_warp_perspective_u8 + ryolo_hsv_gain_u8; the identity angle
           against the copy path;
  dataset  Rotate(degrees=0) and Rotate(p=0) against rotate=None; recorded windows and angles against a BaseDataset twin over host-made
           windows; ignore rows against tests/ignore_ref.py fed the mapped polygons; one batch through the criterion.
Network size 64 at the dataset level."""
import random
import types

import numpy as np
import pytest
import torch

from oracle import ref_data
from tests import ignore_ref as IR
from tests import scene_ref as SR
from tests import scene_rotate_cases as K
from tests import scene_rotate_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ANGLES = (0.0, 90.0, 180.0, 270.0, 17.3, 45.0, -133.0)
GAINS = [(1.01, 1.4, 0.7), (0.99, 0.5, 1.3), (1.0, 1.0, 1.0)]
SCENES = ((61, 83), (200, 260))


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _lut_pixels(img, lut):
    """cv2.LUT on the three hsv planes between the two restated conversions: what the tables of one item do to its pixels."""
    hsv = ref_data.bgr2hsv_numpy(img)
    return ref_data.hsv2bgr_numpy(np.stack((lut[0][hsv[..., 0]], lut[1][hsv[..., 1]], lut[2][hsv[..., 2]]), -1))


@pytest.fixture(scope="module")
def pool():
    """The two scenes in one buffer: the first at offset 0, the second at an offset that is no multiple of 4 (an ImagePool aligns to 16)."""
    rs = np.random.RandomState(17)
    imgs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in SCENES]
    off1 = ((imgs[0].size + 15) // 16) * 16 + 1
    raw = np.zeros(off1 + imgs[1].size + 16, dtype=np.uint8)
    raw[:imgs[0].size], raw[off1:off1 + imgs[1].size] = imgs[0].reshape(-1), imgs[1].reshape(-1)
    assert off1 % 4 == 1
    return types.SimpleNamespace(buf=torch.from_numpy(raw).to(DEV), offsets=[0, off1], shapes=list(SCENES), imgs=imgs)


def _positions(H, W, c):
    """interior; over the left, right, top, bottom border; negative origin; missing the scene; centred on the last pixel; ending at it."""
    return [((W - c) // 2, (H - c) // 2), (-(c // 3), H // 3), (W - c // 2, H // 4), (W // 3, -(c // 3)), (W // 4, H - c // 2), (-5, -7),
            (W + 2 * c, 3), (W - 1 - c // 2, H - 1 - c // 2), (W - c, H - c)]


def _grid(s):
    """[(window, N, angle, lut)] for scene s: per (N, c) every angle at every position (63 items), tables alternating."""
    H, W = SCENES[s]
    out = []
    for N in (32, 64, 96):
        for c in (N, 45, 128):
            pos = _positions(H, W, c)
            pairs = [(p, a) for p in pos for a in ANGLES]
            out += [((x0, y0, c), N, a, (len(out) + j) % 3 if (len(out) + j) % 2 else -1) for j, ((x0, y0), a) in enumerate(pairs)]
    return out


def _want(img, win, N, angle, lut, luts):
    cut = RR.rot_cut(img, RR.maps(win[0], win[1], win[2], N, angle)[0], N)
    return cut if lut < 0 else _lut_pixels(cut, luts[lut])


@pytest.mark.parametrize("s", [0, 1])
def test_rotated_items_equal_the_restatement(pool, s):
    from ryolov4_amd.datasets import augment as A
    luts = np.stack([A.hsv_luts(np.asarray(g, dtype=np.float64)) for g in GAINS])
    grid = _grid(s)
    assert len(grid) == 9 * 63 and {g[3] for g in grid} == {-1, 0, 1, 2}
    items = [(s, win, (N, N), A.INTERP_ROT, lut, A.rot_window_maps(win[0], win[1], win[2], N, a)[0]) for win, N, a, lut in grid]
    stage, offs = A.resize_hsv_windows(pool, items, luts)                              # every item in ONE launch
    got = stage.cpu().numpy()
    missed = 0
    for (win, N, a, lut), off in zip(grid, offs):
        mine = got[off:off + N * N * 3].reshape(N, N, 3)
        want = _want(pool.imgs[s], win, N, a, lut, luts)
        assert np.array_equal(mine, want), (s, win, N, a, lut, int((mine != want).sum()))
        if win[0] == SCENES[s][1] + 2 * win[2] and lut < 0:
            assert (mine == 114).all()                                                 # a window that misses the scene is the fill
            missed += 1
    assert missed >= 9 * 3                                                             # (every size, several angles each)
    # one launch with a single item: an interior one, one over a border, the one that ends at the scene's last pixel
    for k in (0, 8, 15, 100, 62, 500):
        one, o = A.resize_hsv_windows(pool, [items[k]], luts)
        N = grid[k][1]
        assert o == [0] and np.array_equal(one.cpu().numpy()[:N * N * 3], got[offs[k]:offs[k] + N * N * 3]), grid[k]


def test_odd_result_sizes_take_the_byte_stores(pool):
    """Result rows that are no multiple of 4 pixels (a thread's dwords would start off a dword in every other row) and narrower than a tile."""
    from ryolov4_amd.datasets import augment as A
    luts = np.stack([A.hsv_luts(np.asarray(GAINS[0], dtype=np.float64))])
    cases = [((10, 5, 37), 37, 17.3, -1), ((30, 20, 45), 67, -133.0, 0), ((-3, 40, 9), 9, 45.0, -1), ((0, 0, 1), 1, 0.0, 0), ((50, 9, 70), 66, 90.0, -1)]
    items = [(1, win, (N, N), A.INTERP_ROT, lut, A.rot_window_maps(win[0], win[1], win[2], N, a)[0]) for win, N, a, lut in cases]
    stage, offs = A.resize_hsv_windows(pool, items, luts)
    got = stage.cpu().numpy()
    for (win, N, a, lut), off in zip(cases, offs):
        assert np.array_equal(got[off:off + N * N * 3].reshape(N, N, 3), _want(pool.imgs[1], win, N, a, lut, luts)), (win, N, a)
    with pytest.raises(ValueError):
        A.resize_hsv_windows(pool, [(0, (0, 0, 64), (64, 64), A.INTERP_ROT, -1)])      # a rotated item without its map
    with pytest.raises(ValueError):
        A.resize_hsv_windows(pool, [(0, (0, 0, 64), (64, 64), A.INTERP_COPY, -1, np.zeros(6))])
    with pytest.raises(ValueError):
        A.resize_hsv_windows(pool, [(0, (0, 0, 64), (64, 64), A.INTERP_ROT, -1, np.full(6, np.nan))])


def test_mixed_table_and_the_existing_kernels(pool):
    """About 40 items of all four modes in one launch: the unrotated ones are what the table without the rotated ones gives, the rotated
    ones are ryolo_warp_perspective_u8 on the whole scene with the same map followed by ryolo_hsv_gain_u8."""
    from ryolov4_amd import hip
    from ryolov4_amd.datasets import augment as A
    luts = np.stack([A.hsv_luts(np.asarray(g, dtype=np.float64)) for g in GAINS])
    N = 64
    items = []
    for k in range(40):
        s = k % 2
        H, W = SCENES[s]
        x0, y0 = _positions(H, W, 64)[k % 9]
        lut = k % 3 if k % 4 else -1
        mode = (A.INTERP_ROT, A.INTERP_COPY, A.INTERP_LINEAR, A.INTERP_ROT, A.INTERP_AREA)[k % 5]
        c = 64 if mode == A.INTERP_COPY else (64, 45, 128)[k % 3]
        it = (s, (x0, y0, c), (N, N), mode, lut)
        items.append(it + (A.rot_window_maps(x0, y0, c, N, ANGLES[k % 7])[0],) if mode == A.INTERP_ROT else it)
    stage, offs = A.resize_hsv_windows(pool, items, luts)
    got = stage.cpu().numpy()
    plain = [it for it in items if it[3] != A.INTERP_ROT]
    pstage, poffs = A.resize_hsv_windows(pool, plain, luts)
    pgot = pstage.cpu().numpy()
    assert len(plain) == 24
    for it, po in zip(plain, poffs):
        off = offs[items.index(it)]
        assert np.array_equal(got[off:off + N * N * 3], pgot[po:po + N * N * 3]), it
    for it, off in zip(items, offs):
        if it[3] != A.INTERP_ROT:
            continue
        s = it[0]
        H, W = SCENES[s]
        scene = torch.from_numpy(pool.imgs[s]).to(DEV).contiguous()
        m9 = torch.tensor(list(it[5]) + [0.0, 0.0, 1.0], dtype=torch.float64, device=DEV)
        out = torch.empty((N, N, 3), dtype=torch.uint8, device=DEV)
        hip.call("ryolo_warp_perspective_u8", hip.ptr(scene), 1, H, W, hip.ptr(m9), hip.ptr(out), N, N, 114, hip.stream())
        if it[4] >= 0:
            lut = torch.from_numpy(luts[it[4]]).to(DEV).contiguous()
            hip.call("ryolo_hsv_gain_u8", hip.ptr(out), N * N, hip.ptr(lut), hip.stream())
        assert np.array_equal(got[off:off + N * N * 3], out.cpu().numpy().reshape(-1)), it[:5]


def test_identity_angle_is_the_copy_path(pool):
    from ryolov4_amd.datasets import augment as A
    luts = np.stack([A.hsv_luts(np.asarray(g, dtype=np.float64)) for g in GAINS])
    rot, cop = [], []
    for s, (H, W) in enumerate(SCENES):
        for c in (32, 45, 64):
            for k, (x0, y0) in enumerate(_positions(H, W, c)):
                lut = k % 3 if k % 2 else -1
                rot.append((s, (x0, y0, c), (c, c), A.INTERP_ROT, lut, A.rot_window_maps(x0, y0, c, c, 0.0)[0]))
                cop.append((s, (x0, y0, c), (c, c), A.INTERP_COPY, lut))
    a, oa = A.resize_hsv_windows(pool, rot, luts)
    b, ob = A.resize_hsv_windows(pool, cop, luts)
    assert oa == ob and len(rot) == 54
    a, b = a.cpu().numpy(), b.cpu().numpy()
    for it, off in zip(rot, oa):                                                      # (item by item: the padding between results is never written)
        n = it[2][0] * it[2][1] * 3
        assert np.array_equal(a[off:off + n], b[off:off + n]), it[:5]


# ---------------------------------------------------------------------------------------------- the dataset
def _batch(ds, name):
    return ds.assemble_batch(K.DATASET_CASES[name][5])


def _same(a, b):
    assert a[1].shape == b[1].shape and _bytes(a[1]) == _bytes(b[1]), "images differ"
    assert a[2].shape == b[2].shape and _bytes(a[2]) == _bytes(b[2]), "targets differ"


@pytest.mark.parametrize("name", ["plain", "full_csl"])
def test_identity_angle_and_never_rotated_equal_rotate_none(name):
    """rates = (1.0,): Rotate(degrees=0, p=1) reads every window at the identity angle — the copy path's pixels and the plain shift's
    labels; Rotate(p=0) never rotates.  Both give the bits of rotate=None, and leave `rng` and the jitter generator where it leaves them."""
    from ryolov4_amd.datasets.scene_dataset import Rotate
    off = K.dataset(name, DEV, rotate=None)
    want = _batch(off, name)
    assert off.last_angles == [None] * len(off.last_windows) and want[2].shape[0] > 0
    for rot in (Rotate(degrees=0.0, p=1.0), dict(p=0.0)):
        ds = K.dataset(name, DEV, rotate=rot)
        _same(_batch(ds, name), want)
        assert ds.last_windows == off.last_windows and ds._wrng.getstate() == off._wrng.getstate()
        assert ds.rng[0].getstate() == off.rng[0].getstate() and _bytes(torch.from_numpy(ds.rng[1].get_state()[1])) == _bytes(torch.from_numpy(off.rng[1].get_state()[1]))
        assert ds.last_angles == ([0.0] if isinstance(rot, Rotate) else [None]) * len(off.last_windows)


def _twin(name, ds):
    """A BaseDataset over host-made windows, one per recorded use of ds's last batch: the plain cut and the restatement's labels for an
    unrotated use, the restated rotated cut and the mapped, IoF-filtered labels for a rotated one.  Same seeds, same draws from `rng`."""
    from ryolov4_amd.datasets import augment as A
    from ryolov4_amd.datasets.base_dataset import BaseDataset
    hyp, _, csl, _, _, _ = K.DATASET_CASES[name]
    imgs, polys, labels, _ = K.scenes()
    wins, angles = list(ds.last_windows), list(ds.last_angles)
    host_labels = []
    for (_, s, x0, y0, c), a in zip(wins, angles):
        if a is None:
            host_labels.append(SR.window_labels(polys[s], labels[s], x0, y0, c, K.IOF_THR))
        else:
            host_labels.append(RR.window_labels(polys[s], labels[s], RR.maps(x0, y0, c, K.S, a)[1], c, K.IOF_THR))

    class Twin(BaseDataset):
        def _use_shape(self, index, row):
            return wins[row][4], wins[row][4]

        def _use_labels(self, index, row):
            return host_labels[row]

        def _pixel_stage(self, pool, items, luts):
            cuts = [SR.cut_window(imgs[s], x0, y0, c) for _, s, x0, y0, c in wins]
            stage, offs = A.resize_hsv_batch(A.ImagePool(cuts, torch.device(DEV)), [(k, hw, interp, lut) for k, (_, hw, interp, lut) in enumerate(items)], luts)
            for row, a in enumerate(angles):
                if a is not None:
                    _, s, x0, y0, c = wins[row]
                    (n, _), lut = items[row][1], items[row][3]
                    cut = RR.rot_cut(imgs[s], RR.maps(x0, y0, c, n, a)[0], n)
                    cut = cut if lut < 0 else _lut_pixels(cut, luts[lut])
                    stage[offs[row]:offs[row] + cut.size] = torch.from_numpy(np.ascontiguousarray(cut).reshape(-1)).to(DEV)
            return stage, offs

    tw = Twin(hyp, K.S, True, csl, False, device=DEV, rng=(random.Random(5), np.random.RandomState(5)))
    tw.set_arrays([np.zeros((1, 1, 3), np.uint8)] * len(ds), [np.zeros((0, 8), np.float32)] * len(ds), [np.zeros(0, np.float32)] * len(ds))
    return tw


@pytest.mark.parametrize("name", ["plain", "plain_rates", "full_kfiou", "full_csl"])
def test_dataset_equals_a_host_twin(name):
    ds = K.dataset(name, DEV)
    got = _batch(ds, name)
    planned = K.plan(name)
    assert (ds.last_windows, ds.last_angles) == planned                               # the cases the CPU test checked the decision gaps of
    assert any(a is not None for a in ds.last_angles) and len(ds.last_angles) == len(ds.last_windows)
    want = _batch(_twin(name, ds), name)
    assert got[2].shape[0] > 0 and got[2].shape[1] == (187 if K.DATASET_CASES[name][2] else 7)
    _same(got, want)                                                                  # images, targets and their order, bit for bit


def test_ignore_rows_of_rotated_uses():
    """ignore=Ignore(0.1, True) on the plain path: last_ignore is the restatement of tests/ignore_ref.py fed the MAPPED polygons and the
    window (0, 0, c) for a rotated use, the scene's polygons and (x0, y0, c) otherwise."""
    from ryolov4_amd.datasets.scene_dataset import SceneDataset

    class Spy(SceneDataset):
        def _label_side_stage(self, uses, mats, flags):
            self.seen = (list(uses), None if mats is None else np.array(mats), np.array(flags))
            return super()._label_side_stage(uses, mats, flags)

    ds = K.dataset("ignore", DEV, Spy)
    paths, imgs, targets = _batch(ds, "ignore")
    assert (ds.last_windows, ds.last_angles) == K.plan("ignore")
    uses, mats, flags = ds.seen
    want, rotated_rows = [], 0
    for row, slot, hw0, hw, u, mat in uses:
        _, s, x0, y0, c = ds.last_windows[row]
        polys, a = ds.scene_labels(s)[0], ds.last_angles[row]
        if a is not None:
            polys, x0, y0 = RR.map_polys(polys, RR.maps(x0, y0, c, hw[0], a)[1]), 0, 0
        _, shadow = IR.select(polys, ds.scene_difficult(s), x0, y0, c, K.IOF_LO, K.IOF_THR, True)
        for i in shadow:
            if IR.stage_keeps(polys[i], x0, y0, c, hw, u.border, u.crop, u.pad):
                want.append((slot, IR.vertex_path(polys[i], x0, y0, c, hw, u.pad, None if mat < 0 else mats[mat], int(flags[slot]), K.S)))
                rotated_rows += a is not None
    got = ds.last_ignore.cpu().numpy()
    assert rotated_rows > 0 and len(want) > rotated_rows and got.shape == (len(want), 9)
    assert got[:, 0].tolist() == [float(s) for s, _ in want]
    np.testing.assert_allclose(got[:, 1:], np.stack([q for _, q in want]), rtol=0, atol=1e-5)       # (the bound of tests/test_gpu_scene_ignore.py)
    # the targets are the twin's rows minus the difficult labels: every target row is finite and inside its slot range
    assert targets.shape[0] > 0 and bool(torch.isfinite(targets).all()) and int(targets[:, 0].max()) < len(paths)


def test_one_batch_through_the_criterion():
    from tests import ignore_cases as C
    from ryolov4_amd.lib.loss import ComputeKFIoULoss
    from ryolov4_amd.synth import HYP
    ds = K.dataset("loss", DEV)
    paths, imgs, targets = _batch(ds, "loss")
    assert imgs.shape == (4, 3, K.S, K.S) and targets.shape[0] > 0 and any(a is not None for a in ds.last_angles)
    assert bool(torch.isfinite(imgs).all()) and bool(torch.isfinite(targets).all())
    crit = ComputeKFIoULoss(C.Model("kfiou"), HYP)
    outs = [x.to(DEV).requires_grad_() for x in C.heads("kfiou")]
    tg = targets[targets[:, 0] < 2]                                                   # (the planted heads are a batch of 2)
    loss, _ = crit(outs, tg)
    loss.backward()
    assert bool(torch.isfinite(loss).all()) and all(bool(torch.isfinite(o.grad).all()) for o in outs) and tg.shape[0] > 0


def test_load_data_passes_rotate(tmp_path):
    import os
    from ryolov4_amd.lib.load import load_data
    imgs, polys, labels, _ = K.scenes()
    classes = ["plane", "small vehicle", "ship"]
    base = str(tmp_path)
    os.makedirs(os.path.join(base, "images"))
    os.makedirs(os.path.join(base, "annfiles"))
    images = {}
    for i, im in enumerate(imgs):
        ip = os.path.join(base, "images", "%03d.png" % i)
        open(ip, "wb").close()
        with open(os.path.join(base, "annfiles", "%03d.txt" % i), "w") as fh:
            for p, c in zip(polys[i], labels[i]):
                fh.write(" ".join(repr(float(v)) for v in p) + " " + classes[int(c)].replace(" ", "-") + " 0\n")
        images[ip] = im
    kw = dict(imread=lambda p: images[p], imsize=lambda p: images[p].shape[:2], device=DEV)
    ds, loader = load_data(base, classes, "DOTA_scenes", K.FULL, False, img_size=K.S, batch_size=3, augment=True, shuffle=False, overlap=16,
                           rotate=dict(degrees=90.0, p=1.0, step=90.0, seed=2), **kw)
    assert (ds.rotate.degrees, ds.rotate.p, ds.rotate.step, ds.rotate.seed) == (90.0, 1.0, 90.0, 2)
    paths, im, tg = next(iter(loader))
    assert im.shape == (3, 3, K.S, K.S) and bool(torch.isfinite(tg).all())
    assert all(a in (-90.0, 0.0, 90.0) for a in ds.last_angles) and len(ds.last_angles) == len(ds.last_windows) >= 3
    with pytest.raises(ValueError):
        load_data(base, classes, "DOTA_scenes", K.FULL, False, img_size=K.S, augment=False, overlap=16, rotate=dict(p=1.0), **kw)
