"""Ignore rows of scene training on the GPU: SceneDataset(ignore=Ignore(...)) against tests/ignore_ref.py (which labels become rows, where
their vertices go), and one step that hands `dataset.last_ignore` to the criterion through DeviceLoader.

The planted scene (side 96 k, window side 96 k, k = 1 or 2; canvas 96) holds four rectangles of side 20 k:
    A  whole                         -> a target
    B  8 k of its 20 k columns inside: IoF 0.4   -> no target (iof_thr 0.7), an ignore row (iof_lo 0.1)
    C  1 k of 20 k columns inside:     IoF 0.05  -> neither
    D  whole and difficult           -> an ignore row and no target with Ignore(difficult=True), a target otherwise
"""
import random

import numpy as np
import pytest
import torch

from tests import ignore_cases as K
from tests import ignore_ref as R
from tests import scene_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 96
PLAIN = dict(mosaic=0.0, mixup=0.0, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, rotate=10.0, scale=0.3, translate=0.1, fliplr=1.0, flipud=0.0)
MOSAIC = dict(PLAIN, mosaic=1.0, mixup=0.5, fliplr=0.5, flipud=0.3)
RECTS = np.array([[10, 10, 30, 10, 30, 30, 10, 30], [88, 40, 108, 40, 108, 60, 88, 60], [95, 70, 115, 70, 115, 90, 95, 90],
                  [50, 50, 70, 50, 70, 70, 50, 70]], dtype=np.float32)
CLS = np.array([0, 1, 2, 1], dtype=np.float32)
DIFFICULT = [0, 0, 0, 1]


def _scene(k):
    rs = np.random.RandomState(3)
    return rs.randint(0, 256, (S * k, S * k, 3), dtype=np.uint8), RECTS * k


def _ds(k, augment, hyp, ignore, seed=5, **kw):
    from ryolov4_amd.datasets.scene_dataset import SceneDataset

    class Spy(SceneDataset):
        """Records what the hook of assemble_batch was handed."""
        def _label_side_stage(self, uses, mats, flags):
            self.seen = (list(uses), None if mats is None else np.array(mats), np.array(flags))
            return super()._label_side_stage(uses, mats, flags)

    ds = Spy(hyp, S, augment, False, device=DEV, rng=(random.Random(seed), np.random.RandomState(seed)), overlap=0, rates=(1.0 / k,),
             window_seed=seed, ignore=ignore, **kw)
    img, polys = _scene(k)
    ds.set_arrays([img], [polys], [CLS], difficult=[DIFFICULT])
    assert ds.items == [(0, 0, 0, 0, S * k)]
    return ds


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _want_rows(ds, use_difficult, iof_lo=0.1):
    """The restatement's ignore rows of the last (non-mosaic) batch: [(slot, label index, eight coordinates)], in the loader's order."""
    uses, mats, flags = ds.seen
    out = []
    for row, slot, hw0, hw, u, mat in uses:
        _, s, x0, y0, c = ds.last_windows[row]
        polys, _ = ds.scene_labels(s)
        _, shadow = R.select(polys, ds.scene_difficult(s), x0, y0, c, iof_lo, ds.iof_thr, use_difficult)
        for i in shadow:
            if R.stage_keeps(polys[i], x0, y0, c, hw, u.border, u.crop, u.pad):
                out.append((slot, i, R.vertex_path(polys[i], x0, y0, c, hw, u.pad, None if mat < 0 else mats[mat], int(flags[slot]), S)))
    return out


@pytest.mark.parametrize("k", [1, 2])
def test_planted_scene_without_augmentation(k):
    from ryolov4_amd.datasets.base_dataset import BaseDataset
    from ryolov4_amd.datasets.scene_dataset import Ignore
    img, polys = _scene(k)
    off = _ds(k, False, PLAIN, None)
    b_off = off.assemble_batch([0, 0])
    assert off.last_ignore is None
    # ignore=None is what the dataset was: a BaseDataset over the window cut on the host with the restatement's labels
    pre = BaseDataset(PLAIN, S, False, False, False, device=DEV)
    p, c = SR.window_labels(polys, CLS, 0, 0, S * k, 0.7)
    pre.set_arrays([SR.cut_window(img, 0, 0, S * k)], [p], [c])
    b_pre = pre.assemble_batch([0, 0])
    assert _bytes(b_off[1]) == _bytes(b_pre[1]) and b_off[2].shape == (4, 7) and _bytes(b_off[2]) == _bytes(b_pre[2])
    assert b_off[2][:, 1].tolist() == [0.0, 1.0, 0.0, 1.0]          # A and D of both slots

    # difficult=False: the targets do not change, B alone is ignored
    soft = _ds(k, False, PLAIN, Ignore(0.1, False))
    b_soft = soft.assemble_batch([0, 0])
    assert _bytes(b_soft[1]) == _bytes(b_off[1]) and _bytes(b_soft[2]) == _bytes(b_off[2])
    want = _want_rows(soft, False)
    assert [(s, i) for s, i, _ in want] == [(0, 1), (1, 1)]
    got = soft.last_ignore
    assert got.dtype == torch.float32 and got.device.type == "cuda" and got.shape == (2, 9) and got[:, 0].tolist() == [0.0, 1.0]
    np.testing.assert_allclose(got[:, 1:].cpu().numpy(), np.stack([q for _, _, q in want]), rtol=0, atol=1e-5)

    # difficult=True: A alone is a target; B and D are ignored
    hard = _ds(k, False, PLAIN, dict(iof_lo=0.1, difficult=True))
    b_hard = hard.assemble_batch([0, 0])
    assert _bytes(b_hard[1]) == _bytes(b_off[1])
    assert b_hard[2].shape == (2, 7) and _bytes(b_hard[2]) == _bytes(b_off[2][[0, 2]])
    want = _want_rows(hard, True)
    assert [(s, i) for s, i, _ in want] == [(0, 1), (0, 3), (1, 1), (1, 3)]
    got = hard.last_ignore
    assert got.shape == (4, 9) and got[:, 0].tolist() == [0.0, 0.0, 1.0, 1.0]
    np.testing.assert_allclose(got[:, 1:].cpu().numpy(), np.stack([q for _, _, q in want]), rtol=0, atol=1e-5)
    # B by hand: columns 88 .. 108 of 96, rows 40 .. 60
    np.testing.assert_allclose(got[0, 1:].cpu().numpy(), np.array([88, 40, 108, 40, 108, 60, 88, 60]) / 96.0, rtol=0, atol=1e-6)
    # a lower iof_lo takes C in as well; label_table() holds every target whatever the option
    low = _ds(k, False, PLAIN, Ignore(0.01, True))
    low.assemble_batch([0])
    assert low.last_ignore.shape == (3, 9)
    assert _bytes(hard.label_table()) == _bytes(off.label_table()) and hard.label_table().shape == (2, 7)
    assert hard.last_ignore is got                                    # (label_table leaves the last batch's rows alone)


@pytest.mark.parametrize("k", [1, 2])
def test_warp_and_flip_follow_the_vertex_path(k):
    """augment=True, mosaic 0, fliplr 1, fixed seeds: the fp32 stage against the float64 restatement on a 96-pixel canvas, bound 1e-3 px
    (a few hundred fp32 roundings of coordinates below 2^8 would still stay under it).  Measured maximum: 7.6e-6 px, for k = 1 and k = 2."""
    from ryolov4_amd.datasets.scene_dataset import Ignore
    ds = _ds(k, True, PLAIN, Ignore(0.1, True))
    paths, imgs, targets = ds.assemble_batch([0, 0, 0, 0])
    uses, mats, flags = ds.seen
    assert mats is not None and len(mats) == 4 and flags.tolist() == [1, 1, 1, 1]
    want = _want_rows(ds, True)
    got = ds.last_ignore.cpu().numpy()
    assert [(s, i) for s, i, _ in want] == [(s, i) for s in range(4) for i in (1, 3)]
    assert got.shape == (8, 9) and got[:, 0].tolist() == [float(s) for s, _, _ in want]
    err = float(np.abs(got[:, 1:].astype(np.float64) - np.stack([q for _, _, q in want])).max()) * S
    print("k", k, "largest vertex difference in pixels:", err)
    assert err <= 1e-3
    # the same seeds without the option: same pixels; the targets are those rows of the twin that are not D's
    twin = _ds(k, True, PLAIN, None)
    b = twin.assemble_batch([0, 0, 0, 0])
    assert _bytes(b[1]) == _bytes(imgs)
    soft = _ds(k, True, PLAIN, Ignore(0.1, False))
    c = soft.assemble_batch([0, 0, 0, 0])
    assert _bytes(c[1]) == _bytes(imgs) and _bytes(c[2]) == _bytes(b[2]) and soft.last_ignore.shape == (4, 9)


def test_mosaic_batches():
    from ryolov4_amd.datasets.scene_dataset import Ignore
    B = 6
    off = _ds(1, True, MOSAIC, None, seed=7)
    soft = _ds(1, True, MOSAIC, Ignore(0.1, False), seed=7)
    hard = _ds(1, True, MOSAIC, Ignore(0.1, True), seed=7)
    total = 0
    for _ in range(3):
        a, b, c = (d.assemble_batch([0] * B) for d in (off, soft, hard))
        assert _bytes(a[1]) == _bytes(b[1]) == _bytes(c[1])          # no draw from rng moved
        assert a[2].shape == b[2].shape and _bytes(a[2]) == _bytes(b[2])
        assert off.last_ignore is None and off.last_windows == soft.last_windows == hard.last_windows
        for ds, use_difficult in ((soft, False), (hard, True)):
            got = ds.last_ignore.cpu().numpy()
            uses = ds.seen[0]
            n = 0
            for row, slot, hw0, hw, u, mat in uses:
                _, s, x0, y0, cc = ds.last_windows[row]
                polys, _ = ds.scene_labels(s)
                _, shadow = R.select(polys, ds.scene_difficult(s), x0, y0, cc, 0.1, 0.7, use_difficult)
                n += sum(R.stage_keeps(polys[i], x0, y0, cc, hw, u.border, u.crop, u.pad) for i in shadow)
            assert got.shape == (n, 9) and np.isfinite(got).all()
            assert ((got[:, 0] >= 0) & (got[:, 0] < B) & (got[:, 0] == np.floor(got[:, 0]))).all()
            assert (np.diff(got[:, 0]) >= 0).all()                  # slot order, as the targets
            total += n
    assert total > 0


def test_one_step_through_the_device_loader():
    from ryolov4_amd.datasets.base_dataset import DeviceLoader
    from ryolov4_amd.datasets.scene_dataset import Ignore
    from ryolov4_amd.lib.loss import ComputeKFIoULoss
    from ryolov4_amd.synth import HYP
    ds = _ds(1, False, PLAIN, Ignore(0.1, True))
    ds._set_items(ds.items * 2)
    loader = DeviceLoader(ds, 2, shuffle=False)
    crit = ComputeKFIoULoss(K.Model("kfiou"), HYP)
    steps = 0
    for paths, imgs, targets in loader:
        assert imgs.shape == (2, 3, S, S) and ds.last_ignore.shape == (4, 9)
        outs = [x.to(DEV).requires_grad_() for x in K.heads("kfiou")]
        loss, items = crit(outs, targets, ignore=ds.last_ignore)
        loss.backward()
        recs = crit.debug_matches()
        want = [int(R.ignored(ds.last_ignore.cpu().numpy(), 2, 18, gs, recs[i]).sum()) for i, gs in enumerate(K.GS)]
        assert crit.ignored_cells.tolist() == want and sum(want) > 0
        for i, gs in enumerate(K.GS):
            m = torch.from_numpy(R.ignored(ds.last_ignore.cpu().numpy(), 2, 18, gs, recs[i]))
            assert bool((outs[i].grad[..., 5].cpu()[m] == 0).all()) and bool(torch.isfinite(outs[i].grad).all())
        steps += 1
    assert steps == 1
