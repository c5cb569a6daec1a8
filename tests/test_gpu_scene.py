"""GPU tests of training on full-size scenes (csrc/scene.hip, datasets/scene_dataset.py).

  pixels   ryolo_resize_hsv_windows against the EXISTING ryolo_resize_hsv_batch run on windows cut on the host (114 outside the scene):
           np.array_equal for the copy path, the exact 2 x block path, generic INTER_LINEAR, both INTER_AREA forms, with and without hsv;
  labels   ryolo_scene_label_rows against tests/scene_ref.py bit for bit (IoF as float64 bytes, shifted polygons, NaN rows), and through
           ryolo_label_stage + ryolo_encode_labels against the same chain fed with the restatement's pre-filtered labels;
  dataset  SceneDataset against BaseDataset over pre-cut windows with pre-filtered labels: same images and targets, bit for bit, plain
           and with mosaic / mixup / warp / hsv under the same seeds; seeded jitter; keep_empty; load_data(..., "DOTA_scenes").
Network size 64 throughout."""
import os
import random

import numpy as np
import pytest
import torch

from tests import scene_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 64
SCENE_SHAPES = ((97, 131), (40, 40), (211, 53))          # H x W; the second is smaller than every window
HYP = dict(mosaic=1.0, mixup=0.5, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, rotate=10.0, scale=0.3, translate=0.1, fliplr=0.5, flipud=0.3)
CLASSES = ["plane", "small vehicle", "ship"]


def _rot_rects(rs, n, W, H, lo, hi, margin):
    """n rotated rectangles with sides lo .. hi px around an H x W scene, clockwise and counter-clockwise, float32 [n, 8]."""
    cx, cy = rs.uniform(-margin, W + margin, n), rs.uniform(-margin, H + margin, n)
    w, h, a = rs.uniform(lo, hi, n), rs.uniform(lo, hi, n), rs.uniform(0, np.pi, n)
    ux, uy = np.cos(a) * w / 2, np.sin(a) * w / 2
    vx, vy = -np.sin(a) * h / 2, np.cos(a) * h / 2
    q = np.stack([cx - ux - vx, cy - uy - vy, cx + ux - vx, cy + uy - vy, cx + ux + vx, cy + uy + vy, cx - ux + vx, cy - uy + vy], 1)
    flip = rs.rand(n) < 0.5
    q[flip] = q[flip].reshape(-1, 4, 2)[:, ::-1].reshape(-1, 8)
    return q.astype(np.float32)


@pytest.fixture(scope="module")
def scenes():
    rs = np.random.RandomState(11)
    imgs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in SCENE_SHAPES]
    polys = [_rot_rects(rs, 40, w, h, 4, 30, 5) for h, w in SCENE_SHAPES]
    labels = [rs.randint(0, 3, size=40).astype(np.float32) for _ in SCENE_SHAPES]
    return imgs, polys, labels


# ---------------------------------------------------------------------------------------------- 1. pixels
def _origins(H, W, c):
    out = [(x, 3) for x in range(16)]                                                 # every x0 mod 16 (the register realignment)
    out += [(-5, -7), (-c + 1, 2), (2, -c + 1)]                                       # negative origins
    out += [(-10, H // 3), (W - c // 2, 5), (5, -c // 2), (5, H - c // 2)]            # over each border
    out += [(-c // 2, -c // 2), (W - c // 2, -c // 2), (-c // 2, H - c // 2), (W - c // 2, H - c // 2)]      # each corner
    out += [(W + 3, 2), (-c - 5, -c - 5)]                                             # wholly outside the scene
    out += [(W - c, H - c), (W - 16, H - 1), (W - 17, H - 2), (W - 33, H - 1)]        # the scene's last row and column: the read guard
    return out


def _pixel_cases():
    from ryolov4_amd.datasets import augment as A
    return [(64, A.INTERP_COPY), (32, A.INTERP_LINEAR), (48, A.INTERP_LINEAR), (128, A.INTERP_LINEAR), (80, A.INTERP_LINEAR), (80, A.INTERP_AREA), (128, A.INTERP_AREA)]


@pytest.mark.parametrize("hsv", [False, True])
def test_window_pixels_equal_the_existing_kernel_on_host_cuts(scenes, hsv):
    from ryolov4_amd.datasets import augment as A
    imgs = scenes[0]
    gains = [(1.01, 1.4, 0.7), (0.99, 0.5, 1.3), (1.0, 1.0, 1.0)]
    luts = np.stack([A.hsv_luts(np.asarray(g, dtype=np.float64)) for g in gains]) if hsv else None
    wins, cuts, ref_items = [], [], []
    for s, im in enumerate(imgs):
        for c, interp in _pixel_cases():
            for x0, y0 in _origins(im.shape[0], im.shape[1], c):
                lut = len(wins) % 3 if hsv else -1
                wins.append((s, (x0, y0, c), (S, S), interp, lut))
                ref_items.append((len(cuts), (S, S), interp, lut))
                cuts.append(R.cut_window(im, x0, y0, c))
    assert len(wins) == 3 * 7 * 33
    pool = A.ImagePool(imgs, torch.device(DEV))
    stage, offs = A.resize_hsv_windows(pool, wins, luts)                              # every item in ONE launch
    ref_stage, ref_offs = A.resize_hsv_batch(A.ImagePool(cuts, torch.device(DEV)), ref_items, luts)
    assert offs == ref_offs
    got, want = stage.cpu().numpy(), ref_stage.cpu().numpy()
    for k, (w, off) in enumerate(zip(wins, offs)):
        a, b = got[off:off + S * S * 3], want[off:off + S * S * 3]
        assert np.array_equal(a, b), (w, int((a != b).sum()), int(np.flatnonzero(a != b)[0]))
    if not hsv:
        outside = next(k for k, w in enumerate(wins) if w[0] == 0 and w[1] == (131 + 3, 2, 64))
        assert (got[offs[outside]:offs[outside] + S * S * 3] == 114).all()             # a window that misses the scene is the fill


def test_window_pixels_odd_sizes_and_empty_launch(scenes):
    """Results that are no multiple of 16 pixels (the tail chunk of the copy path), non-square results, rows shorter than a chunk, and
    nitems = 0."""
    from ryolov4_amd.datasets import augment as A
    from ryolov4_amd import hip
    imgs = scenes[0]
    pool = A.ImagePool(imgs, torch.device(DEV))
    luts = np.stack([A.hsv_luts(np.asarray((1.01, 1.4, 0.7), dtype=np.float64))])
    wins, cuts, ref_items = [], [], []
    for s, (x0, y0, c), hw, interp, lut in [(0, (7, 9, 37), (37, 37), A.INTERP_COPY, -1), (0, (100, 70, 37), (37, 37), A.INTERP_COPY, 0),
                                            (2, (-3, 190, 9), (9, 9), A.INTERP_COPY, -1), (1, (-2, -2, 50), (50, 50), A.INTERP_COPY, 0),
                                            (2, (1, 1, 52), (52, 52), A.INTERP_COPY, -1), (0, (50, 20, 70), (33, 47), A.INTERP_AREA, 0),
                                            (2, (-9, 100, 90), (47, 33), A.INTERP_LINEAR, -1), (0, (0, 0, 1), (1, 1), A.INTERP_COPY, -1)]:
        wins.append((s, (x0, y0, c), hw, interp, lut))
        ref_items.append((len(cuts), hw, interp, lut))
        cuts.append(R.cut_window(imgs[s], x0, y0, c))
    stage, offs = A.resize_hsv_windows(pool, wins, luts)
    ref_stage, ref_offs = A.resize_hsv_batch(A.ImagePool(cuts, torch.device(DEV)), ref_items, luts)
    got, want = stage.cpu().numpy(), ref_stage.cpu().numpy()
    for w, off in zip(wins, offs):
        n = w[2][0] * w[2][1] * 3
        assert np.array_equal(got[off:off + n], want[off:off + n]), w
    stage0, offs0 = A.resize_hsv_windows(pool, [])
    assert offs0 == [] and stage0.numel() == 16
    dummy = torch.zeros(64, dtype=torch.uint8, device=DEV)
    hip.call("ryolo_resize_hsv_windows", hip.ptr(pool.buf), hip.ptr(dummy), 0, 0, None, hip.ptr(dummy), hip.stream())      # nitems = 0: nothing runs
    torch.cuda.synchronize()
    assert int(dummy.sum()) == 0
    with pytest.raises(ValueError):
        A.resize_hsv_windows(pool, [(0, (0, 0, 64), (32, 32), A.INTERP_COPY, -1)])
    with pytest.raises(RuntimeError):
        hip.call("ryolo_resize_hsv_windows", None, hip.ptr(dummy), 1, 16, None, hip.ptr(dummy), hip.stream())


# ---------------------------------------------------------------------------------------------- 2. labels
def _label_scene(rs, H, W, n):
    q = _rot_rects(rs, n, W, H, 4, 60, 30)
    k = n // 20
    q[0:k] = q[0:k, [0, 1, 0, 1, 4, 5, 4, 5]]                                         # degenerate: a segment (no area)
    q[k:2 * k, 2:] = q[k:2 * k, :2].repeat(3, 0).reshape(k, 6)                        # degenerate: a point
    q[2 * k:4 * k] = q[2 * k:4 * k, [0, 1, 4, 5, 2, 3, 6, 7]]                         # self-intersecting: a bow tie
    q[4 * k:5 * k] = np.round(q[4 * k:5 * k])                                         # integer vertices: some land on window borders
    return q


def _encode(targets10, nslots):
    """ryolo_encode_labels as finalize_batch calls it (no flips, xywha targets): [count, 7] on the host."""
    from ryolov4_amd import hip
    nt = targets10.shape[0]
    out = torch.empty((nt, 7), dtype=torch.float32, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    hip.call("ryolo_encode_labels", hip.ptr(targets10) if nt else None, nt, S, S, None, None, 0, hip.ptr(out) if nt else None, count.data_ptr(), None,
             hip.stream())
    return out[:int(count.item())].cpu().numpy()


def test_label_rows_equal_the_restatement_bit_for_bit():
    from ryolov4_amd.datasets import augment as A
    rs = np.random.RandomState(21)
    thr = 0.7
    shapes = ((300, 400), (260, 180), (90, 500))
    polys = [_label_scene(rs, h, w, 400) for h, w in shapes]
    cls = [rs.randint(0, 5, size=400).astype(np.float32) for _ in shapes]
    wins = []                                                                         # (scene, x0, y0, c): 24 windows, 8 per scene
    for s, (h, w) in enumerate(shapes):
        wins += [(s, -20, -30, 64), (s, 0, 0, 128), (s, w - 64, h - 64, 64), (s, w - 40, -10, 128), (s, 37, 21, 64), (s, -100, h - 50, 128),
                 (s, w // 2, h // 2, 32), (s, 11, h // 3, 200)]
    use = A.Use(0, None, (0, 0), None, None)
    rows, ref_rows, win_of_row, ref = [], [], [], []
    for wi, (s, x0, y0, c) in enumerate(wins):
        idx = R.cull(polys[s], x0, y0, c)
        rows.append(A.label_rows(polys[s][idx], cls[s][idx], wi, (1, 1), (S, S), use))          # (w0, h0: the kernel sets them to c)
        win_of_row.append(np.full(len(idx), wi, dtype=np.int32))
        sh, iof, keep = R.label_rows(polys[s][idx], x0, y0, c, thr)
        ref.append((sh, iof, keep, np.full(len(idx), c, dtype=np.float32)))
        ref_rows.append(A.label_rows(sh[keep], cls[s][idx][keep], wi, (c, c), (S, S), use))     # what a pre-cut window's label file holds
    rows, win_of_row, ref_rows = np.concatenate(rows), np.concatenate(win_of_row), np.concatenate(ref_rows)
    sh, iof, keep, cs = (np.concatenate([r[k] for r in ref]) for k in range(4))
    n = len(rows)
    assert n > 1000 and 0.1 < keep.mean() < 0.9 and ((iof > 0) & (iof < 1)).sum() > 300 and (iof == 0).sum() > 50
    table = A.upload_label_rows(rows, DEV)
    got_iof = A.scene_label_rows(table, n, win_of_row, [w[1:] for w in wins], thr, want_iof=True)
    assert got_iof.cpu().numpy().tobytes() == iof.tobytes()                            # IoF: bit for bit, as float64 bytes
    back = np.frombuffer(table.cpu().numpy().tobytes(), dtype=A.LABEL_ROW_DTYPE)
    assert np.array_equal(np.isnan(back["poly"]).all(1), ~keep) and not np.isnan(back["poly"][keep]).any()
    assert back["poly"][keep].tobytes() == sh[keep].tobytes()                          # kept: the shifted polygon, unclipped
    assert np.array_equal(back["w0"], cs) and np.array_equal(back["h0"], cs)
    for f in ("cls", "slot", "w1", "h1", "padw", "padh", "bx2", "cx2", "mat"):
        assert np.array_equal(back[f], rows[f]), f
    # without iof_out: the same table
    table2 = A.upload_label_rows(rows, DEV)
    assert A.scene_label_rows(table2, n, win_of_row, [w[1:] for w in wins], thr) is None
    assert table2.cpu().numpy().tobytes() == table.cpu().numpy().tobytes()
    # through the rest of the chain
    got = _encode(A.label_stage_table(table, n, None, DEV), len(wins))
    want = _encode(A.label_stage(ref_rows, None, DEV), len(wins))
    assert got.shape == want.shape and got.shape[0] > 100 and got.tobytes() == want.tobytes()
    # another threshold through the same kernel, and the argument checks
    table3 = A.upload_label_rows(rows, DEV)
    A.scene_label_rows(table3, n, win_of_row, [w[1:] for w in wins], 1.0)
    back3 = np.frombuffer(table3.cpu().numpy().tobytes(), dtype=A.LABEL_ROW_DTYPE)
    assert np.array_equal(~np.isnan(back3["poly"]).any(1), iof >= 1.0) and (iof >= 1.0).sum() > 20
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(RuntimeError):
            A.scene_label_rows(table3, n, win_of_row, [w[1:] for w in wins], bad)
    with pytest.raises(ValueError):
        A.scene_label_rows(table3, n, win_of_row + 24, [w[1:] for w in wins], thr)


def test_label_rows_entry_point_drops_rows_without_a_window():
    """The C entry point by itself (no wrapper check): a row whose window index is outside [0, nwin) becomes a NaN row with IoF 0 and
    `wins` is not read for it; its neighbours are unaffected."""
    from ryolov4_amd import hip
    from ryolov4_amd.datasets import augment as A
    sq = np.asarray([10, 10, 20, 10, 20, 20, 10, 20], dtype=np.float32)
    rows = np.zeros(5, dtype=A.LABEL_ROW_DTYPE)
    rows["poly"] = sq
    rows["w0"] = rows["h0"] = 7
    table = A.upload_label_rows(rows, DEV)
    wor = torch.tensor([0, 1, -1, 2, 1 << 30], dtype=torch.int32, device=DEV)
    wins = torch.tensor([[0, 0, 64], [5, 5, 32]], dtype=torch.int32, device=DEV)
    iof = torch.full((5,), -1.0, dtype=torch.float64, device=DEV)
    hip.call("ryolo_scene_label_rows", hip.ptr(table), 5, hip.ptr(wor), hip.ptr(wins), 2, 0.7, hip.ptr(iof), hip.stream())
    back = np.frombuffer(table.cpu().numpy().tobytes(), dtype=A.LABEL_ROW_DTYPE)
    assert iof.cpu().tolist() == [1.0, 1.0, 0.0, 0.0, 0.0]
    assert np.array_equal(back["poly"][0], sq) and np.array_equal(back["poly"][1], sq - 5) and np.isnan(back["poly"][2:]).all()
    assert back["w0"].tolist() == [64, 32, 7, 7, 7] and back["h0"].tolist() == [64, 32, 7, 7, 7]
    with pytest.raises(RuntimeError):
        hip.call("ryolo_scene_label_rows", hip.ptr(table), 5, hip.ptr(wor), hip.ptr(wins), -1, 0.7, None, hip.stream())


# ---------------------------------------------------------------------------------------------- 3. the dataset
def _scene_ds(scenes, augment, rng=None, **kw):
    from ryolov4_amd.datasets.scene_dataset import SceneDataset
    ds = SceneDataset(HYP, S, augment, False, device=DEV, rng=rng, overlap=16, **kw)
    ds.set_arrays(*scenes)
    return ds


def _precut_ds(scenes, items, augment, thr, rng=None):
    """BaseDataset over the items' windows cut on the host, labels pre-filtered by the restatement."""
    from ryolov4_amd.datasets.base_dataset import BaseDataset
    imgs, polys, labels = scenes
    cuts, ps, cs = [], [], []
    for s, _, x0, y0, c in items:
        cuts.append(R.cut_window(imgs[s], x0, y0, c))
        p, k = R.window_labels(polys[s], labels[s], x0, y0, c, thr)
        ps.append(p)
        cs.append(k)
    ds = BaseDataset(HYP, S, augment, False, False, device=DEV, rng=rng)
    ds.set_arrays(cuts, ps, cs)
    return ds


def _same(a, b):
    assert a[1].shape == b[1].shape and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes(), "images differ"
    assert a[2].shape == b[2].shape and a[2].cpu().numpy().tobytes() == b[2].cpu().numpy().tobytes(), "targets differ"


def test_plain_items_equal_precut_windows(scenes):
    ds = _scene_ds(scenes, False, rates=(1.0, 0.5), keep_empty=True, iof_thr=0.6)
    assert ds.jitter is False and len(ds) == sum(len(R.scene_windows(h, w, S, 16, (1.0, 0.5))) for h, w in SCENE_SHAPES) == 17
    ref = _precut_ds(scenes, ds.items, False, 0.6)
    idx = list(range(len(ds)))
    got, want = ds.assemble_batch(idx), ref.assemble_batch(idx)
    _same(got, want)
    assert got[2].shape[0] > 20 and got[0] == [ds.img_files[i] for i in idx] and got[0][0] == "<array 0>#0,0,64"
    assert ds.last_windows == [(i,) + (it[0],) + it[2:] for i, it in enumerate(ds.items)]
    for i in (0, 7, len(ds) - 1):                                                     # one item at a time (API parity path)
        a, b = ds[i], ref[i]
        assert a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes() and a[2].cpu().numpy().tobytes() == b[2].cpu().numpy().tobytes()


def test_augmented_items_equal_precut_windows_under_the_same_seeds(scenes):
    """mosaic = 1.0, mixup = 0.5, warp, hsv, flips; jitter off: the windows are the planned ones, so a BaseDataset over their host cuts
    makes the same draws and must give the same bits.  Rates 1, 0.5, 0.8: copy, exact 2 x and generic INTER_LINEAR sources."""
    kw = dict(rates=(1.0, 0.5, 0.8), keep_empty=True, jitter=False)
    ds = _scene_ds(scenes, True, rng=(random.Random(5), np.random.RandomState(5)), **kw)
    ref = _precut_ds(scenes, ds.items, True, 0.7, rng=(random.Random(5), np.random.RandomState(5)))
    assert len(ds) == len(ref) > 20
    for idx in ([0, 3, 8, len(ds) - 1, 5, 5], [2, 11, 7]):
        got, want = ds.assemble_batch(idx), ref.assemble_batch(idx)
        _same(got, want)
        assert len(ds.last_windows) >= 4 * len(idx)                                   # mosaic partners are uses too
    assert got[2].shape[0] > 0


class _Spy:
    """Mixed into SceneDataset: keeps what the two scene stages produced for the last batch."""

    def _pixel_stage(self, pool, items, luts):
        out = super()._pixel_stage(pool, items, luts)
        self.seen_pixels = (list(items), None if luts is None else np.array(luts), out[0].clone(), list(out[1]))
        return out

    def _label_table(self, rows):
        out = super()._label_table(rows)
        self.seen_labels = (rows.copy(), np.concatenate(self._row_wins) if self._row_wins else np.zeros(0, np.int32),
                            out.clone())
        return out


def test_seeded_jitter(scenes):
    from ryolov4_amd.datasets import augment as A
    from ryolov4_amd.datasets.base_dataset import DeviceLoader
    from ryolov4_amd.datasets.scene_dataset import SceneDataset
    imgs, polys, labels = scenes
    Spy = type("Spy", (_Spy, SceneDataset), {})

    def make(seed=3):
        ds = Spy(HYP, S, True, False, device=DEV, rng=(random.Random(9), np.random.RandomState(9)), overlap=16, rates=(1.0, 0.5), window_seed=seed,
                 p_object=0.5, keep_empty=True)
        ds.set_arrays(imgs, polys, labels)
        return ds

    ds = make()
    assert ds.jitter is True
    idx = [1, 6, 9, 13, 2]
    out = ds.assemble_batch(idx)
    # the windows are the restatement's draws, in use order
    wr = random.Random(3)
    for item, s, x0, y0, c in ds.last_windows:
        assert (s, c) == (ds.items[item][0], ds.items[item][4])
        assert (x0, y0) == R.jitter_window(wr, imgs[s].shape[0], imgs[s].shape[1], c, polys[s], 0.5)
    assert any(w[2] < 0 or w[3] < 0 for w in ds.last_windows) and len(ds.last_windows) >= 20
    # pixels of the stage: the existing kernel on host cuts of those windows
    items, luts, stage, offs = ds.seen_pixels
    cuts = [R.cut_window(imgs[s], x0, y0, c) for _, s, x0, y0, c in ds.last_windows]
    ref_stage, ref_offs = A.resize_hsv_batch(A.ImagePool(cuts, torch.device(DEV)), [(k, hw, interp, lut) for k, (_, hw, interp, lut) in enumerate(items)], luts)
    assert offs == ref_offs and stage.cpu().numpy().tobytes() == ref_stage.cpu().numpy().tobytes()
    # labels of the stage: the restatement, row by row
    rows, win_of_row, table = ds.seen_labels
    back = np.frombuffer(table.cpu().numpy().tobytes(), dtype=A.LABEL_ROW_DTYPE)
    assert len(back) == len(rows) == len(win_of_row) > 50
    at = 0
    for k, (_, s, x0, y0, c) in enumerate(ds.last_windows):
        cull = R.cull(polys[s], x0, y0, c)
        sh, _, keep = R.label_rows(polys[s][cull], x0, y0, c, 0.7)
        mine = back[at:at + len(cull)]
        assert (win_of_row[at:at + len(cull)] == k).all() and np.array_equal(mine["cls"], labels[s][cull])
        assert np.array_equal(np.isnan(mine["poly"]).all(1), ~keep) and mine["poly"][keep].tobytes() == sh[keep].tobytes()
        assert (mine["w0"] == c).all() and (mine["h0"] == c).all()
        at += len(cull)
    assert at == len(back)
    # the same seeds: the same bits; another window seed: other windows
    ds2 = make()
    _same(out, ds2.assemble_batch(idx))
    assert ds2.last_windows == ds.last_windows
    ds3 = make(seed=4)
    ds3.assemble_batch(idx)
    assert ds3.last_windows != ds.last_windows and [w[0] for w in ds3.last_windows] == [w[0] for w in ds.last_windows]
    # len, shard, DeviceLoader
    n = len(ds)
    ds4 = make()
    loader = DeviceLoader(ds4, 4, shuffle=True, rank=1, world_size=2)
    assert len(ds4) == -(-n // 2) and ds4.items == [ds.items[(1 + 2 * k) % n] for k in range(len(ds4))] and len(loader) == -(-len(ds4) // 4)
    seen = 0
    for paths, im, tg in loader:
        assert im.is_cuda and im.shape[1:] == (3, S, S) and tg.shape[1] == 7 and len(paths) == im.shape[0] and "#" in paths[0]
        assert tg.shape[0] == 0 or (int(tg[:, 0].max()) < im.shape[0] and bool(torch.isfinite(tg).all()))
        seen += im.shape[0]
    assert seen == len(ds4)


def test_keep_empty_false_removes_exactly_the_empty_windows(scenes):
    imgs, polys, labels = scenes
    sparse = [p[:3] for p in polys], [c[:3] for c in labels]                          # three labels per scene: most windows keep none
    for thr in (0.7, 0.3):
        full = _scene_ds((imgs,) + sparse, False, rates=(1.0, 2.0), keep_empty=True, iof_thr=thr)
        ds = _scene_ds((imgs,) + sparse, False, rates=(1.0, 2.0), iof_thr=thr)
        want = [it for it in full.items if len(R.window_labels(sparse[0][it[0]], sparse[1][it[0]], it[2], it[3], it[4], thr)[1])]
        assert ds.items == want and 0 < len(want) < len(full.items)
        assert ds.img_files == ["<array {}>#{},{},{}".format(s, x0, y0, c) for s, _, x0, y0, c in want]
        _, _, tg = ds.assemble_batch(list(range(len(ds))))
        assert tg.shape[0] > 0 and int(tg[:, 0].max()) < len(ds)


# ---------------------------------------------------------------------------------------------- 4. load_data
def test_load_data_dota_scenes(tmp_path, scenes):
    from ryolov4_amd.datasets.scene_dataset import DOTASceneDataset
    from ryolov4_amd.lib.load import load_data
    imgs, polys, labels = scenes
    base = str(tmp_path)
    os.makedirs(os.path.join(base, "images"))
    os.makedirs(os.path.join(base, "annfiles"))
    images = {}
    for i, im in enumerate(imgs):
        ip = os.path.join(base, "images", "%03d.png" % i)
        open(ip, "wb").close()
        with open(os.path.join(base, "annfiles", "%03d.txt" % i), "w") as fh:
            for p, c in zip(polys[i], labels[i]):
                fh.write(" ".join(repr(float(v)) for v in p) + " " + CLASSES[int(c)].replace(" ", "-") + " 0\n")
        images[ip] = im
    kw = dict(imread=lambda p: images[p], imsize=lambda p: images[p].shape[:2], device=DEV)
    ds, loader = load_data(base, CLASSES, "DOTA_scenes", HYP, False, img_size=S, batch_size=4, augment=False, shuffle=False, overlap=16, rates=(1.0, 0.5),
                           iof_thr=0.6, keep_empty=True, **kw)
    assert isinstance(ds, DOTASceneDataset) and (ds.overlap, ds.rates, ds.iof_thr, ds.keep_empty, ds.jitter) == (16, (1.0, 0.5), 0.6, True, False)
    assert ds.scene_files == sorted(images) and ds.category == {"plane": 0, "small-vehicle": 1, "ship": 2}
    ref = _scene_ds(scenes, False, rates=(1.0, 0.5), keep_empty=True, iof_thr=0.6)
    assert ds.items == ref.items and ds.img_files[0] == sorted(images)[0] + "#0,0,64" and ds.label_files[0].endswith(os.path.join("annfiles", "000.txt"))
    assert len(loader) == -(-len(ds) // 4)
    at = 0
    for paths, im, tg in loader:
        _same((paths, im, tg), ref.assemble_batch(list(range(at, at + len(paths)))))
        at += len(paths)
    assert at == len(ds)
    # training form: the keywords pass through, empty windows leave the table, batches come out
    tr, tl = load_data(base, CLASSES, "DOTA_scenes", HYP, False, img_size=S, batch_size=3, augment=True, shuffle=True, overlap=16, p_object=1.0, window_seed=5,
                       **kw)
    assert tr.jitter is True and tr.p_object == 1.0 and not tr.keep_empty and 0 < len(tr) <= len(ref)
    paths, im, tg = next(iter(tl))
    assert im.shape == (3, 3, S, S) and tg.shape[1] == 7 and bool(torch.isfinite(tg).all())
    with pytest.raises(ValueError):
        load_data(base, CLASSES, "DOTA_scenes", HYP, False, img_size=S, overlap=16, iof_thr=0.0, **kw)
