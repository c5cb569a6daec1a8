"""GPU tests of object-level copy-paste (csrc/copypaste.hip, datasets/copy_paste.py) against tests/copy_paste_ref.py, bit for bit.

  pixels   ryolo_paste_prepare + ryolo_paste_pixels on a hand-built table: destination quads, bounding boxes and every byte of the canvases;
  labels   ryolo_paste_labels: every bit of the rows, NaN positions included; nt = 0; items outside the slots (IGNORED: no pixel is written
           for them and their row is (0, cls, NaN x 8));
  dataset  SceneDataset(copy_paste=...) against the restatement's composition under the same seeds, against its twin without the option
           outside the pasted masks, the row order of the targets (csl and kfiou), copy_paste=None, label_table();
  loss     a pasted batch through ComputeKFIoULoss without dropped target rows.
Every condition a case is there for is asserted on the restatement first.  Scenes 96 x 160, 128 x 128, 160 x 97; S = 64; 5 slots."""
import random

import numpy as np
import pytest
import torch

from tests import copy_paste_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, B = 64, 5
SCENE_SHAPES = ((96, 160), (128, 128), (160, 97))
HYP_FULL = dict(mosaic=1.0, mixup=0.5, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, rotate=10.0, scale=0.3, translate=0.1, fliplr=0.5, flipud=0.3)
HYP_PLAIN = dict(mosaic=0.0, mixup=0.0, hsv_h=0.0, hsv_s=0.0, hsv_v=0.0, rotate=0.0, scale=0.0, translate=0.0, fliplr=0.0, flipud=0.0)


@pytest.fixture(scope="module")
def images():
    rs = np.random.RandomState(17)
    return [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in SCENE_SHAPES]


def _rect(cx, cy, w, h, a_deg, ccw=False):
    a = np.deg2rad(a_deg)
    ux, uy, vx, vy = np.cos(a) * w / 2, np.sin(a) * w / 2, -np.sin(a) * h / 2, np.cos(a) * h / 2
    q = np.array([cx - ux - vx, cy - uy - vy, cx + ux - vx, cy + uy - vy, cx + ux + vx, cy + uy + vy, cx - ux + vx, cy - uy + vy])
    if ccw:
        q = q.reshape(4, 2)[::-1].reshape(8)
    return q.astype(np.float32)


def _item(src, slot, cls, quad, angle, scale, cx, cy):
    M, Minv = R.matrices(quad, angle, scale, cx, cy)
    H, W = SCENE_SHAPES[src]
    return R.make_item(src, H, W, slot, cls, quad, M, Minv)


def _table():
    """The hand-built items, sorted by slot.  Slot 0: none.  Slot 1: one.  Slot 2: eleven overlapping ones around the centre (angles 0, 90
    (an exact quarter turn and the cos / sin of 90 degrees), generic; scales 0.5, 2.0).  Slot 3: sources reaching past their scene, boxes
    clipped by all four canvas edges.  Slot 4: small boxes at odd offsets, either vertex order."""
    items = [_item(0, 1, 3, _rect(80, 40, 30, 14, 20), 33.0, 1.0, 30.3, 29.6)]
    rs = random.Random(4)
    spec = [(0.0, 0.5), (90.0, 2.0), (17.0, 1.0), (-123.4, 0.5), (60.0, 2.0), (0.0, 2.0), (90.0, 0.5), (179.9, 1.3), (-45.0, 0.8), (271.0, 1.0)]
    for k, (ang, sc) in enumerate(spec):
        src = k % 3
        H, W = SCENE_SHAPES[src]
        quad = _rect(rs.uniform(30, W - 30), rs.uniform(30, H - 30), rs.uniform(10, 22), rs.uniform(8, 16), rs.uniform(0, 180), ccw=bool(k & 1))
        items.append(_item(src, 2, k % 4, quad, ang, sc, 32 + rs.uniform(-9, 9), 32 + rs.uniform(-9, 9)))
    quad = np.float32([40, 50, 60, 50, 60, 62, 40, 62])                              # an exact quarter turn, integer translation
    items.append(R.make_item(1, 128, 128, 2, 1, quad, (0.0, 1.0, -30.0, -1.0, 0.0, 85.0), (0.0, -1.0, 85.0, 1.0, 0.0, 30.0)))
    # sources past the scene: a quad over the right border of scene 0 and one over the top-left corner of scene 2; large, so the canvas clips them
    items.append(_item(0, 3, 0, np.float32([130, 60, 190, 60, 190, 120, 130, 120]), 10.0, 1.5, 50.0, 50.0))
    items.append(_item(2, 3, 2, np.float32([-20, -15, 30, -15, 30, 25, -20, 25]), -30.0, 1.2, 8.0, 10.0))
    items.append(_item(1, 3, 1, _rect(64, 64, 40, 20, 0), 0.0, 2.0, 32.0, 2.0))       # over the top edge, box 0 .. 64 wide
    for k, (cx, cy) in enumerate(((13.0, 9.0), (50.5, 21.25), (61.0, 61.0), (3.0, 40.0), (33.0, 62.5))):
        items.append(_item(k % 3, 4, k, _rect(60, 50, 11, 7, 15 * k, ccw=bool(k & 1)), 25.0 * k, 1.0, cx, cy))
    return items


def _device_items(items, pool):
    from ryolov4_amd.datasets import augment as A
    arr = np.zeros(len(items), dtype=A.PASTE_ITEM_DTYPE)
    for k, it in enumerate(items):
        arr[k] = (pool.offsets[it["src"]], it["SH"], it["SW"], it["slot"], it["cls"], it["quad"], it["M"], it["Minv"])
    return arr


def _pool(images):
    from ryolov4_amd.datasets import augment as A
    return A.ImagePool(images, torch.device(DEV))


def _canvases(seed=3):
    return np.random.RandomState(seed).randint(0, 256, size=(B, S, S, 3)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- 1. pixels
def test_pixels_equal_the_restatement_bit_for_bit(images):
    from ryolov4_amd.datasets import augment as A
    items = _table()
    first = R.first_table(items, B)
    final = _canvases()
    want, union, cover = R.paste_pixels(images, items, first, B, final)
    dq_ref, bbox_ref = R.prepare(items, first, B, S)
    # ---- the conditions this table is there for, on the restatement
    assert first.tolist() == [0, 0, 1, 12, 15, 20]
    assert not union[0].any() and union[1].any() and cover[1].max() == 1
    assert cover[2].max() >= 3 and (cover[2] >= 2).sum() > 50, "a pixel inside three pastes"
    bx = bbox_ref
    assert all(b.any() for b in bx), "every item reaches the canvas"
    assert any(b[0] % 4 and b[2] % 4 and (b[2] - b[0]) % 32 and b[1] % 8 and (b[3] - b[1]) % 8 for b in bx), "a box off every 4-pixel and tile boundary"
    assert any(b[0] == 0 for b in bx) and any(b[1] == 0 for b in bx) and any(b[2] == S for b in bx) and any(b[3] == S for b in bx), "boxes touch the canvas edges"
    assert any(b[2] - b[0] > 32 for b in bx) and any(b[3] - b[1] > 8 for b in bx), "more than one tile"
    for j in (12, 13):                                                               # taps outside the scene: the inverse map leaves it
        it = items[j]
        ys, xs = np.nonzero(R.inside_mask(dq_ref[j], S))
        sx = it["Minv"][0] * xs + it["Minv"][1] * ys + it["Minv"][2]
        sy = it["Minv"][3] * xs + it["Minv"][4] * ys + it["Minv"][5]
        out = (sx < -1) | (sx > it["SW"]) | (sy < -1) | (sy > it["SH"])
        assert out.sum() > 20 and (~out).sum() > 20
        assert (R.sample(images[it["src"]], it["Minv"], S)[ys[out], xs[out]] == 114).all()
    assert {0.5, 2.0} <= {round(float(np.hypot(it["M"][0], it["M"][1])), 6) for it in items}
    # ---- the device
    pool = _pool(images)
    table = A.PasteTable(_device_items(items, pool), B, DEV)
    assert table.first_host.tolist() == first.tolist()
    dev = torch.from_numpy(final).to(DEV)
    A.paste_prepare(table, S)
    A.paste_pixels(pool.buf, table, dev)
    assert table.dq.cpu().numpy().tobytes() == dq_ref.tobytes(), "destination quads"
    assert np.array_equal(table.bbox.cpu().numpy(), bbox_ref), "bounding boxes"
    assert all(bw <= table.max_box[0] and bh <= table.max_box[1] for bw, bh in zip(bx[:, 2] - bx[:, 0], bx[:, 3] - bx[:, 1]))
    got = dev.cpu().numpy()
    diff = (got != want).any(-1)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5].tolist())
    assert np.array_equal(got[~union], final[~union]), "bytes outside the union of masks"
    assert (got[union] != final[union]).any(-1).mean() > 0.9                          # (and the masks were written)
    # a grid smaller than the boxes: the tile loop gives the same bytes
    dev2 = torch.from_numpy(final).to(DEV)
    table.max_box = (1, 1)
    A.paste_pixels(pool, table, dev2)
    assert np.array_equal(dev2.cpu().numpy(), want)


def test_empty_table_launches_nothing(images):
    from ryolov4_amd import hip
    from ryolov4_amd.datasets import augment as A
    pool = _pool(images)
    final = _canvases()
    dev = torch.from_numpy(final).to(DEV)
    tg = torch.rand(4, 10, device=DEV)
    out_final, out_tg, table = A.paste_objects(pool, dev, tg, np.zeros(0, dtype=A.PASTE_ITEM_DTYPE))
    assert out_final is dev and out_tg is tg and table.n == 0
    A.paste_prepare(table, S)                                                         # np = 0 through the entry points themselves
    A.paste_pixels(pool.buf, table, dev)
    rows = A.paste_labels(table, tg, 0.5)
    assert np.array_equal(dev.cpu().numpy(), final) and rows.cpu().numpy().tobytes() == tg.cpu().numpy().tobytes()
    assert A.paste_labels(table, tg[:0], 0.5).shape == (0, 10)
    with pytest.raises(RuntimeError):
        hip.call("ryolo_paste_labels", hip.ptr(tg), 4, None, 0, hip.ptr(table.first), B, None, 0.0, hip.ptr(rows), hip.stream())
    with pytest.raises(ValueError):
        A.PasteTable(_device_items(_table()[::-1], pool), B, DEV)                       # not sorted by slot


# ---------------------------------------------------------------------------------------------- 2. labels
def _rows(items, first):
    """Existing rows around the table's destination quads: shrunk copies (buried), far corners of the canvas, halves, a NaN row, a row
    without area, rows of slot 0 (no paste) and of a slot outside the batch."""
    dq, _ = R.prepare(items, first, B, S)
    rows = []
    for j, it in enumerate(items):
        q = dq[j].astype(np.float64).reshape(4, 2)
        c = q.mean(0)
        rows.append([it["slot"], 1] + (c + 0.5 * (q - c)).reshape(8).tolist())       # inside item j
        rows.append([it["slot"], 2] + (q + (q[1] - q[0]) * 0.55).reshape(8).tolist())  # shifted along an edge: a little under half covered by j
        rows.append([0, 3] + (c + 0.5 * (q - c)).reshape(8).tolist())                  # the same place in slot 0
    rows.append([1, 0, 1, 1, 6, 1, 6, 5, 1, 5])
    rows.append([2, 0] + [np.nan] * 8)
    rows.append([2, 0, 30, 30, 30, 30, 34, 34, 34, 34])
    rows.append([7, 0, 20, 20, 40, 20, 40, 40, 20, 40])
    rows.append([-1, 0, 20, 20, 40, 20, 40, 40, 20, 40])
    rows.append([np.nan, 0, 20, 20, 40, 20, 40, 40, 20, 40])
    return np.asarray(rows, dtype=np.float32)


@pytest.mark.parametrize("occ_thr", [0.5, 0.2])
def test_labels_equal_the_restatement_bit_for_bit(images, occ_thr):
    from ryolov4_amd.datasets import augment as A
    good = _table()
    # items outside the slots, before and behind the valid ones (still sorted): IGNORED by every kernel
    quad = _rect(64, 64, 30, 20, 0)
    items = [_item(1, -2, 5, quad, 0.0, 1.0, 32.0, 32.0)] + good + [_item(1, B, 6, quad, 0.0, 1.0, 32.0, 32.0), _item(1, 1 << 20, 7, quad, 0.0, 1.0, 32.0, 32.0)]
    first = R.first_table(items, B)
    tg = _rows(items, first)
    nt, n = len(tg), len(items)
    want = R.paste_labels(tg, items, first, B, S, occ_thr)
    # ---- conditions, on the restatement
    was, now = np.isnan(tg[:, 2:]).any(1), np.isnan(want[:nt, 2:]).any(1)
    assert (now & ~was).sum() >= 10 and (~now).sum() >= 10, "existing rows buried and not"
    assert not now[[r for r in range(nt) if tg[r, 0] == 0]].any(), "slot 0 has no paste"
    pasted = np.isnan(want[nt:, 2:]).any(1)
    assert pasted[[0, n - 2, n - 1]].all() and (want[[nt, nt + n - 2, nt + n - 1], 0] == 0).all(), "rows of the items outside the slots"
    slot2 = [j for j, it in enumerate(items) if it["slot"] == 2]
    assert pasted[slot2].any() and not pasted[slot2[-1]] and (~pasted).sum() >= 8, "a pasted row buried by a later paste"
    assert want[:nt, :2].tobytes() == tg[:, :2].tobytes()
    # ---- the device
    pool = _pool(images)
    table = A.PasteTable(_device_items(items, pool), B, DEV)
    A.paste_prepare(table, S)
    got = A.paste_labels(table, torch.from_numpy(tg).to(DEV), occ_thr).cpu().numpy()
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))
    assert not len(bad), (bad[:5].tolist(), got[bad[:2]].tolist(), want[bad[:2]].tolist())
    # nt = 0
    got0 = A.paste_labels(table, torch.zeros((0, 10), device=DEV), occ_thr).cpu().numpy()
    assert got0.tobytes() == R.paste_labels(np.zeros((0, 10), np.float32), items, first, B, S, occ_thr).tobytes() == want[nt:].tobytes()
    # the pixels: the items outside the slots write nothing
    final = _canvases(5)
    dev = torch.from_numpy(final).to(DEV)
    A.paste_pixels(pool.buf, table, dev)
    ref_px, union, _ = R.paste_pixels(images, items, first, B, final)
    assert np.array_equal(table.bbox.cpu().numpy()[[0, n - 2, n - 1]], np.zeros((3, 4), np.int32))
    assert np.array_equal(dev.cpu().numpy(), ref_px) and np.array_equal(ref_px, R.paste_pixels(images, good, R.first_table(good, B), B, final)[0])


# ---------------------------------------------------------------------------------------------- 3. through the dataset
def _scene_labels():
    rs = np.random.RandomState(23)
    polys, labels = [], []
    for h, w in SCENE_SHAPES:
        n = 30
        q = np.stack([_rect(rs.uniform(0, w), rs.uniform(0, h), rs.uniform(6, 28), rs.uniform(5, 18), rs.uniform(0, 180), ccw=bool(k & 1))
                      for k in range(n)])
        q[3] = q[3, [0, 1, 4, 5, 2, 3, 6, 7]]                                         # a bow tie and a segment: never sources
        q[4] = q[4, [0, 1, 0, 1, 4, 5, 4, 5]]
        polys.append(q)
        labels.append(rs.choice([0, 0, 0, 0, 1, 1, 2], size=n).astype(np.float32))
    return polys, labels


CP = dict(p=0.8, max_objects=4, alpha=0.5, scale=(0.5, 1.5), rotate=180.0, occ_thr=0.4, min_side=3.0, seed=21)


def _ds(images, hyp, csl, copy_paste, augment=True, seed=5, **kw):
    from ryolov4_amd.datasets.scene_dataset import SceneDataset
    ds = SceneDataset(hyp, S, augment, csl, device=DEV, rng=(random.Random(seed), np.random.RandomState(seed)), overlap=16, rates=(1.0, 0.5),
                      keep_empty=True, window_seed=3, copy_paste=copy_paste, **kw)
    polys, labels = _scene_labels()
    ds.set_arrays(images, polys, labels)
    return ds


@pytest.fixture
def captured(monkeypatch):
    """What assemble_batch hands to finalize_batch: (canvases uint8, targets10, flags) of every batch, as host arrays."""
    from ryolov4_amd.datasets import base_dataset
    seen, real = [], base_dataset.finalize_batch

    def spy(final, targets10, flags=None, csl=False):
        seen.append((final.cpu().numpy().copy(), targets10.cpu().numpy().copy(), flags.cpu().numpy().copy()))
        return real(final, targets10, flags, csl)
    monkeypatch.setattr(base_dataset, "finalize_batch", spy)
    return seen, real


def _encode_survivors(t10):
    """The rows ryolo_encode_labels keeps: mean vertex strictly inside the canvas, in float32 as the kernel sums it."""
    q = t10[:, 2:].astype(np.float32)
    with np.errstate(invalid="ignore"):
        mx = (((q[:, 0] + q[:, 2]) + q[:, 4]) + q[:, 6]) / np.float32(4)
        my = (((q[:, 1] + q[:, 3]) + q[:, 5]) + q[:, 7]) / np.float32(4)
        return (mx > 0) & (mx < S) & (my > 0) & (my < S)


@pytest.mark.parametrize("csl", [False, True], ids=["kfiou", "csl"])
@pytest.mark.parametrize("hyp", [HYP_PLAIN, HYP_FULL], ids=["plain", "mosaic_mixup_warp_flips"])
def test_dataset_equals_the_restatement_and_its_twin_outside_the_masks(images, captured, hyp, csl):
    seen, finalize = captured
    ds, twin = _ds(images, hyp, csl, dict(CP)), _ds(images, hyp, csl, None)
    polys, labels = _scene_labels()
    scene_labels = {s: (polys[s], labels[s]) for s in range(3)}
    counts = R.class_counts(scene_labels)
    rng = random.Random(CP["seed"])                                                   # the restatement's generator lives across batches too
    kw = {k: CP[k] for k in ("p", "max_objects", "alpha", "scale", "rotate", "min_side")}
    pasted_total = buried_total = buried_pasted = 0
    for idx in ([0, 3, 8, len(ds) - 1, 5], [2, 11, 7, 7, 1]):
        got = ds.assemble_batch(idx)
        cp_final, cp_t10, cp_flags = seen[-1]
        base = twin.assemble_batch(idx)
        tw_final, tw_t10, tw_flags = seen[-1]
        assert ds.last_windows == twin.last_windows and np.array_equal(cp_flags, tw_flags)      # the assembler's draws: untouched
        drawn = R.draw(rng, B, S, R.bank_of(scene_labels, [w[1] for w in ds.last_windows]), counts, [S / ds.items[i][4] for i in idx], **kw)
        assert ds.last_pastes == [(t[0], t[1], t[2], t[5], t[6], (t[7], t[8])) for t in drawn] and twin.last_pastes == []
        items = R.items_of(drawn, SCENE_SHAPES)
        ref_final, ref_t10, union, _ = R.compose(images, items, B, tw_final, tw_t10, CP["occ_thr"])
        assert np.array_equal(cp_final, ref_final), "canvases: the restatement's composition"
        assert cp_t10.view(np.uint32).tobytes() == ref_t10.view(np.uint32).tobytes(), "targets10: the restatement's composition"
        assert np.array_equal(cp_final[~union], tw_final[~union]), "canvases outside the masks: the twin's"
        # ---- what the batch returns
        mask = union.copy()
        for b in range(B):
            if cp_flags[b] & 1:
                mask[b] = mask[b][:, ::-1]
            if cp_flags[b] & 2:
                mask[b] = mask[b][::-1, :]
        a, t = got[1].cpu().numpy(), base[1].cpu().numpy()
        outside = np.broadcast_to(~mask[:, None], a.shape)
        assert np.array_equal(a[outside], t[outside]), "images outside the masks: the twin's"
        want = finalize(torch.from_numpy(ref_final).to(DEV), torch.from_numpy(ref_t10).to(DEV), torch.from_numpy(cp_flags).to(DEV), csl)
        assert got[1].cpu().numpy().tobytes() == want[0].cpu().numpy().tobytes() and got[2].cpu().numpy().tobytes() == want[1].cpu().numpy().tobytes()
        # targets: the twin's rows minus the buried ones, in order, then the surviving pasted rows
        nt = len(tw_t10)
        ok = _encode_survivors(tw_t10)
        buried = np.isnan(ref_t10[:nt, 2:]).any(1) & ~np.isnan(tw_t10[:, 2:]).any(1)
        tw_rows, rows = base[2].cpu().numpy(), got[2].cpu().numpy()
        assert tw_rows.shape[0] == ok.sum() and tw_rows.shape[1] == (187 if csl else 7)
        first_part = tw_rows[~buried[ok]]
        n1 = len(first_part)
        assert rows[:n1].tobytes() == first_part.tobytes()
        live = _encode_survivors(ref_t10[nt:])
        assert rows.shape[0] == n1 + live.sum()
        assert rows[n1:, 0].tolist() == ref_t10[nt:][live, 0].tolist() and rows[n1:, 1].tolist() == ref_t10[nt:][live, 1].tolist()
        pasted_total += int(live.sum())
        buried_total += int(buried[ok].sum())
        buried_pasted += int(np.isnan(ref_t10[nt:, 2:]).any(1).sum())
    assert pasted_total >= 8, "objects were pasted"
    print(f"pasted rows {pasted_total}, existing rows buried {buried_total}, pasted rows buried by a later paste {buried_pasted}")
    assert buried_total >= 1, "an existing row was buried"


def test_seed_repeats_and_default_is_off(images, monkeypatch):
    from ryolov4_amd import hip
    idx = [0, 3, 8, 5, 2]
    a, b, c = _ds(images, HYP_FULL, False, dict(CP)), _ds(images, HYP_FULL, False, dict(CP)), _ds(images, HYP_FULL, False, dict(CP, seed=22))
    outs = [d.assemble_batch(idx) for d in (a, b, c)]
    assert a.last_pastes == b.last_pastes != c.last_pastes and len(a.last_pastes) >= 3
    assert outs[0][1].cpu().numpy().tobytes() == outs[1][1].cpu().numpy().tobytes() and outs[0][2].cpu().numpy().tobytes() == outs[1][2].cpu().numpy().tobytes()
    # copy_paste=None: the hook hands its arguments back and no paste kernel is called; augment=False never pastes
    calls, real = [], hip.call
    monkeypatch.setattr(hip, "call", lambda name, *args: (calls.append(name), real(name, *args))[1])
    off = _ds(images, HYP_FULL, False, None)
    f, t = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    back = off._canvas_stage(f, t, idx)
    assert back[0] is f and back[1] is t
    ref = off.assemble_batch(idx)
    assert calls and not [n for n in calls if n.startswith(("ryolo_paste_prepare", "ryolo_paste_pixels", "ryolo_paste_labels"))]
    calls.clear()
    on = _ds(images, HYP_FULL, False, dict(CP))
    got = on.assemble_batch(idx)
    assert [n for n in calls if n.startswith("ryolo_paste_")][-3:] == ["ryolo_paste_prepare", "ryolo_paste_pixels", "ryolo_paste_labels"]
    assert got[1].cpu().numpy().tobytes() != ref[1].cpu().numpy().tobytes()
    plain, plain_cp = _ds(images, HYP_FULL, False, None, augment=False), _ds(images, HYP_FULL, False, dict(CP), augment=False)
    calls.clear()
    x, y = plain.assemble_batch(idx), plain_cp.assemble_batch(idx)
    assert x[1].cpu().numpy().tobytes() == y[1].cpu().numpy().tobytes() and x[2].cpu().numpy().tobytes() == y[2].cpu().numpy().tobytes()
    assert plain_cp.last_pastes == [] and not [n for n in calls if n.startswith("ryolo_paste_p") or n == "ryolo_paste_labels"]


def test_label_table_is_unchanged_by_the_option(images):
    on, off = _ds(images, HYP_FULL, False, dict(CP)), _ds(images, HYP_FULL, False, None)
    state = on.copy_paste.rng.getstate()
    assert on.label_table().cpu().numpy().tobytes() == off.label_table().cpu().numpy().tobytes()
    on.assemble_batch([0, 1, 2, 3, 4])
    pastes = list(on.last_pastes)
    assert pastes and on.copy_paste.rng.getstate() != state
    state = on.copy_paste.rng.getstate()
    assert on.label_table(chunk=7).cpu().numpy().tobytes() == off.label_table().cpu().numpy().tobytes()
    assert on.copy_paste.rng.getstate() == state and on.last_pastes == pastes


# ---------------------------------------------------------------------------------------------- 4. the loss
def test_pasted_batch_runs_through_the_loss_without_dropped_rows(images):
    from oracle import ref_ops
    from ryolov4_amd.lib import loss as L
    from ryolov4_amd.synth import CFG, HYP

    class Model:
        anchors, nc = ref_ops.make_anchors(CFG, "kfiou"), 3

    ds = _ds(images, HYP_FULL, False, dict(CP))
    idx = [0, 3, 8, 5, 2]
    _, imgs, tg = ds.assemble_batch(idx)
    assert len(ds.last_pastes) >= 3 and tg.shape[0] > 0
    slots = tg[:, 0].cpu().numpy()
    assert (np.diff(slots) < 0).any(), "pasted rows behind the batch's rows: the targets are not grouped by slot"
    g = torch.Generator().manual_seed(9)
    outs = [torch.randn(B, 18, S // s, S // s, Model.nc + 6, generator=g).half().float().to(DEV).requires_grad_() for s in (8, 16, 32)]
    crit = L.ComputeKFIoULoss(Model, HYP)
    loss, items = crit(outs, tg)
    loss.backward()
    assert int(crit.dropped_targets) == 0
    assert bool(torch.isfinite(loss).all()) and all(bool(torch.isfinite(o.grad).all()) for o in outs)
    rows = np.concatenate([np.asarray(r)[:, 5] for r in crit.debug_matches() if len(r)])
    assert rows.max() >= tg.shape[0] - len(ds.last_pastes) and rows.max() < tg.shape[0], "pasted rows were assigned"
