"""GPU tests of full-scene detection (csrc/tiled.hip, lib/tiled.py): the window cut bit-exact against numpy and against the
paste_rects + to_tensor chain it replaces; collect + class-wise merge + final order against a numpy / oracle restatement (keep sets identical,
rows bit-equal); scenes wider than 4096 px (no class offset); end to end with a captured model against a host composition; a single window
equals post_process of the captured forward; determinism, detect_files and the DOTA Task1 writer."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle
from ryolov4_amd.synth import CFG, fill_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32


def _mods():
    from ryolov4_amd import hip
    from ryolov4_amd.datasets import augment as A
    from ryolov4_amd.lib import tiled
    return hip, A, tiled


# ------------------------------------------------------------------------------------------ host restatements
def _np_cut(img, x0, y0, S):
    """scene[y0:y0+S, x0:x0+S, ::-1] / 255 in fp32 with 114 outside -> [3, S, S]"""
    win = np.full((S, S, 3), 114, dtype=np.uint8)
    part = img[y0:y0 + S, x0:x0 + S]
    win[:part.shape[0], :part.shape[1]] = part
    return (win[:, :, ::-1].astype(f32) / f32(255)).transpose(2, 0, 1)


def _oracle_merge(windows, rates, dets, nums, mk, nc, thr, gt, max_nms, max_det):
    """fp32 shift of every window's rows, per-class oracle NMS over the max_nms best candidates (score desc, slot asc), final order
    (score desc, slot asc) capped at max_det -> rows [n, 7]."""
    rows, slots = [], []
    for w, (ri, x0, y0) in enumerate(windows):
        r = f32(rates[ri])
        for j in range(int(nums[w])):
            d = dets[w, j].astype(f32)
            rows.append(np.array([(d[0] + f32(x0)) / r, (d[1] + f32(y0)) / r, d[2] / r, d[3] / r, d[4], d[5], d[6]], dtype=f32))
            slots.append(w * mk + j)
    rows = np.array(rows, dtype=f32).reshape(-1, 7)
    slots = np.array(slots, dtype=np.int64)
    kept = []
    for c in range(nc):
        idx = np.nonzero(rows[:, 6] == c)[0]
        o = np.array(sorted(idx, key=lambda i: (-rows[i, 5], slots[i]))[:max_nms], dtype=np.int64)
        if len(o) == 0:
            continue
        b = rows[o, :5].copy()
        b[:, 4] = b[:, 4] / f32(np.pi) * f32(180.0)
        kept.extend(o[oracle.nms_rotated(b, rows[o, 5], thr, gt)])
    kept = sorted(kept, key=lambda i: (-rows[i, 5], slots[i]))[:max_det]
    return rows[np.array(kept, dtype=np.int64)]


def _device_merge(H, W, S, overlap, B, mk, nc, dets, nums, thr, gt, rates=(1.0,), max_nms=5000, max_det=5000):
    """ScenePlan fed with synthetic per-window post_process outputs (dets [T_pad, mk, 7], nums [T_pad])."""
    _, _, tiled = _mods()
    cfg = SimpleNamespace(device=torch.device(DEV), batch=B, mk=mk, nc=nc, size=S, overlap=overlap, rates=rates, max_nms=max_nms,
                          max_det=max_det)
    p = tiled.ScenePlan(cfg, H, W)
    assert dets.shape[0] == p.groups * B
    for g in range(p.groups):
        p.collect(torch.from_numpy(np.ascontiguousarray(dets[g * B:(g + 1) * B])).to(DEV),
                  torch.from_numpy(np.ascontiguousarray(nums[g * B:(g + 1) * B])).to(DEV), g)
    out, num = p.merge(thr, gt)
    n = int(num.item())
    o = out.cpu().numpy()
    assert not o[n:].any(), "rows past num are not zero"
    return o[:n], p


def _synth_dets(windows, T_pad, mk, nc, S, seed, objects=4):
    rng = np.random.RandomState(seed)
    dets = rng.uniform(-50, 50, (T_pad, mk, 7)).astype(f32)           # garbage past num / past the last window: must be ignored
    nums = rng.randint(0, mk + 1, T_pad).astype(np.int32)
    T = len(windows)
    nums[0] = 0                                                         # an empty window
    nums[min(1, T - 1)] = mk                                            # a full one
    for w in range(T_pad):
        n = int(nums[w])
        dets[w, :n, 0:2] = rng.uniform(0, S, (n, 2))
        dets[w, :n, 2:4] = rng.uniform(4, 40, (n, 2))
        dets[w, :n, 4] = rng.uniform(-np.pi / 2, np.pi / 2, n)
        dets[w, :n, 5] = np.round(rng.uniform(0.1, 1.0, n) * 16) / 16     # exact score ties
        dets[w, :n, 6] = rng.randint(0, nc, n)
    # the same objects seen by every window that contains them, with nearby scores
    for k in range(objects):
        X, Y = rng.uniform(S * 0.6, S * 1.2, 2)
        c = rng.randint(0, nc)
        for w, (ri, x0, y0) in enumerate(windows):
            if ri == 0 and nums[w] > 0 and x0 <= X < x0 + S and y0 <= Y < y0 + S:
                j = rng.randint(0, nums[w])
                dets[w, j] = [X - x0, Y - y0, 30, 18, 0.3, 0.7 + 0.002 * w, c]
    return dets, nums


# ------------------------------------------------------------------------------------------ 1. cut
def test_cut_bit_exact_vs_numpy_and_paste_chain():
    hip, A, tiled = _mods()
    S, B = 128, 5
    rng = np.random.RandomState(0)
    for (H, W) in ((250, 302), (90, 101)):
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        off = 7                                                         # odd byte offset in the pool: unaligned source rows
        pool = torch.zeros(off + H * W * 3 + 64, dtype=torch.uint8, device=DEV)
        pool[off:off + H * W * 3] = torch.from_numpy(img.reshape(-1)).to(DEV)
        wins = [(x0, y0) for _, x0, y0 in tiled.tile_plan(H, W, S, 32)]
        wins += [(max(0, W - 100), max(0, H - 100)), (W - 3, 0), (0, H - 1)]     # windows that cross the right / bottom edges
        table = torch.tensor([[off, H, W, x0, y0, 0] for x0, y0 in wins], dtype=torch.int64, device=DEV)      # view code 0: id
        for w0 in range(0, len(wins), B):
            n = min(B, len(wins) - w0)                                   # 12 and 4 windows: the last group is partial
            dst = torch.full((B, 3, S, S), -3.0, dtype=torch.float32, device=DEV)
            hip.call("ryolo_tile_cut_views", hip.ptr(pool), hip.ptr(table), w0, n, S, hip.ptr(dst), hip.stream())
            got = dst.cpu().numpy()
            for k in range(n):
                x0, y0 = wins[w0 + k]
                assert np.array_equal(got[k].view(np.uint32), _np_cut(img, x0, y0, S).view(np.uint32)), (H, W, x0, y0)
            assert (got[n:] == -3.0).all(), "slots past the group's windows were touched"
            # the chain the cut replaces: paste onto a 114 canvas, then to_tensor
            rects = [(off, W, A.Placed(x0, y0, 0, 0, min(S, W - x0), min(S, H - y0)), k) for k, (x0, y0) in enumerate(wins[w0:w0 + n])]
            canvas = A.paste(pool, rects, n, S, S, fill=114)
            ref = torch.empty((n, 3, S, S), dtype=torch.float32, device=DEV)
            hip.call("ryolo_to_tensor", hip.ptr(canvas), n, S, S, None, hip.ptr(ref), hip.stream())
            assert torch.equal(dst[:n].view(torch.int32), ref.view(torch.int32))


# ------------------------------------------------------------------------------------------ 2. collect + merge
@pytest.mark.parametrize("nc", [1, 3, 16])
@pytest.mark.parametrize("gt", [True, False])
def test_collect_merge_vs_oracle(nc, gt):
    _, _, tiled = _mods()
    H, W, S, ov, B, mk = 250, 300, 128, 32, 4, 24
    for rates, max_nms, max_det, seed in (((1.0,), 5000, 5000, nc), ((1.0, 0.5), 5000, 5000, nc + 1), ((1.0,), 9, 13, nc + 2)):
        windows = tiled.tile_plan(H, W, S, ov, rates)
        T_pad = -(-len(windows) // B) * B
        dets, nums = _synth_dets(windows, T_pad, mk, nc, S, seed)
        got, p = _device_merge(H, W, S, ov, B, mk, nc, dets, nums, 0.3, gt, rates, max_nms, max_det)
        exp = _oracle_merge(windows, rates, dets, nums, mk, nc, 0.3, gt, max_nms, max_det)
        assert got.shape == exp.shape, (rates, max_nms, got.shape, exp.shape)
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (rates, max_nms)
        assert len(exp) > 0


def test_merge_all_windows_empty():
    _, _, tiled = _mods()
    windows = tiled.tile_plan(200, 200, 128, 0)
    dets = np.ones((4, 8, 7), dtype=f32)
    got, _ = _device_merge(200, 200, 128, 0, 4, 8, 3, dets, np.zeros(4, np.int32), 0.3, True)
    assert got.shape == (0, 7) and len(windows) == 4


# ------------------------------------------------------------------------------------------ 3. scenes wider than 4096 px
def test_scene_wider_than_4096_keeps_classes_apart():
    _, _, tiled = _mods()
    H, W, S, B, mk, nc = 128, 8400, 128, 8, 2, 2
    windows = tiled.tile_plan(H, W, S, 0)
    T_pad = -(-len(windows) // B) * B
    dets = np.zeros((T_pad, mk, 7), dtype=f32)
    nums = np.zeros(T_pad, dtype=np.int32)

    def put(X, score, c):
        w = next(i for i, (_, x0, _) in enumerate(windows) if x0 <= X < x0 + S)
        dets[w, nums[w]] = [X - windows[w][1], 64, 40, 20, 0.0, score, c]
        nums[w] += 1

    put(4500, 0.9, 0)            # class 0 at x = 4500
    put(404, 0.8, 1)             # class 1 at x = 404: lands exactly on the first box under post_process's cls * 4096 offset
    put(6010, 0.7, 0)            # two overlapping class-0 boxes in neighbouring windows near x = 6000: merged
    put(6020, 0.6, 0)
    assert 404 + 4096 == 4500
    got, _ = _device_merge(H, W, S, 0, B, mk, nc, dets, nums, 0.3, True)
    assert got[:, [0, 5, 6]].tolist() == [[4500, f32(0.9), 0], [404, f32(0.8), 1], [6010, f32(0.7), 0]]
    exp = _oracle_merge(windows, (1.0,), dets, nums, mk, nc, 0.3, True, 5000, 5000)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))


# ------------------------------------------------------------------------------------------ 4-6. with a captured model
def _model(nc):
    from ryolov4_amd.model.yolo import Yolo
    net = Yolo(nc, CFG, "kfiou", "yolov5")
    net.load_state_dict(fill_state(net.state_dict()))
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def det3():
    _, _, tiled = _mods()
    return tiled.TiledDetector(_model(3), size=256, overlap=64, batch=4, conf_thres=0.05, iou_thres=0.4, max_nms=1500)


def _host_composition(det, img, rates, gt=True):
    """numpy cut (resized copies from the existing resize kernels), the detector's own captured graph, host shift + per-class oracle NMS."""
    _, A, tiled = _mods()
    H, W = img.shape[:2]
    srcs = []
    for r in rates:
        if r == 1.0:
            srcs.append(img)
            continue
        h, w = tiled.resized_extent(H, W, r)
        pool = A.ImagePool([img], DEV)
        stage, offs = A.resize_hsv_batch(pool, [(0, (h, w), A.INTERP_AREA if r < 1 else A.INTERP_LINEAR, -1)])
        srcs.append(stage[offs[0]:offs[0] + h * w * 3].cpu().numpy().reshape(h, w, 3))
    windows = tiled.tile_plan(H, W, det.size, det.overlap, rates)
    B, S, mk = det.batch, det.size, det.mk
    T_pad = -(-len(windows) // B) * B
    dets = np.zeros((T_pad, mk, 7), dtype=f32)
    nums = np.zeros(T_pad, dtype=np.int32)
    for g in range(T_pad // B):
        imgs = np.zeros((B, 3, S, S), dtype=f32)
        for k, (ri, x0, y0) in enumerate(windows[g * B:(g + 1) * B]):
            imgs[k] = _np_cut(srcs[ri], x0, y0, S)
        _, _, d, n = det.run(torch.from_numpy(imgs).to(DEV))
        dets[g * B:(g + 1) * B], nums[g * B:(g + 1) * B] = d.cpu().numpy(), n.cpu().numpy()
    nums[len(windows):] = 0
    return _oracle_merge(windows, rates, dets, nums, mk, det.nc, det.merge_iou, gt, det.max_nms, det.max_det)


def test_end_to_end_vs_host_composition(det3):
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, (520, 700, 3)).astype(np.uint8)
    got = det3(img).cpu().numpy()
    exp = _host_composition(det3, img, (1.0,))
    assert len(exp) > 0
    assert got.shape == exp.shape and np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    # two rates: rates select the scene plan only (window table, resized copies), the captured graph is the same
    det3.rates = (1.0, 0.5)
    try:
        got2 = det3(torch.from_numpy(img).to(DEV)).cpu().numpy()
        exp2 = _host_composition(det3, img, (1.0, 0.5))
    finally:
        det3.rates = (1.0,)
    assert got2.shape == exp2.shape and np.array_equal(got2.view(np.uint32), exp2.view(np.uint32))


def test_single_window_equals_post_process():
    _, _, tiled = _mods()
    det = tiled.TiledDetector(_model(1), size=256, overlap=64, batch=2, conf_thres=0.05, iou_thres=0.4)
    img = np.random.RandomState(5).randint(0, 256, (256, 256, 3)).astype(np.uint8)
    got = det(img).cpu().numpy()
    imgs = np.zeros((2, 3, 256, 256), dtype=f32)
    imgs[0] = _np_cut(img, 0, 0, 256)
    _, _, d, n = det.run(torch.from_numpy(imgs).to(DEV))
    exp = d[0, :int(n[0].item())].cpu().numpy()
    assert len(exp) > 0
    assert got.shape == exp.shape and np.array_equal(got.view(np.uint32), exp.view(np.uint32))


def test_determinism_detect_files_and_task1(det3, tmp_path):
    _, _, tiled = _mods()
    rng = np.random.RandomState(9)
    scenes = {"a": rng.randint(0, 256, (300, 400, 3)).astype(np.uint8), "b": rng.randint(0, 256, (300, 400, 3)).astype(np.uint8),
              "c": rng.randint(0, 256, (200, 500, 3)).astype(np.uint8)}
    one = det3(scenes["a"])
    assert torch.equal(one.view(torch.int32), det3(scenes["a"]).view(torch.int32))
    sep = {k: det3(v) for k, v in scenes.items()}
    for overlap in (True, False):
        streamed = dict(det3.detect_files(list(scenes), imread=scenes.__getitem__, overlap=overlap))
        assert list(streamed) == list(scenes)
        for k in scenes:
            assert torch.equal(streamed[k].view(torch.int32), sep[k].view(torch.int32)), (k, overlap)
    # DOTA Task1 lines, checked by hand: theta = 0 -> vertices (x -+ h/2, y -+ w/2)
    d = torch.tensor([[10, 20, 4, 8, 0, 0.5, 1], [100, 50, 2, 6, 0, 0.25, 0], [1, 2, 2, 2, 0, 0.75, 1]], dtype=torch.float32, device=DEV)
    files = tiled.write_dota_task1({"P0001": d, "P0002": d[:0]}, str(tmp_path), ["plane", "ship", "tank"])
    assert [os.path.basename(f) for f in files] == ["Task1_plane.txt", "Task1_ship.txt", "Task1_tank.txt"]
    txt = [open(f).read() for f in files]
    assert txt[0] == "P0001 0.250000 97.0 49.0 103.0 49.0 103.0 51.0 97.0 51.0\n"
    assert txt[1] == ("P0001 0.500000 6.0 18.0 14.0 18.0 14.0 22.0 6.0 22.0\n"
                      "P0001 0.750000 0.0 1.0 2.0 1.0 2.0 3.0 0.0 3.0\n")
    assert txt[2] == ""
