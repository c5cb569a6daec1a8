"""GPU tests of the flip / 90-degree views of full-scene detection (csrc/tiled.hip ryolo_tile_cut_views / ryolo_tile_collect_views,
lib/tiled.py TiledDetector(views=...)).  Everything is compared on the bits with the host restatements of tests/views_ref.py (checked
against each other and against the oracle's polygons in tests/test_tiled_views_cpu.py): the cut in every view, the collect pass, the
class-wise merge over windows x views against the oracle NMS, the whole detector against a host composition around its own captured
graph, and — independent of the cut restatement — the equivariance of the whole path under a transformed scene."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ryolov4_amd.synth import CFG, fill_state
from tests import views_ref as V
from tests.test_gpu_tiled import _np_cut

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32


def _mods():
    from ryolov4_amd import hip
    from ryolov4_amd.datasets import augment as A
    from ryolov4_amd.lib import tiled
    return hip, A, tiled


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ------------------------------------------------------------------------------------------ 1. cut
# S = 128: whole 32 x 32 LDS tiles; S = 96 and S = 100: the kernel's tile is 32 px, so 100 (a multiple of 4 only) leaves a partial tile
# in both directions, 96 is the size a 64 px tile would leave partial.
@pytest.mark.parametrize("S", [128, 96, 100])
def test_cut_views_bit_exact(S):
    hip, _, tiled = _mods()
    B = 7
    rng = np.random.RandomState(S)
    for (H, W) in ((250, 302), (90, 101)):
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
        off = 7                                                         # odd byte offset in the pool: unaligned source rows
        pool = torch.zeros(off + H * W * 3 + 64, dtype=torch.uint8, device=DEV)
        pool[off:off + H * W * 3] = torch.from_numpy(img.reshape(-1)).to(DEV)
        wins = [(x0, y0) for _, x0, y0 in tiled.tile_plan(H, W, S if S % 32 == 0 else 128, 32)]
        wins += [(max(0, W - 100), max(0, H - 100)), (W - 3, 0), (0, H - 1)]     # windows that cross the right / bottom edges
        wins += [(W + 5, H + 9)]                                                # wholly in the fill
        ents = [(x0, y0, v) for x0, y0 in wins for v in range(8)]               # all eight views of a window back to back: every group
        assert len(ents) % B != 0                                               # of 7 mixes views, and the last group is partial
        table = torch.tensor([[off, H, W, x0, y0, v] for x0, y0, v in ents], dtype=torch.int64, device=DEV)
        exp = {}
        for e0 in range(0, len(ents), B):
            n = min(B, len(ents) - e0)
            dst = torch.full((B, 3, S, S), -3.0, dtype=torch.float32, device=DEV)
            hip.call("ryolo_tile_cut_views", hip.ptr(pool), hip.ptr(table), e0, n, S, hip.ptr(dst), hip.stream())
            got = dst.cpu().numpy()
            for k in range(n):
                x0, y0, v = ents[e0 + k]
                if (x0, y0, v) not in exp:
                    exp[(x0, y0, v)] = V.np_cut_view(img, x0, y0, S, V.NAMES[v])
                assert np.array_equal(_bits(got[k]), _bits(exp[(x0, y0, v)])), (S, H, W, x0, y0, V.NAMES[v])
                if v == 0:                                                      # a restatement that shares nothing with views_ref
                    assert np.array_equal(_bits(got[k]), _bits(_np_cut(img, x0, y0, S))), "view id differs from the plain crop"
            assert (got[n:] == -3.0).all(), "slots past the group's entries were touched"
        fill = V.np_cut_view(img, W + 5, H + 9, S, "rot90")
        assert (fill == f32(114) / f32(255)).all()


def test_cut_views_rejects_bad_arguments():
    hip, _, _ = _mods()
    pool = torch.zeros(64, dtype=torch.uint8, device=DEV)
    table = torch.zeros((1, 6), dtype=torch.int64, device=DEV)
    dst = torch.zeros((1, 3, 8, 8), dtype=torch.float32, device=DEV)
    for args in ((0, 1, 6), (0, -1, 8), (-1, 1, 8), (0, 1, 0)):
        with pytest.raises(RuntimeError):
            hip.call("ryolo_tile_cut_views", hip.ptr(pool), hip.ptr(table), args[0], args[1], args[2], hip.ptr(dst), hip.stream())
    with pytest.raises(RuntimeError):
        hip.call("ryolo_tile_cut_views", None, hip.ptr(table), 0, 1, 8, hip.ptr(dst), hip.stream())


# ------------------------------------------------------------------------------------------ 2. collect
def _synth_dets(entries, E_pad, mk, nc, S, seed, objects=4):
    """post_process-like rows per entry: theta over everything kfiou decode can produce (|theta| < pi/2 + 0.27) with the exact values
    +-(float)pi/2 and 0, score ties, garbage past num and past the last entry, and objects seen by every entry whose window holds them
    (placed in the entry's view by the forward map of a point: rot180 and the flips are their own inverses, so only plain windows of view
    id are used for those; the merge test needs overlaps, not a particular geometry)."""
    rng = np.random.RandomState(seed)
    dets = rng.uniform(-50, 50, (E_pad, mk, 7)).astype(f32)
    nums = rng.randint(0, mk + 1, E_pad).astype(np.int32)
    nums[0] = 0
    nums[min(1, len(entries) - 1)] = mk
    for e in range(E_pad):
        n = int(nums[e])
        dets[e, :n, 0:2] = rng.uniform(0, S, (n, 2))
        dets[e, :n, 2:4] = rng.uniform(4, 40, (n, 2))
        dets[e, :n, 4] = rng.uniform(-np.pi / 2 - 0.26, np.pi / 2 + 0.26, n)
        dets[e, :n, 5] = np.round(rng.uniform(0.1, 1.0, n) * 16) / 16
        dets[e, :n, 6] = rng.randint(0, nc, n)
        for j, t in zip(range(n), (V.HALF_PI, -V.HALF_PI, f32(0))):
            if rng.rand() < 0.5:
                dets[e, j, 4] = t
    for k in range(objects):
        X, Y = rng.uniform(S * 0.6, S * 1.2, 2)
        c = rng.randint(0, nc)
        for e, (ri, x0, y0, name) in enumerate(entries):
            if ri == 0 and name in ("id", "rot180", "hflip", "vflip") and nums[e] > 0 and x0 <= X < x0 + S and y0 <= Y < y0 + S:
                vx, vy = V.point_map(name, X - x0, Y - y0, float(S))            # these four maps are involutions
                j = rng.randint(0, nums[e])
                dets[e, j] = [vx, vy, 30, 18, 0.3 if name in ("id", "rot180") else -0.3, 0.7 + 0.002 * e, c]
    return dets, nums


def _plan(tiled, H, W, S, ov, B, mk, nc, rates, views, max_nms=5000, max_det=5000):
    cfg = SimpleNamespace(device=torch.device(DEV), batch=B, mk=mk, nc=nc, size=S, overlap=ov, rates=rates, max_nms=max_nms, max_det=max_det,
                          views=views)
    return tiled.ScenePlan(cfg, H, W)


def _feed(p, dets, nums):
    B = p.batch
    assert dets.shape[0] == p.groups * B
    for g in range(p.groups):
        p.collect(torch.from_numpy(np.ascontiguousarray(dets[g * B:(g + 1) * B])).to(DEV),
                  torch.from_numpy(np.ascontiguousarray(nums[g * B:(g + 1) * B])).to(DEV), g)


@pytest.mark.parametrize("nc", [1, 3])
def test_collect_views_bit_exact(nc):
    _, _, tiled = _mods()
    H, W, S, ov, B, mk, rates = 250, 300, 128, 32, 5, 24, (1.0, 0.5)
    entries = tiled.tile_entries(H, W, S, ov, rates, tiled.VIEWS)
    E = len(entries)
    E_pad = -(-E // B) * B
    assert E_pad > E, "the last group must be partial"
    dets, nums = _synth_dets(entries, E_pad, mk, nc, S, 20 + nc)
    p = _plan(tiled, H, W, S, ov, B, mk, nc, rates, tiled.VIEWS)
    assert p.T == E and p.ld == E_pad * mk
    for t in (p.cand, p.key, p.fkey):
        t.fill_(7.0)                                                    # every slot must be written
    _feed(p, dets, nums)
    cand, key, fkey = p.cand.cpu().numpy(), p.key.cpu().numpy(), p.fkey.cpu().numpy()
    ecand = np.zeros((E_pad * mk, 7), dtype=f32)
    ekey = np.full((nc, E_pad * mk), -np.inf, dtype=f32)
    gap, mapped = 0.0, []
    for e, (ri, x0, y0, name) in enumerate(entries):
        n = int(nums[e])
        m = V.map_rows(dets[e, :n], name, S)
        ecand[e * mk:e * mk + n] = V.shift_rows(m, x0, y0, rates[ri])
        ekey[dets[e, :n, 6].astype(np.int64), e * mk + np.arange(n)] = dets[e, :n, 5]
        gap = max(gap, V.polygon_gap(dets[e, :n], name, S))
        if name not in ("id", "rot180"):
            mapped.append(m[:, 4])
        else:
            assert np.array_equal(_bits(m[:, 4]), _bits(dets[e, :n, 4]))
    assert np.array_equal(_bits(cand), _bits(ecand))
    assert np.array_equal(_bits(key), _bits(ekey))
    assert (fkey == -np.inf).all()
    mapped = np.concatenate(mapped)
    assert len(mapped) > 100 and (mapped >= -V.HALF_PI).all() and (mapped < V.HALF_PI).all()
    assert gap < 1e-2, gap
    # views=("id",): the plain host shift, written out here without map_rows, on the bits; theta untouched
    ids = tiled.tile_entries(H, W, S, ov, rates, ("id",))
    pv = _plan(tiled, H, W, S, ov, B, mk, nc, rates, ("id",))
    n_id = pv.groups * B
    assert pv.T == len(ids) and n_id > len(ids), "the last group must be partial"
    for t in (pv.cand, pv.key, pv.fkey):
        t.fill_(7.0)
    _feed(pv, dets[:n_id], nums[:n_id])
    cand, key, fkey = pv.cand.cpu().numpy(), pv.key.cpu().numpy(), pv.fkey.cpu().numpy()
    ecand = np.zeros((n_id * mk, 7), dtype=f32)
    ekey = np.full((nc, n_id * mk), -np.inf, dtype=f32)
    for e, (ri, x0, y0, name) in enumerate(ids):
        assert name == "id"
        n, r = int(nums[e]), f32(rates[ri])
        d = dets[e, :n]
        ecand[e * mk:e * mk + n] = np.stack([(d[:, 0] + f32(x0)) / r, (d[:, 1] + f32(y0)) / r, d[:, 2] / r, d[:, 3] / r, d[:, 4], d[:, 5], d[:, 6]], 1)
        ekey[d[:, 6].astype(np.int64), e * mk + np.arange(n)] = d[:, 5]
        assert np.array_equal(_bits(cand[e * mk:e * mk + n, 4]), _bits(d[:, 4])), "view id changed theta's bits"
    assert ecand.dtype == f32
    assert np.array_equal(_bits(cand), _bits(ecand))
    assert np.array_equal(_bits(key), _bits(ekey))
    assert (fkey == -np.inf).all()


# ------------------------------------------------------------------------------------------ 3. merge over views
@pytest.mark.parametrize("gt", [True, False])
def test_merge_over_views_vs_oracle(gt):
    _, _, tiled = _mods()
    H, W, S, ov, B, mk, nc = 250, 300, 128, 32, 4, 24, 3
    for rates, views, max_nms, max_det, seed in (((1.0,), tiled.VIEWS, 5000, 5000, 1), ((1.0, 0.5), ("rot270", "id", "hflip"), 5000, 5000, 2),
                                                  ((1.0,), tiled.VIEWS, 9, 13, 3)):
        entries = tiled.tile_entries(H, W, S, ov, rates, views)
        E_pad = -(-len(entries) // B) * B
        dets, nums = _synth_dets(entries, E_pad, mk, nc, S, seed)
        p = _plan(tiled, H, W, S, ov, B, mk, nc, rates, views, max_nms, max_det)
        _feed(p, dets, nums)
        out, num = p.merge(0.3, gt)
        n = int(num.item())
        o = out.cpu().numpy()
        assert not o[n:].any(), "rows past num are not zero"
        exp = V.oracle_merge(entries, rates, S, dets, nums, mk, nc, 0.3, gt, max_nms, max_det)
        assert len(exp) > 0
        assert o[:n].shape == exp.shape, (views, max_nms, o[:n].shape, exp.shape)
        assert np.array_equal(_bits(o[:n]), _bits(exp)), (views, max_nms)
        if max_det == 13:
            assert len(exp) == 13


# ------------------------------------------------------------------------------------------ 4-6. with a captured model
def _model(nc):
    from ryolov4_amd.model.yolo import Yolo
    net = Yolo(nc, CFG, "kfiou", "yolov5")
    net.load_state_dict(fill_state(net.state_dict()))
    return net.to(DEV).eval()


@pytest.fixture(scope="module")
def det3():
    """Built WITHOUT the views argument; tests select views through the attribute (views pick the scene plan only: the captured graph is
    the same), as the existing tests do with rates."""
    _, _, tiled = _mods()
    return tiled.TiledDetector(_model(3), size=256, overlap=64, batch=4, conf_thres=0.05, iou_thres=0.4, max_nms=1500)


class _with:
    def __init__(self, det, **kw):
        self.det, self.kw = det, kw

    def __enter__(self):
        self.old = {k: getattr(self.det, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(self.det, k, v)
        return self.det

    def __exit__(self, *exc):
        for k, v in self.old.items():
            setattr(self.det, k, v)


def _host_composition(det, img, rates, views, gt=True):
    """numpy cut + view (resized copies from the existing resize kernels), the detector's own captured graph, the numpy inverse map and
    shift, per-class oracle NMS."""
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
    entries = tiled.tile_entries(H, W, det.size, det.overlap, rates, views)
    B, S, mk = det.batch, det.size, det.mk
    E_pad = -(-len(entries) // B) * B
    dets = np.zeros((E_pad, mk, 7), dtype=f32)
    nums = np.zeros(E_pad, dtype=np.int32)
    for g in range(E_pad // B):
        imgs = np.zeros((B, 3, S, S), dtype=f32)
        for k, (ri, x0, y0, name) in enumerate(entries[g * B:(g + 1) * B]):
            imgs[k] = V.np_cut_view(srcs[ri], x0, y0, S, name)
        _, _, d, n = det.run(torch.from_numpy(imgs).to(DEV))
        dets[g * B:(g + 1) * B], nums[g * B:(g + 1) * B] = d.cpu().numpy(), n.cpu().numpy()
    nums[len(entries):] = 0
    return V.oracle_merge(entries, rates, S, dets, nums, mk, det.nc, det.merge_iou, gt, det.max_nms, det.max_det)


@pytest.mark.parametrize("rates,views", [((1.0,), ("id", "hflip", "rot90")), ((1.0, 0.5), V.NAMES)])
def test_end_to_end_vs_host_composition(det3, rates, views):
    img = np.random.RandomState(3).randint(0, 256, (520, 700, 3)).astype(np.uint8)
    with _with(det3, rates=rates, views=views):
        got = det3(img).cpu().numpy()
        exp = _host_composition(det3, img, rates, views)
    assert len(exp) > 0
    assert got.shape == exp.shape and np.array_equal(_bits(got), _bits(exp))


@pytest.mark.parametrize("name", V.NAMES[1:])
def test_equivariance_of_the_whole_path(det3, name):
    """views=(v,) on X = the inverse map, row by row, of views=("id",) on view(X, v): the device cut in view v must produce what the plain
    cut produces from the host-transformed scene, and the collect map must be the map applied afterwards.  A 256 x 256 scene is one window
    at (0, 0) and rate 1, so the shift changes no bit."""
    S = det3.size
    X = np.random.RandomState(11).randint(0, 256, (S, S, 3)).astype(np.uint8)
    with _with(det3, views=(name,)):
        got = det3(X).cpu().numpy()
    plain = det3(np.ascontiguousarray(V.view_pixels(X, name))).cpu().numpy()
    assert len(plain) > 0
    exp = V.map_rows(plain, name, S)
    assert got.shape == exp.shape and np.array_equal(_bits(got), _bits(exp)), name


def test_default_unchanged_determinism_and_detect_files(det3):
    _, _, tiled = _mods()
    rng = np.random.RandomState(9)
    scenes = {"a": rng.randint(0, 256, (300, 400, 3)).astype(np.uint8), "b": rng.randint(0, 256, (300, 400, 3)).astype(np.uint8),
              "c": rng.randint(0, 256, (200, 500, 3)).astype(np.uint8)}
    dv = tiled.TiledDetector(_model(3), size=256, overlap=64, batch=4, conf_thres=0.05, iou_thres=0.4, max_nms=1500, views=("id",))
    assert dv.views == ("id",) and det3.views == ("id",)
    for k, s in scenes.items():
        a, b = det3(s), dv(s)
        assert len(a) > 0 and torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    with _with(dv, views=tiled.VIEWS):
        one = dv(scenes["a"])
        assert len(one) > 0 and torch.equal(one.view(torch.int32), dv(scenes["a"]).view(torch.int32))
        sep = {k: dv(v) for k, v in scenes.items()}
        assert torch.equal(sep["a"].view(torch.int32), one.view(torch.int32))
        for overlap in (True, False):
            streamed = dict(dv.detect_files(list(scenes), imread=scenes.__getitem__, overlap=overlap))
            assert list(streamed) == list(scenes)
            for k in scenes:
                assert torch.equal(streamed[k].view(torch.int32), sep[k].view(torch.int32)), (k, overlap)
