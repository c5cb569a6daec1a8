"""GPU tests of the cluster fusion of the full-scene merge (csrc/nms.hip ryolo_nms_owner, csrc/tiled.hip ryolo_tile_fuse, lib/tiled.py
fuse="box" | "wbf").  Everything is compared on the bits with the host restatement tests/fusion_ref.py (checked on the CPU in
tests/test_tiled_fusion_cpu.py): the fused merge over the synthetic scenes of the views tests, the owners against the greedy pass over
the oracle's mask, the invariants of "box" against the unfused merge on the same fed plan, the unchanged default, and the whole detector
against a host composition around its own captured graph."""
import numpy as np
import pytest
import torch

from ryolov4_amd.synth import synth_nms_boxes
from tests import fusion_ref as F
from tests import views_ref as V
from tests.test_gpu_tiled_views import _bits, _feed, _host_composition, _model, _plan, _synth_dets, _with  # noqa: F401  (_synth_dets: through F.scene)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32


def _mods():
    from ryolov4_amd import hip
    from ryolov4_amd.datasets import augment as A
    from ryolov4_amd.lib import tiled
    return hip, A, tiled


def _fed_plan(i):
    _, _, tiled = _mods()
    nc, rates, views, seed, thr, max_nms, max_det = F.CONFIGS[i]
    entries, dets, nums = F.scene(i)
    p = _plan(tiled, F.SH, F.SW, F.S, F.OV, F.B, F.MK, nc, rates, views, max_nms, max_det)
    assert p.n_ens == len(rates) * len(views)
    _feed(p, dets, nums)
    return p


def _result(p, thr, gt, fuse):
    out, num = p.merge(thr, gt, fuse)
    n = int(num.item())
    o = out.cpu().numpy()
    assert not o[n:].any(), "rows past num are not zero"
    return o[:n]


# ------------------------------------------------------------------------------------------ 1. the fused merge on the bits
@pytest.mark.parametrize("gt", [True, False])
@pytest.mark.parametrize("i", range(len(F.CONFIGS)))
def test_fused_merge_vs_host_restatement(i, gt):
    nc, rates, views, seed, thr, max_nms, max_det = F.CONFIGS[i]
    entries, dets, nums = F.scene(i)
    p = _fed_plan(i)
    cand = p.cand.clone()
    for mode in F.MODES:
        st = {}
        exp = F.fused_merge(entries, rates, F.S, dets, nums, F.MK, nc, thr, gt, max_nms, max_det, mode, stats=st)
        sizes = np.array(st["sizes"])
        print(f"config {i} gt {gt} {mode}: rows {len(exp)} clusters>=2 {(sizes >= 2).sum()} >=3 {(sizes >= 3).sum()} largest {sizes.max()} "
              f"wraps {st.get('wraps', 0)} swaps {st.get('swaps', 0)} per class {st['per_class']}")
        if max_det == 13:
            assert len(exp) == 13 and max(st["per_class"]) == 9              # candidates beyond max_nms per class contribute to nothing
        else:                                                                 # floors: the comparison below must not go vacuous
            assert (sizes >= 2).sum() >= 30 and (sizes >= 3).sum() >= 5 and st.get("wraps", 0) >= 5 and st.get("swaps", 0) >= 10
        if nc == 1:
            assert st["per_class"][0] > 128                                   # owners and members cross more than two mask words
        got = _result(p, thr, gt, mode)
        assert got.shape == exp.shape, (mode, got.shape, exp.shape)
        assert np.array_equal(_bits(got), _bits(exp)), (mode, np.nonzero((_bits(got) != _bits(exp)).any(1))[0][:8])
    assert torch.equal(p.cand.view(torch.int32), cand.view(torch.int32)), "the candidates were modified"


# ------------------------------------------------------------------------------------------ 2. owners alone
def _nms_and_owner(boxes, counts, thr, gt):
    """boxes [batch, nmax, 5] (score-descending rows), counts [batch] -> (keep, num_keep, owner) as numpy, through the two entry points."""
    hip, _, _ = _mods()
    batch, nmax = boxes.shape[:2]
    need = hip._Z()
    hip.call("ryolo_nms_workspace_bytes", batch, nmax, need)
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    b = torch.from_numpy(boxes).to(DEV)
    cnt = torch.from_numpy(np.asarray(counts, dtype=np.int32)).to(DEV)
    keep = torch.full((batch, nmax), -7, dtype=torch.int64, device=DEV)
    nkeep = torch.full((batch,), -7, dtype=torch.int32, device=DEV)
    owner = torch.full((batch, nmax), -7, dtype=torch.int32, device=DEV)
    hip.call("ryolo_nms_rotated_batched", hip.ptr(b), hip.ptr(cnt), batch, nmax, thr, 1 if gt else 0, nmax, hip.ptr(ws), ws.numel(), hip.ptr(keep),
             nmax, hip.ptr(nkeep), hip.stream())
    hip.call("ryolo_nms_owner", hip.ptr(cnt), batch, nmax, hip.ptr(ws), ws.numel(), hip.ptr(keep), nmax, hip.ptr(nkeep), hip.ptr(owner), hip.stream())
    return keep.cpu().numpy(), nkeep.cpu().numpy(), owner.cpu().numpy()


@pytest.mark.parametrize("gt", [True, False])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 130, 700])
def test_owner_vs_greedy_pass_over_the_oracle_mask(N, gt):
    """Clustered boxes (about twenty per site: most are suppressed, many by a kept row several mask words back); three rows of unequal
    counts, one of them empty where N allows it or not."""
    import oracle
    thr = 0.2
    counts = [N, 0 if N in (1, 130) else (2 * N + 2) // 3, N // 2]
    boxes = np.zeros((3, N, 5), dtype=f32)
    for b in range(3):
        bx, _ = synth_nms_boxes(N, "C", seed=10 * N + b, ncls=1)
        boxes[b] = bx
        boxes[b, counts[b]:] = 0                                               # rows past the count must not matter
    keep, nkeep, owner = _nms_and_owner(boxes, counts, thr, gt)
    moved = 0
    for b in range(3):
        n = counts[b]
        exp_owner, exp_keep = F.owners_from_mask(oracle.nms_mask(boxes[b, :n], thr, gt), n)
        assert nkeep[b] == len(exp_keep) and np.array_equal(keep[b, :nkeep[b]], exp_keep)
        assert np.array_equal(owner[b, :n], exp_owner), (b, np.nonzero(owner[b, :n] != exp_owner)[0][:8])
        assert (owner[b, n:] == -1).all()
        assert np.array_equal(np.nonzero(owner[b, :n] == np.arange(n))[0], exp_keep)        # owner[k] == k exactly on the keep set
        moved += int((exp_owner != np.arange(n)).sum())
    if N >= 63:
        assert moved > N // 2, "the boxes did not cluster: nothing to own"


def test_owner_rejects_bad_arguments():
    hip, _, _ = _mods()
    batch, nmax = 2, 70
    need = hip._Z()
    hip.call("ryolo_nms_workspace_bytes", batch, nmax, need)
    ws = torch.zeros(need.value, dtype=torch.uint8, device=DEV)
    keep = torch.zeros((batch, nmax), dtype=torch.int64, device=DEV)
    nkeep = torch.zeros(batch, dtype=torch.int32, device=DEV)
    owner = torch.zeros((batch, nmax), dtype=torch.int32, device=DEV)
    good = [None, batch, nmax, hip.ptr(ws), ws.numel(), hip.ptr(keep), nmax, hip.ptr(nkeep), hip.ptr(owner), hip.stream()]
    hip.call("ryolo_nms_owner", *good)                                          # counts may be NULL; an empty keep list owns nothing
    assert (owner == torch.arange(nmax, device=DEV, dtype=torch.int32)).sum() == 0 and (owner == -1).all()
    ARG, WORKSPACE = "ryolo_nms_owner failed: invalid argument$", "ryolo_nms_owner failed: workspace too small$"      # hip.call names the status
    for at, bad, err in ((3, None, ARG), (5, None, ARG), (7, None, ARG), (8, None, ARG), (1, -1, ARG), (2, -1, ARG), (6, 0, ARG),
                         (4, need.value - 1, WORKSPACE), (4, 0, WORKSPACE)):
        args = list(good)
        args[at] = bad
        with pytest.raises(RuntimeError, match=err):
            hip.call("ryolo_nms_owner", *args)
    hip.call("ryolo_nms_owner", None, 0, nmax, None, 0, None, 0, None, None, hip.stream())          # nothing to do
    hip.call("ryolo_nms_owner", None, batch, 0, None, 0, None, 0, None, None, hip.stream())


def test_fuse_rejects_bad_arguments():
    hip, _, _ = _mods()
    p = _fed_plan(2)
    p.merge(0.3, True, "box")
    good = [hip.ptr(p.cand), hip.ptr(p.order), hip.ptr(p.nsel), hip.ptr(p.keep), hip.ptr(p.nkeep), hip.ptr(p.owner), p.nc, p.Kc, p.Kc, p.ld, 0,
            p.n_ens, hip.ptr(p.fused), hip.ptr(p.fkey), hip.stream()]
    hip.call("ryolo_tile_fuse", *good)
    for at, bad in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (12, None), (13, None), (12, hip.ptr(p.cand)), (6, -1),
                    (7, -1), (8, p.Kc + 1), (9, -1), (10, 2), (10, -1), (11, 0)):
        args = list(good)
        args[at] = bad
        with pytest.raises(RuntimeError, match="ryolo_tile_fuse failed: invalid argument$"):
            hip.call("ryolo_tile_fuse", *args)


# ------------------------------------------------------------------------------------------ 3. "box" against the unfused merge
@pytest.mark.parametrize("i", [0, 3])
def test_box_invariants_and_repeatable_merge(i):
    nc, rates, views, seed, thr, max_nms, max_det = F.CONFIGS[i]
    entries, dets, nums = F.scene(i)
    p = _fed_plan(i)
    cand = p.cand.clone()
    res = {}
    for step, mode in enumerate((None, "box", "wbf", None)):
        res[step] = _result(p, thr, True, mode)
    assert len(res[0]) > 0 and np.array_equal(_bits(res[3]), _bits(res[0])), "merge is not repeatable across modes"
    assert torch.equal(p.cand.view(torch.int32), cand.view(torch.int32))
    assert np.array_equal(_bits(res[0]), _bits(V.oracle_merge(entries, rates, F.S, dets, nums, F.MK, nc, thr, True, max_nms, max_det)))
    plain, box, wbf = res[0], res[1], res[2]
    assert box.shape == plain.shape and np.array_equal(_bits(box[:, 5:]), _bits(plain[:, 5:]))      # score, class, num, order
    st = {}
    F.fused_merge(entries, rates, F.S, dets, nums, F.MK, nc, thr, True, max_nms, max_det, "box", stats=st)
    single = np.array(st["out_sizes"]) == 1
    assert single.sum() > 20 and (~single).sum() > 20
    assert np.array_equal(_bits(box[single]), _bits(plain[single]))                                  # lone boxes: bit for bit
    assert (_bits(box[~single, :5]) != _bits(plain[~single, :5])).any(1).sum() > 20                    # clusters: fused
    assert wbf.shape == plain.shape and not np.array_equal(_bits(wbf[:, 5]), _bits(plain[:, 5]))
    assert (np.diff(wbf[:, 5]) <= 0).all()


# ------------------------------------------------------------------------------------------ 4-5. the detector
@pytest.fixture(scope="module")
def det3():
    _, _, tiled = _mods()
    return tiled.TiledDetector(_model(3), size=256, overlap=64, batch=4, conf_thres=0.05, iou_thres=0.4, max_nms=1500)


SCENE = np.random.RandomState(3).randint(0, 256, (520, 700, 3)).astype(np.uint8)


def test_default_unchanged(det3):
    _, _, tiled = _mods()
    assert det3.fuse is None
    rates, views = (1.0,), ("id", "hflip", "rot90")
    with _with(det3, rates=rates, views=views):
        without = det3(SCENE).cpu().numpy()
        with _with(det3, fuse=None):
            got = det3(SCENE).cpu().numpy()
        exp = _host_composition(det3, SCENE, rates, views)
    assert len(exp) > 0
    assert got.shape == exp.shape and np.array_equal(_bits(got), _bits(exp))
    assert np.array_equal(_bits(without), _bits(exp))
    with pytest.raises(ValueError):
        tiled.TiledDetector(det3.model, size=256, overlap=64, batch=4, fuse="max")
    with _with(det3, fuse="max"):
        with pytest.raises(ValueError):
            det3(SCENE)


_REPLAYS = {}


def _replays(det, img, rates, views):
    """The detector's own captured graph over numpy cuts of every entry (test_gpu_tiled_views._host_composition without its merge) ->
    (entries, dets [E_pad, mk, 7], nums [E_pad]); once per (rates, views)."""
    if (rates, views) in _REPLAYS:
        return _REPLAYS[(rates, views)]
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
    _REPLAYS[(rates, views)] = (entries, dets, nums)
    return _REPLAYS[(rates, views)]


@pytest.mark.parametrize("mode", F.MODES)
@pytest.mark.parametrize("rates,views", [((1.0,), ("id", "hflip", "rot90")), ((1.0, 0.5), V.NAMES)])
def test_end_to_end_vs_host_composition(det3, rates, views, mode):
    scene = torch.from_numpy(SCENE).to(DEV)
    with _with(det3, rates=rates, views=views, fuse=mode):
        got = det3(SCENE).cpu().numpy()
        again = det3(SCENE).cpu().numpy()
        entries, dets, nums = _replays(det3, SCENE, rates, views)
        st = {}
        exp = F.fused_merge(entries, rates, det3.size, dets, nums, det3.mk, det3.nc, det3.merge_iou, True, det3.max_nms, det3.max_det, mode,
                            n_ens=len(rates) * len(views), stats=st)
        print(f"{rates} x {len(views)} views {mode}: rows {len(exp)} clusters>=2 {(np.array(st['sizes']) >= 2).sum()}")
        assert len(exp) > 0
        assert got.shape == exp.shape and np.array_equal(_bits(got), _bits(exp))
        assert np.array_equal(_bits(again), _bits(got)), "two consecutive runs differ"
        # run_async leaves everything on the device: with the plan built (the calls above), a synchronising call raises
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out, num = det3.run_async(scene)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        n = int(num.item())
        assert np.array_equal(_bits(out[:n].cpu().numpy()), _bits(got))
