"""GPU tests of the seam-aware full-scene merge (csrc/seam.hip ryolo_tile_seam_flags / ryolo_tile_seam_cover, lib/tiled.py Seam).
Everything is compared on the bits with the host restatement tests/seam_ref.py (checked on the CPU in tests/test_tiled_seam_cpu.py): the
cut / redundant bits, key2 and the counts; the whole merge for every seam x fuse x gt_only; the planted scene whose answer is known by
construction; rule 2 alone over keep lists of every size class; argument validation; and the whole detector against a host composition
around its own captured graph."""
import numpy as np
import pytest
import torch

from ryolov4_amd.synth import synth_nms_boxes
from tests import seam_ref as R
from tests import test_gpu_tiled_fusion as TF
from tests import views_ref as V
from tests.test_gpu_tiled_views import _bits, _feed, _host_composition, _model, _plan, _with

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
NV = len(R.VIEWS)


def _mods():
    from ryolov4_amd import hip
    from ryolov4_amd.lib import tiled
    return hip, tiled


def _fed_plan(i):
    """A ScenePlan of the synthetic scene i with its candidates collected and its window table uploaded (TiledDetector does the upload
    per scene; a plan fed by hand has to)."""
    _, tiled = _mods()
    nc = R.CONFIGS[i][0]
    entries, dets, nums = R.seam_scene(i)
    p = _plan(tiled, R.SH, R.SW, R.S, R.OV, R.BATCH, R.MK, nc, R.RATES, R.VIEWS)
    assert p.T == len(entries) and p.T % R.BATCH != 0 and p.nviews == NV
    tiled._h2d(p.win, p.rows)
    _feed(p, dets, nums)
    return p


def _result(p, thr, gt, fuse, seam):
    out, num = p.merge(thr, gt, fuse) if seam is None else p.merge_seam(thr, gt, fuse, seam)
    n = int(num.item())
    o = out.cpu().numpy()
    assert not o[n:].any(), "rows past num are not zero"
    return o[:n]


def _ref(i, gt, seam, fuse, stats=None, max_nms=5000, max_det=5000):
    nc, _, thr = R.CONFIGS[i]
    entries, dets, nums = R.seam_scene(i)
    return R.seam_merge(entries, R.RATES, R.S, dets, nums, R.MK, nc, thr, gt, max_nms, max_det, R.SH, R.SW, NV, seam, fuse, stats=stats)


# ------------------------------------------------------------------------------------------ 1. flags, key2 and counts
@pytest.mark.parametrize("i", range(len(R.CONFIGS)))
def test_flags_key2_and_counts_vs_host_restatement(i):
    hip, _ = _mods()
    nc = R.CONFIGS[i][0]
    entries, dets, nums = R.seam_scene(i)
    p = _fed_plan(i)
    cand, key = p.cand.clone(), p.key.clone()
    hkey = key.cpu().numpy()
    for margin in R.MARGINS:
        rows, slots, fl, gap = R.seam_flags(entries, R.RATES, R.S, dets, nums, R.MK, nc, R.SH, R.SW, NV, margin, True)
        cut = fl & 15
        if margin == 2.0:                                                   # floors: the comparison below must not go vacuous
            assert all(((cut & b) != 0).sum() > 0 for b in (1, 2, 4, 8)) and ((cut & (cut - 1)) != 0).sum() > 0
            assert (cut != 0).sum() >= 100 and (fl & 16).astype(bool).sum() >= 20
        for whole in (1, 0):
            flags = torch.full((p.ld,), 99, dtype=torch.uint8, device=DEV)
            key2 = torch.full((nc + 1, p.ld), 7.0, dtype=torch.float32, device=DEV)
            counts = torch.full((2,), 77, dtype=torch.int32, device=DEV)
            hip.call("ryolo_tile_seam_flags", hip.ptr(p.cand), hip.ptr(p.key), hip.ptr(p.win), hip.ptr(p.geom), p.T, NV, R.MK, p.ld, nc, R.S, margin,
                     whole, hip.ptr(flags), hip.ptr(key2), hip.ptr(counts), hip.stream())
            exp = np.zeros(p.ld, dtype=np.uint8)
            exp[slots] = fl if whole else cut
            got = flags.cpu().numpy()
            assert np.array_equal(got, exp), (margin, whole, np.nonzero(got != exp)[0][:8])
            red = np.nonzero(fl & 16)[0] if whole else np.zeros(0, np.int64)
            assert counts.cpu().tolist() == [len(red), 0]
            if whole:
                ekey = hkey.copy()
                ekey[rows[red, 6].astype(np.int64), slots[red]] = -np.inf
                assert np.array_equal(_bits(key2[:nc].cpu().numpy()), _bits(ekey))
            else:
                assert (key2[:nc] == 7.0).all(), "key2 was written without rule 1"
            assert (key2[nc] == -np.inf).all(), "the seam merge's final key is not reset"
    assert torch.equal(p.cand.view(torch.int32), cand.view(torch.int32)) and torch.equal(p.key.view(torch.int32), key.view(torch.int32))


# ------------------------------------------------------------------------------------------ 2. the whole merge
SEAMS = (R.SeamRef(), R.SeamRef(0.0, 0.5, True), R.SeamRef(2.0, 0.3, False), R.SeamRef(2.0, None, True))


@pytest.mark.parametrize("gt", [True, False])
@pytest.mark.parametrize("i", range(len(R.CONFIGS)))
def test_seam_merge_vs_host_restatement(i, gt):
    _, tiled = _mods()
    nc, _, thr = R.CONFIGS[i]
    entries, dets, nums = R.seam_scene(i)
    p = _fed_plan(i)
    cand, key = p.cand.clone(), p.key.clone()
    plain = V.oracle_merge(entries, R.RATES, R.S, dets, nums, R.MK, nc, thr, gt, 5000, 5000)
    for seam in SEAMS:
        for fuse in (None, "box", "wbf"):
            st = {}
            exp = _ref(i, gt, seam, fuse, st)
            if seam == R.SeamRef():                                         # floors
                assert st["redundant"] >= 20 and st["covered"] >= 5, st
            got = _result(p, thr, gt, fuse, tiled.Seam(*seam) if fuse else seam._asdict())
            assert got.shape == exp.shape, (seam, fuse, got.shape, exp.shape)
            assert np.array_equal(_bits(got), _bits(exp)), (seam, fuse, np.nonzero((_bits(got) != _bits(exp)).any(1))[0][:8])
            assert p.seam_counts.cpu().tolist() == [st["redundant"], st["covered"]], (seam, fuse)
            if fuse is None:
                assert got.shape != plain.shape or not np.array_equal(_bits(got), _bits(plain)), "the seam rules changed nothing"
        again = _result(p, thr, gt, None, None)                             # seam=None afterwards: the plain merge, bit for bit
        assert again.shape == plain.shape and np.array_equal(_bits(again), _bits(plain)), seam
    assert torch.equal(p.cand.view(torch.int32), cand.view(torch.int32)) and torch.equal(p.key.view(torch.int32), key.view(torch.int32))


def test_seam_merge_with_a_capped_selection():
    """max_nms 9 per class and max_det 13: rule 1 frees places in the selection for rows that were beyond the cap."""
    _, tiled = _mods()
    nc, _, thr = R.CONFIGS[0]
    entries, dets, nums = R.seam_scene(0)
    p = _plan(tiled, R.SH, R.SW, R.S, R.OV, R.BATCH, R.MK, nc, R.RATES, R.VIEWS, 9, 13)
    tiled._h2d(p.win, p.rows)
    _feed(p, dets, nums)
    for seam in (R.SeamRef(), R.SeamRef(2.0, 0.3, False)):
        for fuse in (None, "wbf"):
            exp = _ref(0, True, seam, fuse, max_nms=9, max_det=13)
            got = _result(p, thr, True, fuse, tiled.Seam(*seam))
            assert got.shape == exp.shape and np.array_equal(_bits(got), _bits(exp)), (seam, fuse)


# ------------------------------------------------------------------------------------------ 3. the planted scene
def test_planted_scene_through_a_scene_plan():
    _, tiled = _mods()
    entries, dets, nums = R.planted_scene()
    p = _plan(tiled, R.PH, R.PW, R.PS, R.POV, 4, R.PMK, 1, (1.0,), ("id",))
    assert p.entries == entries
    tiled._h2d(p.win, p.rows)
    _feed(p, dets, nums)
    thr = 0.4
    off = _result(p, thr, True, None, None)
    assert len(off) == 9 and R.has_box(off, (238, 100, 36, 20)) and not R.has_box(off, (250, 100, 60, 20))
    on = _result(p, thr, True, None, tiled.Seam())
    assert len(on) == 8 and R.has_box(on, (250, 100, 60, 20)) and not R.has_box(on, (320, 269.5, 24, 11))
    assert p.seam_counts.cpu().tolist() == [3, 0]
    low = _result(p, thr, True, None, tiled.Seam(cover=0.5))
    assert len(low) == 7 and not R.has_box(low, (193, 300, 126, 16)) and R.has_box(low, (261, 300, 138, 16))
    assert p.seam_counts.cpu().tolist() == [3, 1]
    only2 = _result(p, thr, True, None, tiled.Seam(whole=False))
    assert np.array_equal(_bits(only2), _bits(off)) and p.seam_counts.cpu().tolist() == [0, 0]
    only2 = _result(p, thr, True, None, tiled.Seam(whole=False, cover=0.5))
    assert len(only2) == 8 and not R.has_box(only2, (193, 300, 126, 16)) and p.seam_counts.cpu().tolist() == [0, 1]
    only1 = _result(p, thr, True, None, tiled.Seam(cover=None))
    assert np.array_equal(_bits(only1), _bits(on)) and p.seam_counts.cpu().tolist() == [3, 0]
    for seam in (None, tiled.Seam(), tiled.Seam(cover=0.5), tiled.Seam(cover=0.05), tiled.Seam(whole=False), tiled.Seam(cover=None),
                 tiled.Seam(margin=0.0), tiled.Seam(margin=8.0, cover=0.3)):
        for fuse in (None, "box"):
            out = _result(p, thr, True, fuse, seam)
            for box in ((100, 100, 20, 10), (100, 100, 60, 40), (20, 20, 30, 30), (687.5, 500, 25, 30)):
                assert R.has_box(out, box), (seam, fuse, box)
            if seam is not None:
                exp = R.seam_merge(entries, (1.0,), R.PS, dets, nums, R.PMK, 1, thr, True, 5000, 5000, R.PH, R.PW, 1, R.SeamRef(seam.margin, seam.cover, seam.whole),
                                   fuse, check=seam.margin != 0.0)          # margin 0 on this scene: tests/test_tiled_seam_cpu.py _planted
                assert out.shape == exp.shape and np.array_equal(_bits(out), _bits(exp)), (seam, fuse)
    assert np.array_equal(_bits(_result(p, thr, True, None, None)), _bits(off))


# ------------------------------------------------------------------------------------------ 4. rule 2 alone
def _cover_case(N, cover, seed):
    """Three classes of clustered boxes with N, 0 or (2N + 2) // 3, and N // 2 kept positions out of K = 2 * max(N, 1) selected ones; random
    cut bits; boxes of a pair within GUARD of `cover` are moved (from the seeded stream) until no pair is."""
    rng = np.random.RandomState(seed)
    K = 2 * max(N, 1)
    nks = [N, 0 if N in (1, 130) else (2 * N + 2) // 3, N // 2]
    ld = 3 * K + 5
    rboxes = np.zeros((3, K, 5), dtype=f32)
    order = np.zeros((3, K), dtype=np.int64)
    keep = np.full((3, K), -7, dtype=np.int64)
    flags = (rng.randint(0, 16, ld) * (rng.rand(ld) < 0.6)).astype(np.uint8)
    slots = rng.permutation(ld)[:3 * K].reshape(3, K)
    for c in range(3):
        rboxes[c] = synth_nms_boxes(K, "C", seed=seed + c, ncls=1)[0]
        order[c] = slots[c]
        keep[c, :nks[c]] = np.sort(rng.permutation(K)[:nks[c]])
    while True:
        moved = 0
        for c in range(3):
            kp = keep[c, :nks[c]]
            g = []
            cov, area = R.cov_matrix(rboxes[c, kp])
            elig = (area[None, :] > area[:, None]) & ((flags[order[c, kp]] & 15) != 0)[:, None] & ~np.eye(len(kp), dtype=bool)
            with np.errstate(invalid="ignore"):
                near = elig & (np.abs(cov.astype(np.float64) - np.float64(f32(cover))) < R.GUARD)
            for a in np.nonzero(near.any(1))[0]:
                rboxes[c, kp[a], :2] += rng.uniform(-3, 3, 2).astype(f32)
                moved += 1
        if not moved:
            break
    return K, ld, nks, rboxes, order, keep, flags


def _run_cover(K, ld, nks, rboxes, order, keep, flags, cover, nsel=None):
    hip, _ = _mods()
    need = hip._Z()
    hip.call("ryolo_tile_seam_workspace_bytes", 3, K, need)
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    d_rb, d_or, d_keep, d_fl = t(rboxes), t(order), t(keep), t(flags)
    d_nsel = t(np.full(3, K, dtype=np.int32) if nsel is None else np.asarray(nsel, dtype=np.int32))
    d_nk = t(np.asarray(nks, dtype=np.int32))
    fkey = torch.full((ld,), 0.5, dtype=torch.float32, device=DEV)
    counts = torch.tensor([5, 0], dtype=torch.int32, device=DEV)
    hip.call("ryolo_tile_seam_cover", hip.ptr(d_rb), hip.ptr(d_or), hip.ptr(d_nsel), hip.ptr(d_keep), hip.ptr(d_nk), 3, K, K, hip.ptr(d_fl), ld, cover,
             hip.ptr(fkey), hip.ptr(counts), hip.ptr(ws), ws.numel(), hip.stream())
    return fkey.cpu().numpy(), counts.cpu().tolist()


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 130, 700])
def test_cover_alone_vs_host_restatement(N):
    cover = 0.5
    K, ld, nks, rboxes, order, keep, flags = _cover_case(N, cover, 100 + N)
    exp = np.full(ld, 0.5, dtype=f32)
    drops = 0
    for c in range(3):
        kp = keep[c, :nks[c]]
        d = R.cover_drops(rboxes[c, kp], (flags[order[c, kp]] & 15) != 0, cover)
        exp[order[c, kp[d]]] = -np.inf
        drops += int(d.sum())
    if N >= 63:
        assert drops >= 5 and drops < sum(nks), "nothing to drop, or nothing to keep"
    fkey, counts = _run_cover(K, ld, nks, rboxes, order, keep, flags, cover)
    assert np.array_equal(_bits(fkey), _bits(exp)), np.nonzero(fkey != exp)[0][:8]
    assert counts == [5, drops]                                             # rule 1's count is left alone
    if N != 65:
        return
    # device tables are not trusted: a kept position outside the selection and a slot outside the candidates are empty boxes — never
    # cut, covering nothing — and no access leaves the buffers.  The expectation is the restatement over the remaining keep list.
    keep2, order2 = keep.copy(), order.copy()
    nsel = [K, K, int(keep[2, nks[2] - 1])]                                 # class 2: its last kept position is past the selection
    keep2[0, 3], keep2[0, 7] = K + 3, -1
    order2[0, keep[0, 11]], order2[0, keep[0, 12]] = ld + 7, -2
    exp = np.full(ld, 0.5, dtype=f32)
    drops = 0
    for c in range(3):
        kp = keep2[c, :nks[c]]
        ok = (kp >= 0) & (kp < nsel[c])
        ok[ok] &= (order2[c, kp[ok]] >= 0) & (order2[c, kp[ok]] < ld)
        kp = kp[ok]
        d = R.cover_drops(rboxes[c, kp], (flags[order2[c, kp]] & 15) != 0, cover, gaps=(g := []))
        assert not g or min(g) >= R.GUARD
        exp[order2[c, kp[d]]] = -np.inf
        drops += int(d.sum())
    fkey, counts = _run_cover(K, ld, nks, rboxes, order2, keep2, flags, cover, nsel)
    assert np.array_equal(_bits(fkey), _bits(exp)) and counts == [5, drops]


# ------------------------------------------------------------------------------------------ 5. validation
def test_seam_entry_points_reject_bad_arguments():
    hip, tiled = _mods()
    p = _fed_plan(0)
    p.merge_seam(0.3, True, None, tiled.Seam())
    ARG, WS = "failed: invalid argument$", "failed: workspace too small$"
    good = [hip.ptr(p.cand), hip.ptr(p.key), hip.ptr(p.win), hip.ptr(p.geom), p.T, NV, R.MK, p.ld, p.nc, R.S, 2.0, 1, hip.ptr(p.flags), hip.ptr(p.key2),
            hip.ptr(p.seam_counts), hip.stream()]
    hip.call("ryolo_tile_seam_flags", *good)
    for at, bad in ((0, None), (1, None), (2, None), (3, None), (12, None), (13, None), (14, None), (13, hip.ptr(p.key)), (4, -1), (4, p.T - 1), (5, 0),
                    (5, -1), (6, -1), (6, 0), (6, R.MK + 1), (7, -1), (8, -1), (9, 0), (10, -1.0), (10, float("nan")), (10, float("inf")), (11, 2), (11, -1)):
        args = list(good)
        args[at] = bad
        with pytest.raises(RuntimeError, match="ryolo_tile_seam_flags " + ARG):
            hip.call("ryolo_tile_seam_flags", *args)
    need = hip._Z()
    hip.call("ryolo_tile_seam_workspace_bytes", p.nc, p.Kc, need)
    assert 0 < need.value <= p.seam_ws.numel()
    for args in ((-1, 4, need), (3, -1, need), (3, 4, None)):
        with pytest.raises(RuntimeError, match="ryolo_tile_seam_workspace_bytes " + ARG):
            hip.call("ryolo_tile_seam_workspace_bytes", *args)
    good = [hip.ptr(p.rboxes), hip.ptr(p.order), hip.ptr(p.nsel), hip.ptr(p.keep), hip.ptr(p.nkeep), p.nc, p.Kc, p.Kc, hip.ptr(p.flags), p.ld, 0.7,
            hip.ptr(p.fkey), hip.ptr(p.seam_counts), hip.ptr(p.seam_ws), p.seam_ws.numel(), hip.stream()]
    hip.call("ryolo_tile_seam_cover", *good)
    for at, bad, err in ((0, None, ARG), (1, None, ARG), (2, None, ARG), (3, None, ARG), (4, None, ARG), (8, None, ARG), (11, None, ARG), (12, None, ARG),
                         (13, None, ARG), (5, -1, ARG), (6, -1, ARG), (7, -1, ARG), (7, p.Kc + 1, ARG), (9, -1, ARG), (10, 0.04, ARG), (10, 1.01, ARG),
                         (10, float("nan"), ARG), (14, need.value - 1, WS), (14, 0, WS)):
        args = list(good)
        args[at] = bad
        with pytest.raises(RuntimeError, match="ryolo_tile_seam_cover " + err):
            hip.call("ryolo_tile_seam_cover", *args)
    hip.call("ryolo_tile_seam_cover", None, None, None, None, None, 0, p.Kc, p.Kc, None, p.ld, 0.7, None, None, None, 0, hip.stream())       # nothing to do
    for bad in ("on", {"cover": 2.0}, {"whole": False, "cover": None}, 0.7):
        with pytest.raises(ValueError):
            p.merge_seam(0.3, True, None, bad)


def test_detector_validates_seam(det3):
    _, tiled = _mods()
    assert det3.seam is None
    with pytest.raises(ValueError):
        tiled.TiledDetector(det3.model, size=256, overlap=64, batch=4, seam={"cover": 2.0})
    with pytest.raises(ValueError):
        tiled.TiledDetector(det3.model, size=256, overlap=64, batch=4, seam="on")
    for bad in ("on", {"margin": -1}, {"whole": False, "cover": None}):
        with _with(det3, seam=bad):
            with pytest.raises(ValueError):
                det3(_scene(3))


# ------------------------------------------------------------------------------------------ 6. the detector
@pytest.fixture(scope="module")
def det3():
    _, tiled = _mods()
    return tiled.TiledDetector(_model(3), size=256, overlap=64, batch=4, conf_thres=0.05, iou_thres=0.4, max_nms=1500)


def _scene(seed):
    return np.random.RandomState(seed).randint(0, 256, (520, 700, 3)).astype(np.uint8)


E2E_CASES = ((R.SeamRef(), None), (R.SeamRef(), "wbf"), (R.SeamRef(2.0, 0.3, False), None))


def _guarded_replays(det, rates, views):
    """The detector's own captured graph over numpy cuts of every entry (test_gpu_tiled_fusion._replays), for the first seeded scene whose
    detections keep GUARD from every threshold that decides something in E2E_CASES (seam_ref check="decisive": the network fills every
    window with boxes on its lattice, thousands of them): a network's boxes cannot be redrawn, the scene can.  The restatement's results
    come back with the replays, computed once."""
    for seed in range(3, 35):
        img = _scene(seed)
        TF._REPLAYS.pop((rates, views), None)                               # that cache is keyed for the one scene of its own tests
        entries, dets, nums = TF._replays(det, img, rates, views)
        TF._REPLAYS.pop((rates, views), None)
        dets, nums = dets.copy(), nums.copy()
        refs = {}
        try:
            for seam, fuse in E2E_CASES:
                st = {}
                exp = R.seam_merge(entries, rates, det.size, dets, nums, det.mk, det.nc, det.merge_iou, True, det.max_nms, det.max_det, 520, 700,
                                   len(views), seam, fuse, n_ens=len(rates) * len(views), stats=st, check="decisive")
                refs[(seam, fuse)] = (exp, st)
        except AssertionError as e:
            if "on a threshold" in str(e) or "from a rule-1 threshold" in str(e):
                print(f"scene {seed} redrawn:", e)
                continue
            raise
        return img, entries, dets, nums, refs
    raise AssertionError("every scene has a detection on a threshold")


@pytest.mark.parametrize("rates,views", [((1.0,), ("id", "hflip", "rot90")), ((1.0, 0.5), V.NAMES)])
def test_end_to_end_vs_host_composition(det3, rates, views):
    _, tiled = _mods()
    with _with(det3, rates=rates, views=views):
        img, entries, dets, nums, refs = _guarded_replays(det3, rates, views)
        scene = torch.from_numpy(img).to(DEV)
        plain = det3(img).cpu().numpy()
        assert np.array_equal(_bits(plain), _bits(V.oracle_merge(entries, rates, det3.size, dets, nums, det3.mk, det3.nc, det3.merge_iou, True,
                                                                  det3.max_nms, det3.max_det)))
        if len(views) == 3:                                                 # the replays above are what the independent composition sees
            assert np.array_equal(_bits(plain), _bits(_host_composition(det3, img, rates, views)))
        for seam, fuse in E2E_CASES:
            with _with(det3, seam=tiled.Seam(*seam), fuse=fuse):
                got = det3(img).cpu().numpy()
                again = det3(img).cpu().numpy()
                exp, st = refs[(seam, fuse)]
                print(f"{rates} x {len(views)} views {seam} {fuse}: rows {len(exp)} (plain {len(plain)}) {st}")
                assert len(exp) > 0
                assert got.shape == exp.shape and np.array_equal(_bits(got), _bits(exp)), (seam, fuse)
                assert np.array_equal(_bits(again), _bits(got)), "two consecutive runs differ"
                p = det3.plan(520, 700)
                assert p.seam_counts.cpu().tolist() == [st["redundant"], st["covered"]]
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode("error")                 # run_async leaves everything on the device
                try:
                    out, num = det3.run_async(scene)
                finally:
                    torch.cuda.set_sync_debug_mode("default")
                n = int(num.item())
                assert np.array_equal(_bits(out[:n].cpu().numpy()), _bits(got))
        assert np.array_equal(_bits(det3(img).cpu().numpy()), _bits(plain)), "seam=None after seam merges is not the plain result"
