"""CPU tests of the cluster fusion of the full-scene merge (lib/tiled.py fuse="box" | "wbf", include/ryolo.h ryolo_tile_fuse): the
host restatement tests/fusion_ref.py against hand cases, against its own structure (owners partition the selection, the keep set is
the oracle's), against views_ref.oracle_merge where fusion must change nothing, and against a float64 run of the same formulas; and
the pure-Python argument check."""
import numpy as np
import pytest

import oracle
from tests import fusion_ref as F
from tests import views_ref as V

f32 = np.float32


def _row(x, y, w, h, t, s, c=0):
    return [x, y, w, h, t, s, c]


def _pair(a, b, mode="box", n=8):
    return F.fuse_cluster(np.array([a, b], dtype=f32), mode, n)


# ------------------------------------------------------------------------------------------ hand cases
def test_theta_has_period_pi():
    """1.55 and -1.56 are 0.03 rad apart across the seam, not 3.11: the fused angle stays next to the owner's, far from the mean -0.005."""
    x, y, w, h, t, s = _pair(_row(100, 100, 20, 60, 1.55, 0.9), _row(100, 100, 20, 60, -1.56, 0.6))
    assert abs(float(t) - 1.56264) < 5e-6, t
    assert (x, y, w, h) == (f32(100), f32(100), f32(20), f32(60)) and s == f32(0.9)


def test_near_square_box_seen_both_ways_takes_the_swap():
    """(30 x 31, 0.10) and (31 x 30, 0.10 - pi/2) are one box: fused in the owner's frame, not averaged to 30.5 x 30.5 at -0.69."""
    st = {}
    r = np.array([_row(100, 100, 30, 31, 0.10, 0.8), _row(100, 100, 31, 30, f32(0.10) - V.HALF_PI, 0.8)], dtype=f32)
    x, y, w, h, t, s = F.fuse_cluster(r, "box", 8, stats=st)
    assert st.get("swaps") == 1
    assert w == f32(30) and h == f32(31.000002) and t == f32(0.1), (w, h, t)


def test_unwrapped_inputs():
    """theta as the plain collect path leaves it (|theta| up to pi/2 + 0.27): 1.80 and -1.80 are 0.458 apart; the result is wrapped."""
    x, y, w, h, t, s = _pair(_row(100, 100, 20, 60, 1.80, 0.9), _row(100, 100, 20, 60, -1.80, 0.5))
    assert abs(float(t) - -1.50531) < 5e-6, t
    assert -V.HALF_PI <= t < V.HALF_PI


@pytest.mark.parametrize("mode", F.MODES)
def test_single_member_row_comes_back_bit_for_bit(mode):
    for t in (1.80, -1.83, float(V.HALF_PI), -float(V.HALF_PI), 0.0, 0.3):
        r = np.array([_row(123.456, 7.25, 13.7, 41.3, t, 0.37, 2)], dtype=f32)
        x, y, w, h, th, s = F.fuse_cluster(r, mode, 8)
        got = np.array([x, y, w, h, th], dtype=f32)
        assert np.array_equal(got.view(np.uint32), r[0, :5].view(np.uint32)), t      # theta unwrapped
        if mode == "box":
            assert s.view(np.uint32) == r[0, 5].view(np.uint32)
        else:
            assert s == (r[0, 5] / f32(1)) * (f32(1) / f32(8))


def test_wbf_score_counts_the_ensemble():
    a, b = _row(50, 50, 10, 30, 0.2, 0.75), _row(51, 50, 10, 30, 0.2, 0.25)
    assert _pair(a, b, "wbf", 8)[5] == f32(0.5) * f32(0.25)                      # 2 of 8 saw it
    assert _pair(a, b, "wbf", 2)[5] == f32(0.5)
    assert _pair(a, b, "wbf", 1)[5] == f32(0.5)                                  # min(m, n): more boxes than members do not raise it
    assert _pair(a, b, "box", 8)[5] == f32(0.75)


# ------------------------------------------------------------------------------------------ structure on the synthetic scenes
def _clusters(i, gt):
    nc, rates, views, seed, thr, max_nms, max_det = F.CONFIGS[i]
    entries, dets, nums = F.scene(i)
    rows, slots = F.candidates(entries, rates, F.S, dets, nums, F.MK)
    for c in range(nc):
        o, owner, keep = F.class_clusters(rows, slots, c, thr, gt, max_nms)
        yield rows, slots, o, owner, keep, thr


@pytest.mark.parametrize("gt", [True, False])
def test_owners_partition_the_selection(gt):
    seen = 0
    for i in (0, 2, 3):
        for rows, slots, o, owner, keep, thr in _clusters(i, gt):
            n = len(o)
            b = rows[o, :5].copy()
            b[:, 4] = b[:, 4] / f32(np.pi) * f32(180.0)
            assert np.array_equal(np.nonzero(owner == np.arange(n))[0], oracle.nms_rotated(b, rows[o, 5], thr, gt))    # fixed points = keep set
            assert (owner >= 0).all() and (owner <= np.arange(n)).all() and np.isin(owner, keep).all()               # everyone, once
            assert np.array_equal(owner[owner], owner)
            mask = oracle.nms_mask(b, thr, gt)
            kept = np.zeros(n, dtype=bool)
            kept[keep] = True
            for p in np.nonzero(owner != np.arange(n))[0]:
                col = (mask[:p, p >> 6] >> np.uint64(p & 63)) & np.uint64(1)
                first = np.nonzero(col.astype(bool) & kept[:p])[0]
                assert len(first) and first[0] == owner[p]                                                          # the smallest kept suppressor
                seen += 1
    assert seen > 300


@pytest.mark.parametrize("i", range(len(F.CONFIGS)))
@pytest.mark.parametrize("gt", [True, False])
def test_box_mode_changes_geometry_only(i, gt):
    nc, rates, views, seed, thr, max_nms, max_det = F.CONFIGS[i]
    entries, dets, nums = F.scene(i)
    ref = V.oracle_merge(entries, rates, F.S, dets, nums, F.MK, nc, thr, gt, max_nms, max_det)
    st = {}
    got = F.fused_merge(entries, rates, F.S, dets, nums, F.MK, nc, thr, gt, max_nms, max_det, "box", stats=st)
    assert got.dtype == f32 and got.shape == ref.shape and len(ref) > 0
    assert np.array_equal(got[:, 5:].view(np.uint32), ref[:, 5:].view(np.uint32))            # score and class columns, row count, order
    sizes = np.array(st["sizes"])
    assert sum(st["per_class"]) == sizes.sum()                                              # every selected candidate in exactly one cluster
    if max_det != 13:
        assert (sizes >= 2).sum() >= 30 and not np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    else:
        assert len(got) == 13 and max(st["per_class"]) == max_nms


def test_wbf_with_one_ensemble_member_is_the_mean_score():
    """n = 1: the score is W / m, and every cluster of the scenes is held to one ulp of the float64 mean of its members' scores.  Most
    scores lie on the 1/16 lattice the synthetic scenes draw, whose sums are exact, so W / m is one correctly rounded division; the
    planted objects' scores are off it, their sums round at every step, and they are asserted all the same (`rounded` counts them)."""
    checked = multi = rounded = 0
    for i in (0, 1, 3, 4):
        for rows, slots, o, owner, keep, thr in _clusters(i, True):
            for k in keep:
                mem = rows[o[np.nonzero(owner == k)[0]]]
                sc = mem[:, 5].astype(np.float64)
                s = F.fuse_cluster(mem, "wbf", 1)[5]
                mean = sc.sum() / len(sc)
                assert abs(float(s) - mean) <= float(np.spacing(f32(mean))), (s, mean, len(mem))
                checked += 1
                multi += len(mem) > 1
                rounded += len(mem) > 1 and not (sc * 16 == np.round(sc * 16)).all()
    assert checked > 500 and multi > 100 and rounded > 0


def _angle_gap(a, b):
    """|a - b| modulo pi (theta has period pi: a result that rounds to either side of the seam is the same box)."""
    d = (np.asarray(a, np.float64) - np.asarray(b, np.float64) + np.pi / 2) % np.pi - np.pi / 2
    return np.abs(d)


@pytest.mark.parametrize("i", range(len(F.CONFIGS)))
def test_float64_run_of_the_same_formulas_agrees(i):
    """Cluster by cluster (the final order of "wbf" depends on the last bit of a score, so the sorted outputs of two precisions need not
    line up): positions and sizes to 1e-4 px, theta to 1e-5 rad modulo pi.  Scores: at most 36 additions, a division, a quotient and a
    product, each within 2^-24 relative of a value below 1 -> below 40 * 2^-24 = 2.4e-6; asserted at 1e-5."""
    n_ens = len(F.CONFIGS[i][1]) * len(F.CONFIGS[i][2])
    worst = np.zeros(3)
    count = 0
    for gt in (True, False):
        for rows, slots, o, owner, keep, thr in _clusters(i, gt):
            for k in keep:
                mem = rows[o[np.nonzero(owner == k)[0]]]
                for mode in F.MODES:
                    a = np.array(F.fuse_cluster(mem, mode, n_ens), dtype=np.float64)
                    b = np.array(F.fuse_cluster(mem, mode, n_ens, ft=np.float64), dtype=np.float64)
                    worst = np.maximum(worst, [np.abs(a[:4] - b[:4]).max(), _angle_gap(a[4], b[4]), abs(a[5] - b[5])])
                    count += 1
    assert count > 20
    assert worst[0] <= 1e-4 and worst[1] <= 1e-5 and worst[2] <= 1e-5, worst


# ------------------------------------------------------------------------------------------ the argument check
def test_check_fuse():
    from ryolov4_amd.lib import tiled
    assert tiled.check_fuse(None) is None and tiled.check_fuse("box") == "box" and tiled.check_fuse("wbf") == "wbf"
    for bad in ("max", "", 0, True, "BOX", ("box",), 1.0):
        with pytest.raises(ValueError):
            tiled.check_fuse(bad)


def test_merge_signature_keeps_the_two_argument_call():
    import inspect
    from ryolov4_amd.lib import tiled
    p = inspect.signature(tiled.ScenePlan.merge).parameters
    assert list(p) == ["self", "merge_iou", "gt_only", "fuse"] and p["fuse"].default is None and p["gt_only"].default is True
    assert inspect.signature(tiled.TiledDetector.__init__).parameters["fuse"].default is None
