"""CPU tests of the seam-aware full-scene merge: the host restatement tests/seam_ref.py (which the GPU tests compare the kernels with on
the bits) against the planted scene whose answer is known by construction, against an independent float64 polygon clip, and against
its own float64 run; the floors the GPU tests rely on; the redraw loop of the scene generator; and the validation of lib/tiled.py Seam."""
import numpy as np
import pytest

from tests import fusion_ref as F
from tests import seam_ref as R
from tests import views_ref as V

f32, f64 = np.float32, np.float64
THR = 0.4                                                                 # the detector's default merge_iou


def _planted(seam, fuse=None, stats=None):
    entries, dets, nums = R.planted_scene()
    if seam is None:
        return V.oracle_merge(entries, (1.0,), R.PS, dets, nums, R.PMK, 1, THR, True, 5000, 5000)
    # margin 0 puts every fragment's clipped side exactly on its threshold.  That is this scene's point, and it is safe here only: theta
    # is 0 and every coordinate a multiple of 0.5, so each step is exact in fp32, in float64 and on the device alike
    return R.seam_merge(entries, (1.0,), R.PS, dets, nums, R.PMK, 1, THR, True, 5000, 5000, R.PH, R.PW, 1, seam, fuse, stats=stats,
                        check=seam.margin != 0.0)


# ------------------------------------------------------------------------------------------ the planted scene
def test_planted_scene_plain_merge_shows_both_failures():
    out = _planted(None)
    assert len(out) == 9
    assert R.has_box(out, (238, 100, 36, 20)) and not R.has_box(out, (250, 100, 60, 20))      # the fragment suppressed the whole object
    assert R.has_box(out, (320, 269.5, 24, 11))                                               # a fragment survives as a false positive
    assert R.has_box(out, (193, 300, 126, 16)) and R.has_box(out, (261, 300, 138, 16))        # longer than the overlap: two fragments


def test_planted_scene_default_seam():
    st = {}
    out = _planted(R.SeamRef(), stats=st)
    assert len(out) == 8
    assert R.has_box(out, (250, 100, 60, 20)) and not R.has_box(out, (238, 100, 36, 20))
    assert R.has_box(out, (320, 250, 24, 50)) and not R.has_box(out, (320, 269.5, 24, 11))
    assert R.has_box(out, (193, 300, 126, 16)) and R.has_box(out, (261, 300, 138, 16))        # no window holds the long object whole
    assert st["redundant"] == 3 and st["covered"] == 0


def test_planted_scene_lower_cover_removes_the_smaller_long_fragment():
    st = {}
    out = _planted(R.SeamRef(cover=0.5), stats=st)
    assert len(out) == 7
    assert not R.has_box(out, (193, 300, 126, 16)) and R.has_box(out, (261, 300, 138, 16))
    assert st["covered"] == 1


def test_planted_scene_one_rule_at_a_time():
    st = {}
    only2 = _planted(R.SeamRef(whole=False), stats=st)                     # rule 2 alone at cover 0.7: the fragments that survived the NMS
    assert st["redundant"] == 0                                            # overlap their whole boxes by less than that, or have none
    assert np.array_equal(only2, _planted(None)) and st["covered"] == 0
    only2 = _planted(R.SeamRef(whole=False, cover=0.5), stats=st)
    assert len(only2) == 8 and not R.has_box(only2, (193, 300, 126, 16)) and st["covered"] == 1
    only1 = _planted(R.SeamRef(cover=None), stats=st)
    assert st["covered"] == 0 and st["redundant"] == 3
    assert np.array_equal(only1, _planted(R.SeamRef()))


@pytest.mark.parametrize("seam", [None, R.SeamRef(), R.SeamRef(cover=0.5), R.SeamRef(cover=0.05), R.SeamRef(whole=False), R.SeamRef(cover=None),
                                  R.SeamRef(margin=0.0), R.SeamRef(margin=8.0, cover=0.3)])
@pytest.mark.parametrize("fuse", [None, "box"])
def test_planted_scene_uncut_boxes_survive_every_setting(seam, fuse):
    if seam is None and fuse is not None:
        entries, dets, nums = R.planted_scene()
        out = F.fused_merge(entries, (1.0,), R.PS, dets, nums, R.PMK, 1, THR, True, 5000, 5000, fuse)
    else:
        out = _planted(seam, fuse)
    for box in ((100, 100, 20, 10), (100, 100, 60, 40),                    # the small box inside the larger one: neither is cut
                (20, 20, 30, 30), (687.5, 500, 25, 30)):                   # at the scene border (the second one clipped by it): never cut
        assert R.has_box(out, box), (seam, box)


# ------------------------------------------------------------------------------------------ cov against a polygon clip
def _corners(b):
    """(x, y, w, h, degrees) -> [4, 2] float64 in the NMS's convention (a corner offset (dx, dy) goes to (dx cos + dy sin, -dx sin + dy cos)),
    counter-clockwise in a y-up frame."""
    x, y, w, h, t = (f64(v) for v in b)
    c, s = np.cos(np.deg2rad(t)), np.sin(np.deg2rad(t))
    return np.array([[x + dx * c + dy * s, y - dx * s + dy * c] for dx, dy in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2))])


def _clip_area(subject, clip):
    """Sutherland-Hodgman: area of the convex polygon `subject` inside the convex counter-clockwise polygon `clip`, float64."""
    out = [tuple(p) for p in subject]
    for i in range(len(clip)):
        a, b = clip[i], clip[(i + 1) % len(clip)]
        inside = lambda p: (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]) >= 0        # noqa: E731
        src, out = out, []
        for j in range(len(src)):
            p, q = src[j], src[(j + 1) % len(src)]
            if inside(p) != inside(q):
                d1 = (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
                d2 = (b[0] - a[0]) * (q[1] - a[1]) - (b[1] - a[1]) * (q[0] - a[0])
                t = d1 / (d1 - d2)
                cross = (p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1]))
                if inside(p):
                    out.append(p)
                    out.append(cross)
                else:
                    out.append(cross)
            elif inside(p):
                out.append(p)
        if not out:
            return 0.0
    x, y = np.array([p[0] for p in out]), np.array([p[1] for p in out])
    return 0.5 * abs(float(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))))


def test_cov_is_intersection_over_the_cut_area():
    """cov of the definition is inter / area_a written through the pair function's IoU.  Tolerance, from the pair function: it clips in
    fp32 about the pair's midpoint and accepts crossings up to EPS = 1e-5 of an edge's length beyond its ends, so for boxes of at most
    ~60 px the intersection is off by at most a few 1e-3 px^2 plus fp32 rounding of ~1e4 px^2 products (~1e-3 px^2); over area_a >= 16
    px^2 and through the two fp32 divisions that stays below 1e-3 of cov."""
    rng = np.random.RandomState(5)
    n = 120
    b = np.stack([rng.uniform(0, 60, n), rng.uniform(0, 60, n), rng.uniform(4, 40, n), rng.uniform(4, 40, n), rng.uniform(-105, 105, n)], 1).astype(f32)
    b[:6] = [(238, 100, 36, 20, 0), (250, 100, 60, 20, 0), (193, 300, 126, 16, 0), (261, 300, 138, 16, 0), (320, 269.5, 24, 11, 0), (320, 250, 24, 50, 0)]
    cov, area = R.cov_matrix(b)
    assert cov.dtype == f32
    # the planted pairs, known by hand, to the fp32 rounding of cov's five operations (a contained box can come out one ulp below 1)
    assert abs(cov[0, 1] - 1) < 1e-6 and abs(cov[4, 5] - 1) < 1e-6 and abs(cov[2, 3] - 64 / 126) < 1e-6
    worst, nonzero = 0.0, 0
    for i in range(n):
        pi = _corners(b[i])
        for j in range(n):
            if i == j:
                continue
            exp = _clip_area(pi, _corners(b[j])) / (f64(b[i, 2]) * f64(b[i, 3]))
            worst = max(worst, abs(f64(cov[i, j]) - exp))
            nonzero += exp > 0.05
    print(f"cov vs float64 polygon clip: worst |diff| {worst:.2e} over {n * (n - 1)} pairs, {nonzero} above 0.05")
    assert nonzero > 500 and worst < 1e-3


def test_fp32_restatement_against_its_float64_run():
    """seam_flags asserts per row that the float64 run sets the same bits (and returns the distance from the nearest threshold);
    cover_drops must decide alike in both dtypes, and cov itself agrees to fp32 rounding of its five operations."""
    for i in range(len(R.CONFIGS)):
        nc, seed, thr = R.CONFIGS[i]
        entries, dets, nums = R.seam_scene(i)
        for m in R.MARGINS:
            rows, slots, flags, gap = R.seam_flags(entries, R.RATES, R.S, dets, nums, R.MK, nc, R.SH, R.SW, len(R.VIEWS), m, True)
            assert gap.min() >= R.GUARD
        kb = R.deg(rows[rows[:, 6] == 0][:300])
        c32, _ = R.cov_matrix(kb, f32)
        c64, _ = R.cov_matrix(kb, f64)
        ok = ~np.isnan(c64)
        assert np.abs(c32[ok] - c64[ok]).max() <= 4 * np.finfo(f32).eps * max(1.0, np.abs(c64[ok]).max())
        cut = (flags[rows[:, 6] == 0][:300] & 15) != 0
        for cover in R.COVERS:
            g = []
            d32 = R.cover_drops(kb, cut, cover, f32, g)
            assert min(g) >= R.GUARD
            assert np.array_equal(d32, R.cover_drops(kb, cut, cover, f64))


# ------------------------------------------------------------------------------------------ the synthetic scenes of the GPU tests
@pytest.mark.parametrize("i", range(len(R.CONFIGS)))
def test_generator_ends_and_reaches_the_floors(i):
    nc, seed, thr = R.CONFIGS[i]
    R._SCENES.pop(i, None)
    log = []
    entries, dets, nums = R.seam_scene(i, log)
    print(f"scene {i}: rows redrawn per round {log}")
    assert log[-1] == 0 and len(log) <= 6, log                              # the redraw loop ends, and quickly
    assert len(entries) % R.BATCH != 0 and {e[0] for e in entries} == {0, 1} and len({e[3] for e in entries}) == 8
    rows, slots, flags, gap = R.seam_flags(entries, R.RATES, R.S, dets, nums, R.MK, nc, R.SH, R.SW, len(R.VIEWS), 2.0, True)
    cut = flags & 15
    assert all(((cut & b) != 0).sum() > 0 for b in (R.L, R.R, R.T, R.B))
    assert ((cut & (cut - 1)) != 0).sum() > 0 and (cut != 0).sum() >= 100 and ((flags & R.REDUNDANT) != 0).sum() >= 20
    assert ((flags & R.REDUNDANT) != 0).sum() < (cut != 0).sum(), "every cut row is redundant: the negative case is missing"
    for ri in (0, 1):                                                       # both rates have cut rows; only rate 1.0 has a second window in y
        of_rate = np.array([entries[s // R.MK][0] == ri for s in slots])
        assert (cut[of_rate] != 0).sum() > 0
    plain = V.oracle_merge(entries, R.RATES, R.S, dets, nums, R.MK, nc, thr, True, 5000, 5000)
    for fuse in (None, "wbf"):
        st = {}
        out = R.seam_merge(entries, R.RATES, R.S, dets, nums, R.MK, nc, thr, True, 5000, 5000, R.SH, R.SW, len(R.VIEWS), R.SeamRef(), fuse, stats=st)
        assert st["redundant"] >= 20 and st["covered"] >= 5, st
        assert len(out) < len(plain)
    st = {}
    R.seam_merge(entries, R.RATES, R.S, dets, nums, R.MK, nc, thr, True, 5000, 5000, R.SH, R.SW, len(R.VIEWS), R.SeamRef(whole=False), None, stats=st)
    assert st["redundant"] == 0 and st["covered"] >= 50, st


# ------------------------------------------------------------------------------------------ Seam
def test_seam_validation():
    from ryolov4_amd.lib.tiled import Seam, check_seam
    s = Seam()
    assert (s.margin, s.cover, s.whole) == (2.0, 0.7, True)
    assert check_seam(None) is None and check_seam(s) == s and check_seam({"cover": 0.5}) == Seam(cover=0.5)
    assert check_seam({"margin": 0, "cover": None}) == Seam(0.0, None, True) and Seam(cover=0.05).cover == 0.05 and Seam(cover=1).cover == 1.0
    assert Seam(whole=False).whole is False
    for kw in ({"margin": -1}, {"margin": float("nan")}, {"margin": float("inf")}, {"margin": "2"}, {"margin": None}, {"cover": 0.04}, {"cover": 1.01},
               {"cover": float("nan")}, {"cover": "0.7"}, {"cover": True}, {"whole": 1}, {"whole": None}, {"whole": False, "cover": None},
               {"edge": 3}):
        with pytest.raises(ValueError):
            Seam(**kw) if "edge" not in kw else check_seam(kw)
        with pytest.raises(ValueError):
            check_seam(kw)
    for bad in ("on", 0.7, True, (2.0, 0.7, True)):
        with pytest.raises(ValueError):
            check_seam(bad)
    s.cover = 3.0                                                           # a value set after construction is checked where it is used
    with pytest.raises(ValueError):
        check_seam(s)
