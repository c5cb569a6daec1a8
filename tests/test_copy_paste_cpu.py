"""CPU tests of object-level copy-paste (datasets/copy_paste.py) and of its restatement tests/copy_paste_ref.py, which the kernels of
csrc/copypaste.hip are held to bit for bit in tests/test_gpu_copy_paste.py.

test_clip_ratio_fp64_against_exact_rationals and the hand cases run the restatement ALONE: they pin it (against fractions.Fraction on
this file's lattice set, `_lattice_pairs(6000, seed 7)`: largest deviation 2.8e-14, bound 1e-12; and by hand), they are no coverage of
the kernels.  The draw tests run the product's CopyPaste against the restatement's draw sequence."""
import math
import random
from fractions import Fraction

import numpy as np
import pytest

from tests import copy_paste_ref as R


# ---------------------------------------------------------------------------------------------- 1. the clip against exact rationals
def _lattice_pairs(n, seed):
    """(row quad, item quad) on the integer lattice: the item strictly convex in either orientation, the row anything (convex, bow tie,
    concave, with vertices on the item's edges)."""
    rs = random.Random(seed)
    out = []
    while len(out) < n:
        quad = [(rs.randint(-12, 12), rs.randint(-12, 12)) for _ in range(4)]
        if not R.strictly_convex([v for p in quad for v in p]):
            continue
        row = [(rs.randint(-14, 14), rs.randint(-14, 14)) for _ in range(4)]
        if rs.random() < 0.3:                                          # a vertex of the row ON a vertex / an edge midpoint of the item
            k = rs.randrange(4)
            a, b = quad[k], quad[(k + 1) % 4]
            row[rs.randrange(4)] = a if rs.random() < 0.5 or (a[0] + b[0]) % 2 or (a[1] + b[1]) % 2 else ((a[0] + b[0]) // 2, (a[1] + b[1]) // 2)
        out.append((row, quad))
    return out


def test_clip_ratio_fp64_against_exact_rationals():
    worst, used, partial = 0.0, 0, 0
    for row, quad in _lattice_pairs(6000, 7):
        exact = R.clip_ratio(row, quad, Fraction)
        got = R.clip_ratio(row, quad, float)
        assert (exact is None) == (got is None)
        if exact is None:
            continue
        used += 1
        partial += 0 < exact < 1
        worst = max(worst, abs(got - float(exact)))
    print(f"clip ratio: {used} pairs with area, {partial} partly covered, largest deviation from exact {worst:.3e}")
    assert used > 5000 and partial > 2000
    assert worst <= 1e-12


# ---------------------------------------------------------------------------------------------- 2. hand cases (the restatement alone)
S = 32


def _scene(seed, H=S, W=S):
    return np.random.RandomState(seed).randint(0, 256, size=(H, W, 3)).astype(np.uint8)


def _canvas(B=1):
    return np.full((B, S, S, 3), 7, dtype=np.uint8)


IDENT = ((1.0, 0.0, 0.0, 0.0, 1.0, 0.0),) * 2


def test_identity_paste():
    sc = _scene(1)
    quad = [10, 10, 30, 10, 30, 20, 10, 20]
    it = R.make_item(0, S, S, 0, 2, quad, *IDENT)
    out, tg, union, cover = R.compose([sc], [it], 1, _canvas(), np.zeros((0, 10), np.float32), 0.5)
    want = np.zeros((S, S), dtype=bool)
    want[10:21, 10:31] = True                                           # edges are inside: 21 x 11 pixels
    assert np.array_equal(union[0], want) and cover.max() == 1
    assert np.array_equal(out[0][want], sc[want]) and (out[0][~want] == 7).all()
    assert tg.shape == (1, 10) and tg[0].tolist() == [0.0, 2.0] + [float(v) for v in quad]
    # the opposite vertex order (the sign of the shoelace sum turns) covers the same pixels
    it2 = R.make_item(0, S, S, 0, 2, [10, 10, 10, 20, 30, 20, 30, 10], *IDENT)
    out2, _, union2, _ = R.compose([sc], [it2], 1, _canvas(), np.zeros((0, 10), np.float32), 0.5)
    assert np.array_equal(union2, union) and np.array_equal(out2, out)


def test_quarter_turn_paste():
    sc = _scene(2)
    # x' = y + 3, y' = -x + 25;  back: x = 25 - y', y = x' - 3
    M, Minv = (0.0, 1.0, 3.0, -1.0, 0.0, 25.0), (0.0, -1.0, 25.0, 1.0, 0.0, -3.0)
    quad = [4, 2, 12, 2, 12, 6, 4, 6]
    it = R.make_item(0, S, S, 0, 1, quad, M, Minv)
    out, tg, union, _ = R.compose([sc], [it], 1, _canvas(), np.zeros((0, 10), np.float32), 0.5)
    assert tg[0, 2:].tolist() == [5, 21, 5, 13, 9, 13, 9, 21]
    ys, xs = np.nonzero(union[0])
    assert (xs.min(), xs.max(), ys.min(), ys.max()) == (5, 9, 13, 21) and len(xs) == 5 * 9
    for x, y in zip(xs, ys):
        assert np.array_equal(out[0, y, x], sc[x - 3, 25 - y])
    assert (out[0][~union[0]] == 7).all()


def test_taps_outside_the_scene_read_the_fill():
    sc = _scene(3, 8, 8)
    it = R.make_item(0, 8, 8, 0, 0, [4, 4, 20, 4, 20, 20, 4, 20], *IDENT)     # the source quad reaches past the 8 x 8 scene
    out, _, union, _ = R.compose([sc], [it], 1, _canvas(), np.zeros((0, 10), np.float32), 0.5)
    assert union[0, 4:21, 4:21].all() and union.sum() == 17 * 17
    assert np.array_equal(out[0, 4:8, 4:8], sc[4:8, 4:8]) and (out[0, 8:21, 4:21] == 114).all() and (out[0, 4:21, 8:21] == 114).all()


def _row(slot, cls, x0, y0, x1, y1):
    return [slot, cls, x0, y0, x1, y0, x1, y1, x0, y1]


def test_rows_covered_fully_and_around_the_threshold():
    sc = _scene(4)
    e = 2.0 ** -20
    tg = np.array([_row(0, 1, 12, 12, 18, 18),                          # inside the item: share 1
                   _row(0, 1, 0, 0, 10, 10),                            # x >= 5 of it covered: share exactly 0.5 -> buried (>=)
                   _row(0, 1, 0 + 2 * e, 0, 10, 10),                    # a little narrower on the uncovered side: just over
                   _row(0, 1, 0 - 2 * e, 0, 10, 10),                    # a little wider there: just under -> kept
                   _row(0, 1, 0, 20, 4, 30),                            # not touched: share 0
                   _row(1, 1, 12, 12, 18, 18),                          # another slot
                   [0, 1] + [np.nan] * 8,                               # already NaN
                   [0, 1, 6, 6, 6, 6, 9, 9, 9, 9]], dtype=np.float32)   # no area
    it = R.make_item(0, S, S, 0, 3, [5, 0, 25, 0, 25, 25, 5, 25], *IDENT)
    out, got, _, _ = R.compose([sc, sc], [it], 2, _canvas(2), tg, 0.5)
    pts = lambda r: [(float(r[2 + 2 * k]), float(r[3 + 2 * k])) for k in range(4)]
    q = R.quad_pts(np.float32([5, 0, 25, 0, 25, 25, 5, 25]))
    assert R.clip_ratio(pts(tg[0]), q) == 1.0 and R.clip_ratio(pts(tg[1]), q) == 0.5
    assert R.clip_ratio(pts(tg[2]), q) > 0.5 > R.clip_ratio(pts(tg[3]), q) > 0.4999999 and R.clip_ratio(pts(tg[4]), q) == 0.0
    buried = np.isnan(got[:, 2:]).all(1)
    assert buried.tolist() == [True, True, True, False, False, False, True, False, False]
    keep = ~buried
    assert got[keep][:-1].tobytes() == tg[[3, 4, 5, 7]].tobytes() and np.array_equal(got[:8, :2], tg[:, :2])
    assert got[8].tolist() == [0.0, 3.0, 5, 0, 25, 0, 25, 25, 5, 25]
    # with a higher threshold the half-covered rows stay
    _, got9, _, _ = R.compose([sc, sc], [it], 2, _canvas(2), tg, 0.9)
    assert np.isnan(got9[:, 2:]).all(1).tolist() == [True, False, False, False, False, False, True, False, False]


def test_two_overlapping_pastes_the_later_wins():
    a, b = _scene(5), _scene(6)
    first = R.make_item(0, S, S, 0, 1, [4, 4, 14, 4, 14, 14, 4, 14], *IDENT)
    later = R.make_item(1, S, S, 0, 2, [6, 2, 20, 2, 20, 16, 6, 16], *IDENT)   # covers 8 / 10 of the first
    out, tg, union, cover = R.compose([a, b], [first, later], 1, _canvas(), np.zeros((0, 10), np.float32), 0.5)
    assert cover[0, 6:15, 4:15].max() == 2 and cover[0, 4:15, 4:6].max() == 1
    assert np.array_equal(out[0, 4:15, 4:6], a[4:15, 4:6])                      # what the later paste leaves of the first
    assert np.array_equal(out[0, 2:17, 6:21], b[2:17, 6:21])                    # the later paste, whole
    assert np.isnan(tg[0, 2:]).all() and tg[0, :2].tolist() == [0.0, 1.0] and not np.isnan(tg[1]).any()
    # the other order: the small one on top, the large one keeps its row (100 of 196 covered... of ITS area 14 x 14: share 80 / 196)
    out2, tg2, _, _ = R.compose([b, a], [R.make_item(0, S, S, 0, 2, later["quad"], *IDENT), R.make_item(1, S, S, 0, 1, first["quad"], *IDENT)], 1,
                                _canvas(), np.zeros((0, 10), np.float32), 0.5)
    assert np.array_equal(out2[0, 4:15, 4:15], a[4:15, 4:15]) and not np.isnan(tg2).any()


def test_items_outside_the_slots_and_dead_quads_are_ignored():
    sc = _scene(7)
    quad = [4, 4, 14, 4, 14, 14, 4, 14]
    items = [R.make_item(0, S, S, -1, 1, quad, *IDENT), R.make_item(0, S, S, 0, 2, [4, 4, 9, 9, 14, 14, 9, 9], *IDENT),
             R.make_item(0, S, S, 1, 3, quad, *IDENT)]
    tg = np.array([_row(0, 0, 5, 5, 10, 10)], dtype=np.float32)
    out, got, union, _ = R.compose([sc], items, 1, _canvas(), tg, 0.5)
    assert not union.any() and np.array_equal(out, _canvas())
    assert got[0].tobytes() == tg[0].tobytes()
    assert got[1, :2].tolist() == [0.0, 1.0] and np.isnan(got[1, 2:]).all()        # slot -1: not valid
    assert got[2].tolist() == [0.0, 2.0, 4, 4, 9, 9, 14, 14, 9, 9]                  # no area: its row stays, it pastes and buries nothing
    assert got[3, :2].tolist() == [0.0, 3.0] and np.isnan(got[3, 2:]).all()        # slot 1 of a batch of 1


# ---------------------------------------------------------------------------------------------- 3. matrices and draws
def test_matrices_are_inverse_and_keep_the_orientation():
    from ryolov4_amd.datasets.copy_paste import paste_matrices
    quad = np.float32([10, 10, 30, 12, 29, 22, 9, 20])
    for angle, sc in ((0.0, 1.0), (90.0, 0.5), (-37.5, 2.0), (179.0, 1.25)):
        M, Minv = paste_matrices(quad, angle, sc, 40.0, 50.0)
        assert (M, Minv) == R.matrices(quad, angle, sc, 40.0, 50.0)
        A, Ai = np.array([M[:3], M[3:], [0, 0, 1]]), np.array([Minv[:3], Minv[3:], [0, 0, 1]])
        assert np.abs(A @ Ai - np.eye(3)).max() < 1e-12
        assert abs(np.linalg.det(A[:2, :2]) - sc * sc) < 1e-12                      # positive: no reflection
        mean = quad.reshape(4, 2).astype(np.float64).mean(0)
        assert np.abs(A @ [mean[0], mean[1], 1.0] - [40.0, 50.0, 1.0]).max() < 1e-12
    M, _ = paste_matrices(quad, 0.0, 1.0, 19.5, 16.0)                               # centre = mean vertex: the identity
    assert M == (1.0, 0.0, 0.0, -0.0, 1.0, 0.0)


def _bank(seed, counts):
    rs = np.random.RandomState(seed)
    bank = {}
    for c, n in counts.items():
        quads = []
        for i in range(min(n, 50)):
            x, y, w, h = rs.uniform(0, 500), rs.uniform(0, 500), rs.uniform(6, 40), rs.uniform(6, 40)
            quads.append((int(c), i, np.float32([x, y, x + w, y, x + w, y + h, x, y + h])))
        bank[float(c)] = quads
    return bank


def test_draws_equal_the_restatement_and_repeat_under_a_seed():
    from ryolov4_amd.datasets.copy_paste import CopyPaste
    counts = {0.0: 5000, 1.0: 300, 2.0: 40, 5.0: 7}
    bank = _bank(1, counts)
    unit = [1.0, 0.5, 2.0, 1.0, 0.8, 1.0, 1.0, 1.25] * 4
    state, nstate = random.getstate(), np.random.get_state()
    kw = dict(p=0.6, max_objects=5, alpha=0.7, scale=(0.5, 2.0), rotate=45.0, min_side=8.0)
    a = CopyPaste(seed=11, **kw).draw(32, 96, bank, counts, unit)
    b = CopyPaste(seed=11, **kw).draw(32, 96, bank, counts, unit)
    c = CopyPaste(seed=12, **kw).draw(32, 96, bank, counts, unit)
    want = R.draw(random.Random(11), 32, 96, bank, counts, unit, **kw)
    key = lambda d: [(t[0], t[1], t[2], t[3], t[5], t[6], t[7], t[8]) for t in d]
    assert key(a) == key(b) == key(want) and key(a) != key(c) and len(a) > 20
    assert random.getstate() == state and all(np.array_equal(u, v) for u, v in zip(np.random.get_state(), nstate))     # the global generators: untouched
    slots = [t[0] for t in a]
    assert slots == sorted(slots) and 0 < len(set(slots)) < 32                      # slot by slot; the coin leaves slots out
    # the skip rule was in force: the draws are the same with min_side = 0, and some of those objects were dropped after they were drawn
    full = key(R.draw(random.Random(11), 32, 96, bank, counts, unit, **dict(kw, min_side=0.0)))
    assert len(full) > len(a) and [t for t in full if t in set(key(a))] == key(a)
    for slot, _, _, cls, quad, angle, sc, cx, cy in a:
        q = quad.astype(np.float64).reshape(4, 2)
        r = sc * np.sqrt(((q - q.mean(0)) ** 2).sum(1)).max()
        assert 2 * r <= 96 and r - 1e-9 <= cx <= 96 - r + 1e-9 and r - 1e-9 <= cy <= 96 - r + 1e-9
        assert sc * min(np.hypot(*(q[(k + 1) % 4] - q[k])) for k in range(4)) >= 8.0 and -45.0 <= angle < 45.0
        assert 0.5 * unit[slot] <= sc <= 2.0 * unit[slot]
    assert CopyPaste(seed=1).draw(8, 64, {}, {}, [1.0] * 8) == []                   # an empty bank draws nothing


def test_class_draw_follows_the_inverse_power_of_the_counts():
    from ryolov4_amd.datasets.copy_paste import CopyPaste
    counts = {0.0: 20000, 1.0: 2500, 3.0: 300, 4.0: 40, 9.0: 5}
    bank = _bank(2, counts)
    alpha = 0.5
    cp = CopyPaste(p=1.0, max_objects=8, alpha=alpha, scale=(1.0, 1.0), rotate=0.0, min_side=0.0, seed=0)
    drawn = cp.draw(3000, 4096, bank, counts, [1.0] * 3000)                        # nothing is skipped at this canvas size
    N = len(drawn)
    assert N > 10000
    w = {c: n ** -alpha for c, n in counts.items()}
    tot = sum(w.values())
    for c in counts:
        p = w[c] / tot
        f = sum(1 for t in drawn if t[3] == c) / N
        sigma = math.sqrt(p * (1 - p) / N)                                        # binomial standard error at this sample size
        print(f"class {c}: expected {p:.4f}, drawn {f:.4f}, {abs(f - p) / sigma:.2f} sigma (N = {N})")
        assert abs(f - p) <= 4.5 * sigma
    # and it is neither uniform nor the raw frequency: the rarest class is drawn most, far from 1 / 5
    assert sum(1 for t in drawn if t[3] == 9.0) / N > 0.5 > 0.2 + 20 * math.sqrt(0.16 / N)
    # alpha = 0 is uniform over the classes present
    cp0 = CopyPaste(p=1.0, max_objects=8, alpha=0.0, scale=(1.0, 1.0), rotate=0.0, min_side=0.0, seed=0)
    d0 = cp0.draw(3000, 4096, bank, counts, [1.0] * 3000)
    for c in counts:
        f = sum(1 for t in d0 if t[3] == c) / len(d0)
        assert abs(f - 0.2) <= 4.5 * math.sqrt(0.16 / len(d0))


def test_argument_errors():
    from ryolov4_amd.datasets.copy_paste import CopyPaste
    for kw in (dict(p=1.5), dict(max_objects=0), dict(scale=(0.0, 1.0)), dict(scale=(2.0, 1.0)), dict(occ_thr=0.0), dict(occ_thr=1.5),
               dict(rotate=-1.0), dict(min_side=-1.0)):
        with pytest.raises(ValueError):
            CopyPaste(**kw)
