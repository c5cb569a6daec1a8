"""CPU tests of the ignore regions: the restatement tests/ignore_ref.py on cases small enough to check by hand, the validation of the
loader's Ignore option, the layout of the three LossParams fields the feature appended, and — so that the GPU tests of
tests/test_gpu_loss_ignore.py cannot be vacuous — that the quads of tests/ignore_cases.py ignore some but not all cells of every scale and
lie over matched cells."""
import ctypes as C

import numpy as np
import pytest

from tests import ignore_cases as K
from tests import ignore_ref as R

NAN = float("nan")


def _row(img, *q):
    return np.array([img] + list(q), dtype=np.float32)


def test_edge_through_a_centre_is_inside():
    # gs 4: the quad [1.5, 3] x [0.5, 2] in grid units; its left edge x = 1.5 passes through the centres of column 1, its top edge
    # y = 0.5 through the centres of row 0; x = 3 and y = 2 pass between centres
    row = _row(0, 1.5 / 4, 0.5 / 4, 3 / 4, 0.5 / 4, 3 / 4, 2 / 4, 1.5 / 4, 2 / 4)
    want = np.zeros((4, 4), dtype=bool)
    want[0:2, 1:3] = True                                          # rows 0, 1 (centres 0.5, 1.5), columns 1, 2 (centres 1.5, 2.5)
    assert R.row_live(row, 1, 4) and np.array_equal(R.row_cells(row, 4), want)
    # moved right by a quarter cell the centres of column 1 fall outside
    row2 = _row(0, 1.75 / 4, 0.5 / 4, 3 / 4, 0.5 / 4, 3 / 4, 2 / 4, 1.75 / 4, 2 / 4)
    want[:, 1] = False
    assert np.array_equal(R.row_cells(row2, 4), want)


def test_diamond_and_both_orientations():
    # gs 8: centre (4.5, 3.5) — a cell centre — and |dx| + |dy| <= 2: 13 cells, the four tips on the boundary
    q = [2.5 / 8, 3.5 / 8, 4.5 / 8, 1.5 / 8, 6.5 / 8, 3.5 / 8, 4.5 / 8, 5.5 / 8]
    a = R.row_cells(_row(0, *q), 8)
    want = np.zeros((8, 8), dtype=bool)
    for gj in range(8):
        for gi in range(8):
            want[gj, gi] = abs(gi + 0.5 - 4.5) + abs(gj + 0.5 - 3.5) <= 2
    assert want.sum() == 13 and np.array_equal(a, want)
    rev = [v for k in (0, 3, 2, 1) for v in q[2 * k:2 * k + 2]]
    x, y = R.grid_quad(_row(0, *q), 8)
    xr, yr = R.grid_quad(_row(0, *rev), 8)
    assert R.shoelace(x, y) == -R.shoelace(xr, yr) != 0
    assert np.array_equal(R.row_cells(_row(0, *rev), 8), want)


def test_dead_rows_cover_nothing():
    full = [0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0]
    assert R.covered(_row(0, *full)[None], 2, 3)[0].all() and not R.covered(_row(0, *full)[None], 2, 3)[1].any()
    dead = [_row(-1, *full), _row(2, *full), _row(NAN, *full), _row(0, *(full[:5] + [NAN] + full[6:])), _row(0, *(full[:2] + [float("inf")] + full[3:])),
            _row(0, *([0.25, 0.5] * 4)),                               # a point
            _row(0, 0.0, 0.0, 0.5, 0.5, 1.0, 1.0, 0.25, 0.25),         # four points on one line
            _row(0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 1.0)]           # a symmetric bow tie: the two lobes cancel
    for r in dead:
        assert not R.row_live(r, 2, 3), r
    assert not R.covered(np.stack(dead), 2, 3).any()
    assert R.row_live(_row(-0.5, *full), 2, 3) and R.row_live(_row(1.9, *full), 2, 3)      # (int) truncates toward zero
    assert R.covered(_row(1.9, *full)[None], 2, 3)[1].all()
    # wholly outside the grid: live, and covers nothing
    out = _row(0, 1.25, 0.0, 1.5, 0.0, 1.5, 1.0, 1.25, 1.0)
    assert R.row_live(out, 2, 3) and not R.covered(out[None], 2, 3).any()


def test_ignored_leaves_matched_cells_and_counts_every_anchor():
    full = _row(1, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0)[None]
    rec = np.array([[1, 2, 0, 1, 0, 0, 0, 0], [0, 0, 1, 1, 0, 0, 0, 0]])
    m = R.ignored(full, 2, 3, 2, rec)
    assert m.shape == (2, 3, 2, 2) and not m[0].any() and m[1].sum() == 11 and not m[1, 2, 0, 1]


def test_objectness_element():
    x = np.array([-3.0, 0.0, 2.5])
    np.testing.assert_allclose(R.obj_element(x), np.log1p(np.exp(x)), rtol=1e-15)
    p = 1 / (1 + np.exp(-x))
    np.testing.assert_allclose(R.obj_element(x, 1.5), np.log1p(np.exp(x)) * 0.75 * p ** 1.5, rtol=1e-15)
    logits, masks = [np.array([[0.0, 1.0], [2.0, -1.0]])], [np.array([[True, False], [False, True]])]
    plain = 0.7 * float(np.log1p(np.exp(logits[0])).sum()) / 4
    want = 0.7 * float(np.log1p(np.exp(np.array([1.0, 2.0]))).sum()) / 4
    assert abs(R.conf_without(plain, 0.7, logits, masks) - want) < 1e-15 and abs(R.conf_no_targets(0.7, logits, masks) - want) < 1e-15


@pytest.mark.parametrize("mode", ["csl", "kfiou"])
@pytest.mark.parametrize("empty", [False, True], ids=["targets", "no_targets"])
def test_the_gpu_cases_are_not_vacuous(mode, empty):
    ig = K.ignore_table().numpy()
    tg = K.targets(mode, empty)
    assert tg.shape[0] == (0 if empty else 12)
    recs = K.cpu_matches(mode, tg)
    under = 0
    for i, gs in enumerate(K.GS):
        m = R.ignored(ig, K.B, K.NA[mode], gs, recs[i])
        assert 0 < m.sum() < m.size, (gs, m.sum())
        assert 0 < m[0].sum() < m[0].size and m[1].sum() > 0                # image 0 partly; image 1 under the whole-image quad
        cov = R.covered(ig, K.B, gs)
        under += int((np.broadcast_to(cov[:, None], m.shape) & R.matched_mask(recs[i], K.B, K.NA[mode], gs)).sum())
    assert empty or under > 0                                               # a matched cell under a quad keeps its bits
    assert empty or R.matched_mask(recs[0], K.B, K.NA[mode], 12)[0, :, 3, 6].any()       # the target the last quad was laid over
    for what, img, q in K.QUADS:
        row = np.array([img] + q, dtype=np.float32)
        for gs in K.GS:
            n = int(R.covered(row[None], K.B, gs).sum())
            assert (n == 0) == (what in K.DEAD), (what, gs, n)
    a = R.covered(np.array([[0.0] + K.DIAMOND], dtype=np.float32), 1, 12)
    b = R.covered(np.array([[0.0] + K.QUADS[2][2]], dtype=np.float32), 1, 12)
    assert a.sum() > 0 and np.array_equal(a, b)
    # x = 1/8 at gs 12: column 1's centres lie on the first quad's left edge and count
    assert R.covered(np.array([[0.0] + K.QUADS[0][2]], dtype=np.float32), 1, 12)[0, 3:8, 1].all()


def test_selection_rule():
    # window (0, 0, 96): A whole, B 40 % inside, C 5 % inside, D whole and difficult
    polys = np.array([[10, 10, 30, 10, 30, 30, 10, 30], [88, 40, 108, 40, 108, 60, 88, 60], [95, 70, 115, 70, 115, 90, 95, 90],
                      [50, 50, 70, 50, 70, 70, 50, 70]], dtype=np.float32)
    diff = [0, 0, 0, 1]
    assert R.select(polys, diff, 0, 0, 96, 0.1, 0.7, True) == ([0], [1, 3])
    assert R.select(polys, diff, 0, 0, 96, 0.1, 0.7, False) == ([0, 3], [1])
    assert R.select(polys, diff, 0, 0, 96, 0.01, 0.7, False) == ([0, 3], [1, 2])


def test_vertex_path_by_hand():
    poly = np.array([100, 200, 148, 200, 148, 248, 100, 248], dtype=np.float32)
    # window origin (100, 200), side 48, resized to 96: coordinates double; no pad, no warp
    got = R.vertex_path(poly, 100, 200, 48, (96, 96), (0.0, 0.0), None, 0, 96)
    np.testing.assert_allclose(got, [0, 0, 1, 0, 1, 1, 0, 1], atol=0)
    M = np.array([[1.0, 0, 24], [0, 1.0, 0], [0, 0, 1]])
    got = R.vertex_path(poly, 100, 200, 96, (96, 96), (12.0, 0.0), M, 1, 96)      # half size, 12 rows of pad, 24 px right, flipped left-right
    np.testing.assert_allclose(got, [0.75, 0.125, 0.25, 0.125, 0.25, 0.625, 0.75, 0.625], atol=1e-15)


def test_ignore_option_validation():
    from ryolov4_amd.datasets.scene_dataset import Ignore, check_ignore
    assert check_ignore(None, 0.7) is None
    ig = check_ignore({"iof_lo": 0.2, "difficult": False}, 0.7)
    assert ig == Ignore(0.2, False) and repr(ig) == "Ignore(iof_lo=0.2, difficult=False)"
    assert check_ignore(Ignore(), 0.7) == Ignore(0.1, True)
    for bad in ({"iof_lo": 0.0}, {"iof_lo": 0.7}, {"iof_lo": 0.9}, {"iof_lo": NAN}, {"iof_lo": True}, {"iof_lo": "0.1"}, {"difficult": 1},
                {"difficult": None}, {"margin": 2}, 0.1, "on"):
        with pytest.raises(ValueError):
            check_ignore(bad, 0.7)
    with pytest.raises(ValueError):
        Ignore(-0.1)
    ig = Ignore(0.1)
    ig.iof_lo = 0.8                                                 # set after construction: checked again
    with pytest.raises(ValueError):
        check_ignore(ig, 0.7)


def test_loss_params_gained_three_fields_at_the_end():
    from ryolov4_amd import abi
    t = abi.STRUCTS["LossParams"]
    before = [("mode", 0), ("nc", 4), ("na", 8), ("batch", 12), ("nt", 16), ("tcols", 20), ("targets", 24), ("head", 32), ("grad", 56), ("gs", 80),
              ("anchors", 92), ("box", 740), ("obj", 744), ("cls", 748), ("theta_gain", 752), ("obj_pw", 756), ("cls_pw", 760), ("ws", 768),
              ("ws_bytes", 776), ("items", 784), ("compute_grad", 792), ("fl_gamma", 796), ("fl_alpha", 800), ("objgrad", 808), ("headobj", 832)]
    got = [(f, getattr(t, f).offset) for f, _ in t._fields_]
    assert got[:len(before)] == before
    assert got[len(before):] == [("ignore", 856), ("ni", 864), ("ign_count", 872)] and C.sizeof(t) == 880
    kinds = dict(t._fields_)
    assert kinds["ignore"] is C.c_void_p and kinds["ni"] is C.c_int and kinds["ign_count"] is C.c_void_p
    z = t()                                                         # a zeroed block means "no ignore rows"
    assert not z.ignore and z.ni == 0 and not z.ign_count
