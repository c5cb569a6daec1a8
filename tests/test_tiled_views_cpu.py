"""CPU tests of the flip / 90-degree views of full-scene detection (lib/tiled.py VIEWS, tile_entries, TiledDetector(views=...)): argument
validation, entry order and slot numbering, and the host restatements the GPU tests rely on (tests/views_ref.py) checked against each
other: the pixel definition against the point map at pixel centres, and the box map against oracle.ref_data.xywha2xyxyxyxy (polygon
identity).  No GPU needed."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ryolov4_amd.lib import tiled
from tests import views_ref as V


def test_views_constant():
    assert tiled.VIEWS == V.NAMES and len(set(tiled.VIEWS)) == 8


class _FakeModel:
    training = False

    def capture_inference(self, batch, size, post=None):
        def run(imgs):
            raise AssertionError("not replayed here")
        run.static_input = torch.zeros((batch, 3, size, size))
        run.post_plan = SimpleNamespace(nc=3, mk=10)
        return run


@pytest.mark.parametrize("views", [(), ("id", "id"), ("hflip", "rot90", "hflip"), ("flip",), ("id", "ROT90"), "id", (0,), ("id", None)])
def test_views_rejected(views):
    with pytest.raises(ValueError):
        tiled.check_views(views)
    with pytest.raises(ValueError):
        tiled.TiledDetector(_FakeModel(), size=64, overlap=16, batch=2, views=views)
    with pytest.raises(ValueError):
        tiled.tile_entries(100, 100, 64, 16, (1.0,), views)


def test_views_accepted_and_default():
    assert tiled.TiledDetector(_FakeModel(), size=64, overlap=16, batch=2).views == ("id",)
    det = tiled.TiledDetector(_FakeModel(), size=64, overlap=16, batch=2, views=["rot270", "id", "antitranspose"])
    assert det.views == ("rot270", "id", "antitranspose")                      # the order given is kept
    assert tiled.TiledDetector(_FakeModel(), size=64, overlap=16, batch=2, views=tiled.VIEWS).views == tiled.VIEWS


def test_entry_order_and_slots_two_rates_three_views():
    H, W, S, ov, rates, views, mk = 300, 420, 128, 32, (1.0, 0.5), ("rot90", "id", "vflip"), 7
    windows = tiled.tile_plan(H, W, S, ov, rates)
    entries = tiled.tile_entries(H, W, S, ov, rates, views)
    assert {w[0] for w in windows} == {0, 1} and len(windows) > 4
    assert len(entries) == len(windows) * 3
    for wi, (ri, x0, y0) in enumerate(windows):
        for vi, v in enumerate(views):
            assert entries[wi * 3 + vi] == (ri, x0, y0, v)                     # window-major, views in the order given
    slots = [e * mk + j for e in range(len(entries)) for j in range(mk)]
    assert slots == list(range(len(entries) * mk))                             # slot e * mk + j: dense, entry order = slot order
    assert tiled.tile_plan(H, W, S, ov, rates) == [e[:3] for e in entries[::3]]   # tile_plan keeps returning (rate_index, x0, y0)
    assert tiled.tile_entries(H, W, S, ov, rates) == [w + ("id",) for w in windows]


@pytest.mark.parametrize("name", V.NAMES)
@pytest.mark.parametrize("S", [8, 12])
def test_pixel_definition_matches_point_map_at_centres(name, S):
    """The view's pixel (iy, ix) is the window pixel under the mapped centre (ix + 0.5, iy + 0.5): pixel i covers [i, i + 1)."""
    win = np.random.RandomState(S).randint(0, 256, (S, S, 3)).astype(np.uint8)
    v = V.view_pixels(win, name)
    assert v.shape == win.shape
    iy, ix = np.mgrid[0:S, 0:S]
    px, py = V.point_map(name, ix + 0.5, iy + 0.5, float(S))
    assert (px % 1 == 0.5).all() and (py % 1 == 0.5).all()
    assert np.array_equal(v, win[np.floor(py).astype(int), np.floor(px).astype(int)])


def test_view_pixels_by_hand():
    win = np.arange(4, dtype=np.uint8).reshape(2, 2, 1).repeat(3, 2)            # [[0, 1], [2, 3]]
    exp = {"id": [[0, 1], [2, 3]], "hflip": [[1, 0], [3, 2]], "vflip": [[2, 3], [0, 1]], "rot180": [[3, 2], [1, 0]],
           "transpose": [[0, 2], [1, 3]], "rot90": [[1, 3], [0, 2]], "rot270": [[2, 0], [3, 1]], "antitranspose": [[3, 1], [2, 0]]}
    for name in V.NAMES:
        assert V.view_pixels(win, name)[:, :, 0].tolist() == exp[name], name


@pytest.mark.parametrize("name", V.NAMES)
@pytest.mark.parametrize("S", [64, 1024])
def test_polygon_identity_and_angle_range(name, S):
    """The polygon of the mapped box is the mapped polygon of the view's box (as a vertex set) within 1e-2 px: the smallest real
    mistake, S - 1 - x for S - x, is 1 px, and fp32 rounding at these sizes stays below 1e-3 px.  theta of the six mapped views lands in
    [-pi/2, pi/2) for every theta kfiou decode can produce (|theta| < pi/2 + 0.27)."""
    rng = np.random.RandomState(7)
    n = 50
    rows = np.zeros((n, 7), dtype=np.float32)
    rows[:, 0:2] = rng.uniform(0, S, (n, 2))
    rows[:, 2] = rng.uniform(2, S / 4, n)
    rows[:, 3] = rows[:, 2] + rng.uniform(0, S / 4, n)                          # h the long side
    rows[:, 4] = rng.uniform(-np.pi / 2 - 0.26, np.pi / 2 + 0.26, n)
    rows[:5, 4] = [V.HALF_PI, -V.HALF_PI, 0.0, np.nextafter(V.HALF_PI, np.float32(0)), np.nextafter(-V.HALF_PI, np.float32(-2))]
    assert V.polygon_gap(rows, name, S) < 1e-2
    m = V.map_rows(rows, name, S)
    assert np.array_equal(m[:, 2:4], rows[:, 2:4]) and np.array_equal(m[:, 5:], rows[:, 5:])     # w, h never swapped
    if name in ("id", "rot180"):
        assert np.array_equal(m[:, 4].view(np.uint32), rows[:, 4].view(np.uint32))              # no wrap: bits unchanged
    else:
        assert (m[:, 4] >= -V.HALF_PI).all() and (m[:, 4] < V.HALF_PI).all()
    # the mistake the bound is sized for is caught
    if name != "id":
        off = rows.copy()
        off[:, 0] += 1.0
        a = V.polygon(V.map_rows(off, name, S))
        b = V.polygon(V.map_rows(rows, name, S))
        assert np.abs(a - b).max() > 0.9
