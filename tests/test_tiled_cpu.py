"""CPU tests of the full-scene window plan (lib/tiled.py tile_plan): against a short independent restatement, and its properties
(coverage, bounds, no duplicates, row-major order, argument validation).  No GPU needed."""
import numpy as np
import pytest

from ryolov4_amd.lib.tiled import resized_extent, tile_plan


def _ref_plan(H, W, size, overlap, rates):
    """Restatement: starts k * stride while the window still ends inside the axis, then one window flush with the end."""
    def axis(L):
        if L <= size:
            return [0]
        n = -(-(L - size) // (size - overlap))           # windows k * stride with k * stride + size < L: k < (L - size) / stride
        return [k * (size - overlap) for k in range(n)] + [L - size]
    out = []
    for ri, r in enumerate(rates):
        h, w = int(H * r + 0.5), int(W * r + 0.5)
        out += [(ri, x, y) for y in axis(h) for x in axis(w)]
    return out


CASES = [
    (4000, 4000, 1024, 200, (1.0,)),
    (1001, 777, 256, 64, (1.0,)),
    (777, 1001, 256, 0, (1.0,)),
    (1001, 777, 256, 224, (1.0,)),             # overlap = size - 32
    (256, 256, 256, 32, (1.0,)),               # equal to size
    (100, 300, 256, 32, (1.0,)),               # smaller along one axis
    (300, 100, 256, 32, (1.0,)),
    (50, 60, 128, 0, (1.0,)),                  # smaller along both
    (257, 255, 256, 0, (1.0,)),
    (4000, 4000, 1024, 200, (1.0, 0.5)),       # two rates
    (1001, 777, 128, 32, (0.5, 1.5)),
    (700, 520, 256, 96, (1.0, 0.5)),
]


@pytest.mark.parametrize("H,W,size,overlap,rates", CASES)
def test_tile_plan_matches_restatement(H, W, size, overlap, rates):
    assert tile_plan(H, W, size, overlap, rates) == _ref_plan(H, W, size, overlap, rates)


def test_tile_plan_known_answers():
    assert tile_plan(4000, 4000, 1024, 200) == [(0, x, y) for y in (0, 824, 1648, 2472, 2976) for x in (0, 824, 1648, 2472, 2976)]
    assert tile_plan(100, 3000, 1024, 200) == [(0, 0, 0), (0, 824, 0), (0, 1648, 0), (0, 1976, 0)]
    assert tile_plan(1025, 1024, 1024, 0) == [(0, 0, 0), (0, 0, 1)]
    assert tile_plan(800, 900, 1024, 200, (1.0, 2.0)) == [(0, 0, 0), (1, 0, 0), (1, 776, 0), (1, 0, 576), (1, 776, 576)]
    assert resized_extent(1001, 777, 0.5) == (501, 389)


@pytest.mark.parametrize("H,W,size,overlap,rates", CASES)
def test_tile_plan_properties(H, W, size, overlap, rates):
    plan = tile_plan(H, W, size, overlap, rates)
    assert len(plan) == len(set(plan)), "duplicate windows"
    assert plan == sorted(plan, key=lambda t: (t[0], t[2], t[1])), "not row-major by (rate, y0, x0)"
    for ri, r in enumerate(rates):
        h, w = resized_extent(H, W, r)
        cover = np.zeros((h, w), dtype=bool)
        for (q, x0, y0) in plan:
            if q != ri:
                continue
            assert x0 >= 0 and y0 >= 0
            assert x0 + size <= w or (x0 == 0 and w < size)       # inside the resized extent unless the scene is smaller than a window
            assert y0 + size <= h or (y0 == 0 and h < size)
            cover[y0:y0 + size, x0:x0 + size] = True
        assert cover.all(), "a pixel is not covered"
        xs = sorted({x for q, x, _ in plan if q == ri})
        assert all(b - a <= size - overlap for a, b in zip(xs, xs[1:])), "gap between windows"


@pytest.mark.parametrize("args", [
    (100, 100, 100, 0), (100, 100, 0, 0), (100, 100, -32, 0), (100, 100, 96, 96), (100, 100, 96, -1), (100, 100, 96, 200),
    (100, 100, 128, 0, (0.0,)), (100, 100, 128, 0, (-1.0,)), (100, 100, 128, 0, ()), (0, 100, 128, 0), (100, 0, 128, 0),
    (100, 100, 128, 0, (float("nan"),)), (100, 100, 128.0, 0),
])
def test_tile_plan_rejects_bad_arguments(args):
    with pytest.raises(ValueError):
        tile_plan(*args)


def test_detector_keeps_the_model_alive():
    """The captured graph replays into the model's runtime buffers, and the callable capture_inference returns does not reference the
    model: the detector must hold it, or the buffers are freed (and handed back to the driver by the next graph capture's empty_cache)
    under a graph that still writes them."""
    import gc
    import weakref
    from types import SimpleNamespace

    import torch
    from ryolov4_amd.lib.tiled import TiledDetector

    class FakeModel:
        training = False

        def capture_inference(self, batch, size, post=None):
            def run(imgs):
                raise AssertionError("not replayed here")
            run.static_input = torch.zeros((batch, 3, size, size))
            run.post_plan = SimpleNamespace(nc=3, mk=10)
            return run

    m = FakeModel()
    ref = weakref.ref(m)
    det = TiledDetector(m, size=64, overlap=16, batch=2)
    del m
    gc.collect()
    assert ref() is not None and det.model is ref()
