"""The Gaussian box regressions (KLD, GWD, ProbIoU; fused-loss modes 3-5) as tests/gauss_loss_ref.py restates them, checked on the CPU in
float64: the closed forms the kernel evaluates against the textbook matrix forms, hand values, and the properties that make these losses
worth having (functions of the Gaussian alone).  The kernel itself is held to the same restatement in tests/test_gpu_gauss_loss.py."""
import math

import pytest
import torch

from tests import gauss_loss_ref as G

PI = math.pi


def _boxes(n, seed):
    """[n, 5] float64: centres within a few cells, w in [0.05, 8.05], h in [0.05, 12.05], theta over the full range [-pi, pi)."""
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(n, 5, generator=g, dtype=torch.float64)
    return torch.stack((r[:, 0] * 6 - 3, r[:, 1] * 6 - 3, 0.05 + 8 * r[:, 2], 0.05 + 12 * r[:, 3], (r[:, 4] * 2 - 1) * PI), 1)


@pytest.fixture(scope="module")
def pairs():
    return _boxes(2000, 1), _boxes(2000, 2)


@pytest.mark.parametrize("kind", G.KINDS)
def test_closed_form_equals_matrix_form(pairs, kind):
    p, t = pairs
    d_mat = G.gauss_distance_matrix(kind, p, t)
    d = G.gauss_distance(kind, p, t)
    lo, hi = (1e-7, 100.0) if kind == "probiou" else (0.0, float("inf"))
    err = (d - d_mat.clamp(min=lo, max=hi)).abs()
    print(kind, "max |closed - matrix| / (1 + |D|):", float((err / (1 + d_mat.abs())).max()))
    assert bool((err <= 1e-10 * (1 + d_mat.abs())).all())
    assert float(d_mat.min()) > 0 and float(d_mat.max()) > 1      # the clamps were inert on most of the range the forms are compared on


def _sq(w, x=0.0, y=0.0):
    return torch.tensor([[x, y, w, w, 0.0]], dtype=torch.float64)


@pytest.mark.parametrize("kind,d0,inc", [("kld", 0.6362944, 0.125), ("gwd", 2.0, 1.0), ("probiou", 0.5 * math.log(1.5625), 0.05)])
def test_hand_values(kind, d0, inc):
    """Concentric axis-aligned squares, prediction w = h = 2 (a = b = 1), target w = h = 4 (a = b = 4); then the centre offset (1, 0)."""
    assert abs(0.5 * math.log(1.5625) - 0.2231436) < 1e-7
    for fn in (G.gauss_distance, G.gauss_distance_matrix):
        d = float(fn(kind, _sq(2.0), _sq(4.0)))
        assert abs(d - d0) < 1e-7, (kind, fn.__name__, d)
        d1 = float(fn(kind, _sq(2.0, 1.0, 0.0), _sq(4.0)))
        assert abs(d1 - d - inc) < 1e-12, (kind, fn.__name__, d1 - d)


@pytest.mark.parametrize("kind", G.KINDS)
def test_distance_of_a_box_to_itself_is_zero(pairs, kind):
    p = pairs[0]
    raw = G.gauss_distance(kind, p, p, clamp=False)
    assert float(raw.abs().max()) <= (0.0 if kind == "kld" else 1e-12), float(raw.abs().max())
    floor = 1e-7 if kind == "probiou" else 0.0                  # ProbIoU's D is clamped to [1e-7, 100]
    assert float((G.gauss_distance(kind, p, p) - floor).abs().max()) <= (0.0 if kind == "kld" else 1e-12)


@pytest.mark.parametrize("kind", G.KINDS)
def test_symmetry(pairs, kind):
    p, t = pairs
    asym = float((G.gauss_distance(kind, p, t) - G.gauss_distance(kind, t, p)).abs().max())
    if kind == "kld":
        assert asym > 1e-3
    else:
        assert asym <= 1e-10 * (1 + float(G.gauss_distance(kind, p, t).abs().max()))


def _swap(b):
    """(w, h, theta) -> (h, w, theta + pi/2): the same rectangle, hence the same Gaussian."""
    return torch.stack((b[:, 0], b[:, 1], b[:, 3], b[:, 2], b[:, 4] + PI / 2), 1)


def _turn(b):
    """theta -> theta + pi."""
    return torch.cat((b[:, :4], b[:, 4:] + PI), 1)


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("fn", [_swap, _turn], ids=["swap_wh_quarter_turn", "half_turn"])
def test_invariant_under_reparametrisation_of_either_box(pairs, kind, fn):
    p, t = pairs
    d = G.gauss_distance(kind, p, t)
    for q, s in ((fn(p), t), (p, fn(t)), (fn(p), fn(t))):
        e = (G.gauss_distance(kind, q, s) - d).abs()
        assert bool((e <= 1e-10 * (1 + d.abs())).all()), float((e / (1 + d.abs())).max())


@pytest.mark.parametrize("kind", G.KINDS)
def test_loss_and_score_ranges(pairs, kind):
    """L in [0, 1) and score = max(1 - L, 0) in (0, 1].  For KLD and GWD that holds for every D >= 0.  ProbIoU's L = sqrt(1 - exp(-D) + 1e-7)
    stays below 1 while exp(-D) > 1e-7, i.e. D < ln 1e7 = 16.1 (boxes that still overlap in any sense); beyond that it saturates at
    sqrt(1 + 1e-7) and the score's max(., 0) makes it 0 — so its open bounds are asserted on the pairs with D < 16 and the closed ones on all."""
    p, t = pairs
    near = t + 1e-3 * (p - t)                                    # nearly identical pairs as well as distant ones
    for a in (p, near, t):
        d = G.gauss_distance(kind, a, t)
        L = G.loss_of_distance(kind, d)
        score = (1 - L).clamp(0)
        assert bool(torch.isfinite(L).all()) and float(L.min()) >= 0.0
        assert float(L.max()) <= math.sqrt(1 + 1e-7) and float(score.min()) >= 0.0 and float(score.max()) <= 1.0
        sel = d < 16 if kind == "probiou" else torch.ones_like(d, dtype=torch.bool)
        assert int(sel.sum()) > 500
        assert float(L[sel].max()) < 1.0 and float(score[sel].min()) > 0.0
    # the loss grows with the distance
    d = torch.linspace(1e-7, 16, 1000, dtype=torch.float64)
    assert bool((G.loss_of_distance(kind, d).diff() > 0).all())


def test_make_loss_and_the_table_of_losses():
    """ryolov4_amd.lib.loss imports without a device (tests/test_dropin_imports.py relies on the same); constructing a criterion launches
    nothing."""
    from oracle import ref_ops
    from ryolov4_amd.lib import loss as L
    from ryolov4_amd.synth import CFG, HYP
    assert set(L.LOSSES) == {"csl", "kfiou", "sl1iou", "kld", "gwd", "probiou"}
    assert (L.LOSSES["csl"], L.LOSSES["kfiou"], L.LOSSES["sl1iou"]) == (L.ComputeCSLLoss, L.ComputeKFIoULoss, L.ComputeSL1IoULoss)
    assert (L.LOSSES["kld"], L.LOSSES["gwd"], L.LOSSES["probiou"]) == (L.ComputeKLDLoss, L.ComputeGWDLoss, L.ComputeProbIoULoss)
    assert [L.LOSSES[k].MODE for k in ("csl", "kfiou", "sl1iou", "kld", "gwd", "probiou")] == [0, 1, 2, 3, 4, 5]

    class M:
        pass
    m = M()
    m.anchors, m.nc = ref_ops.make_anchors(CFG, "kfiou"), 3
    for name in ("kld", "gwd", "probiou"):
        crit = L.make_loss(name, m, HYP)
        assert type(crit) is L.LOSSES[name] and isinstance(crit, L._ComputeLossBase)
        assert crit.KEYS == L.ComputeKFIoULoss.KEYS and set(crit.loss_items) == set(crit.KEYS)
    with pytest.raises(ValueError) as ei:
        L.make_loss("giou", m, HYP)
    for name in L.LOSSES:
        assert name in str(ei.value)
