"""Ignore regions of the fused loss on the GPU (csrc/loss.hip: loss_ignore_kernel marks, loss_obj_kernel skips) against the numpy
restatement tests/ignore_ref.py.  The reference has no ignore regions; the rule is this build's (include/ryolo.h, ryolo_loss).

Inputs: tests/ignore_cases.py — B = 2, nc = 3, grids (12, 6, 3), modes csl (na 3) and kfiou (na 18), a dozen targets or none, and
twelve rows whose vertices are multiples of 1/8.  Every call with rows is held against its TWIN, the same call without: every gradient
element bit-equal except the objectness element of the cells the restatement marks and the match records show unmatched, which are exactly
0.0; reg / cls / theta bit-equal; conf within 1e-4 relative of the float64 restatement (the bound tests/test_gpu_gauss_loss.py uses for
items) and — since bce_val(-1e4, 0) = -1e4 + (log1p(exp(-1e4)) + 1e4) is exactly 0.0f — bit-equal to a plain call whose objectness
logits at the ignored cells are -1e4."""
import numpy as np
import pytest
import torch

from tests import ignore_cases as K
from tests import ignore_ref as R
from ryolov4_amd.synth import CFG, HYP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ITEM_KEYS = ("reg_loss", "conf_loss", "cls_loss", "theta_loss", "total_loss")


def _crit(mode, hyp=HYP):
    from ryolov4_amd.lib import loss as L
    return L.LOSSES[mode](K.Model(mode), hyp)


def _call(crit, outs, tg, ignore, grad=True):
    o = [x.to(DEV).requires_grad_(grad) for x in outs]
    if grad:
        loss, items = crit(o, tg.to(DEV), ignore=ignore)
        loss.backward()
    else:
        with torch.no_grad():
            loss, items = crit(o, tg.to(DEV), ignore=ignore)
    return loss, dict(items), [x.grad for x in o], crit.ignored_cells.cpu().numpy().copy()


def _check(mode, empty, hyp=HYP):
    gamma = float(hyp.get("fl_gamma", 0.0))
    outs, tg, ig = K.heads(mode), K.targets(mode, empty), K.ignore_table()
    och, na = K.OCH[mode], K.NA[mode]
    crit = _crit(mode, hyp)
    l0, it0, g0, n0 = _call(crit, outs, tg, None)
    assert not n0.any()
    l1, it1, g1, n1 = _call(crit, outs, tg, ig)
    recs = crit.debug_matches()
    assert [len(r) for r in recs] == [len(r) for r in K.cpu_matches(mode, tg)]
    masks = [R.ignored(ig.numpy(), K.B, na, gs, recs[i]) for i, gs in enumerate(K.GS)]
    under = 0
    for i, gs in enumerate(K.GS):
        m = torch.from_numpy(masks[i])
        assert 0 < int(m.sum()) < m.numel()                         # (not vacuous: checked on the CPU too, tests/test_ignore_ref_cpu.py)
        a, b = g0[i].cpu(), g1[i].cpu()
        keep = torch.ones_like(a, dtype=torch.bool)
        keep[..., och][m] = False
        assert torch.equal(a[keep].view(torch.int32), b[keep].view(torch.int32)), (mode, gs)
        ign = b[..., och][m]
        assert bool((ign.view(torch.int32) == 0).all()), (mode, gs)          # exactly +0.0
        assert bool((a[..., och][m] != 0).all())                              # (the twin's elements there were not zero: the feature acted)
        mm = torch.from_numpy(np.broadcast_to(R.covered(ig.numpy(), K.B, gs)[:, None], masks[i].shape) & R.matched_mask(recs[i], K.B, na, gs))
        under += int(mm.sum())
        assert torch.equal(a[mm].view(torch.int32), b[mm].view(torch.int32))  # whole rows of the matched cells under a quad
        assert int(n1[i]) == int(m.sum()), (mode, gs, n1, int(m.sum()))
    assert empty or under > 0
    for k in ("reg_loss", "cls_loss", "theta_loss"):
        if k in it0:
            assert np.float32(it0[k]).tobytes() == np.float32(it1[k]).tobytes(), (k, it0[k], it1[k])
    logits = [x[..., och].numpy() for x in outs]
    want = R.conf_without(it0["conf_loss"], hyp["obj"], logits, masks, gamma)
    print(mode, "empty" if empty else "targets", "gamma", gamma, "conf plain", it0["conf_loss"], "with rows", it1["conf_loss"], "restated", want)
    assert it1["conf_loss"] < it0["conf_loss"]
    assert abs(it1["conf_loss"] - want) < 1e-4 * max(1.0, abs(want)), (it1["conf_loss"], want)
    if empty:
        whole = R.conf_no_targets(hyp["obj"], logits, masks, gamma)
        assert abs(it1["conf_loss"] - whole) < 1e-4 * max(1.0, abs(whole)), (it1["conf_loss"], whole)
    tot = want + sum(it0[k] for k in ("reg_loss", "cls_loss", "theta_loss") if k in it0)
    assert abs(it1["total_loss"] - tot) < 1e-4 * max(1.0, abs(tot)) and abs(float(l1) - tot) < 1e-4 * max(1.0, abs(tot))
    return crit, outs, tg, ig, masks, it1, g1


@pytest.mark.parametrize("empty", [False, True], ids=["targets", "no_targets"])
@pytest.mark.parametrize("mode", ["csl", "kfiou"])
def test_against_the_plain_twin(mode, empty):
    crit, outs, tg, ig, masks, it1, g1 = _check(mode, empty)
    # the same numbers from a plain call whose objectness logits at the ignored cells are -1e4 (value exactly 0 there), bit for bit
    och = K.OCH[mode]
    low = [x.clone() for x in outs]
    for x, m in zip(low, masks):
        x[..., och][torch.from_numpy(m)] = -1e4
    _, it2, _, _ = _call(_crit(mode), low, tg, None, grad=False)
    for k in ITEM_KEYS:
        if k in it1:
            assert np.float32(it1[k]).tobytes() == np.float32(it2[k]).tobytes(), (k, it1[k], it2[k])
    # evaluation (compute_grad == 0) gives the same items and counts
    _, it3, _, n3 = _call(_crit(mode), outs, tg, ig, grad=False)
    assert it3 == it1 and [int(v) for v in n3] == [int(m.sum()) for m in masks]


@pytest.mark.parametrize("mode", ["csl", "kfiou"])
def test_focal_loss(mode):
    _check(mode, False, dict(HYP, fl_gamma=1.5))


@pytest.mark.parametrize("mode", ["csl", "kfiou", "sl1iou", "kld", "gwd", "probiou"])
def test_empty_table_is_the_plain_call(mode):
    base = "csl" if mode == "csl" else "kfiou"
    outs, tg = K.heads(base), K.targets(base)
    l0, it0, g0, n0 = _call(_crit(mode), outs, tg, None)
    l1, it1, g1, n1 = _call(_crit(mode), outs, tg, torch.empty(0, 9))
    assert torch.equal(l0, l1) and it0 == it1 and not n0.any() and not n1.any()
    for a, b in zip(g0, g1):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # every mode takes rows: objectness is shared
    crit = _crit(mode)
    l2, it2, g2, n2 = _call(crit, outs, tg, K.ignore_table())
    recs = crit.debug_matches()
    assert [int(v) for v in n2] == [int(R.ignored(K.ignore_table().numpy(), K.B, K.NA[base], gs, recs[i]).sum()) for i, gs in enumerate(K.GS)]
    assert it2["conf_loss"] < it0["conf_loss"] and it2["reg_loss"] == it0["reg_loss"]


def test_bad_shape_raises_before_a_launch():
    crit = _crit("kfiou")
    outs, tg = [x.to(DEV) for x in K.heads("kfiou")], K.targets("kfiou").to(DEV)
    gen = crit._gen
    for bad in (torch.zeros(4, 8), torch.zeros(9), torch.zeros(2, 3, 9), torch.zeros(4, 9, dtype=torch.int32), [[0.0] * 9]):
        with pytest.raises(RuntimeError, match="ignore must be a float tensor"):
            crit(outs, tg, ignore=bad)
    assert crit._gen == gen and crit._ws is None                  # nothing was allocated or launched


def test_through_the_engine():
    """Yolo(kfiou) yolov4, batch 4 at 128 x 128 (as tests/test_gpu_gauss_loss.py builds it): forward + loss + backward with ignore rows through
    the compact headobj / objgrad hand-over."""
    import bench
    from ryolov4_amd.lib.loss import make_loss
    from ryolov4_amd.model.yolo import Yolo
    from ryolov4_amd.synth import synth_batch
    torch.manual_seed(42)
    m = Yolo(2, CFG, "kfiou", "yolov4")
    m.apply(bench.weights_init_normal)
    m.to(DEV).train()
    crit = make_loss("kfiou", m, HYP)
    imgs, tg = synth_batch(4, 128, 2, False, seed=42)
    imgs, tg = imgs.to(DEV), tg.to(DEV)
    ig = torch.tensor([[0.0, 1 / 8, 1 / 8, 7 / 8, 1 / 8, 7 / 8, 6 / 8, 1 / 8, 6 / 8],
                       [2.0, 4 / 8, 0.0, 1.0, 4 / 8, 4 / 8, 1.0, 0.0, 4 / 8],
                       [3.0, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0],
                       [4.0, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0]])
    na, attrs = 18, 8
    bias = {}
    for tag, rows in (("rows", ig), ("plain", None)):
        m.zero_grad(set_to_none=True)
        outs = m(imgs, training=True)
        dense = {}
        for i, o in enumerate(outs):
            o.register_hook(lambda g, i=i: dense.__setitem__(i, g.clone()))
        loss, items = crit(outs, tg, ignore=rows)
        assert crit._compact is not None and all(crit._used_head_obj)
        compact = crit._compact[0]
        counts = crit.ignored_cells
        loss.backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
        for i in range(3):                                           # compact objectness gradient == the dense map's objectness channel
            assert torch.equal(compact[i].view(torch.int32), dense[i][..., 5].contiguous().view(torch.int32))
        if rows is not None:
            recs = crit.debug_matches()
            for i, o in enumerate(outs):
                gs = o.shape[2]
                mk = R.ignored(ig.numpy(), 4, na, gs, recs[i])
                assert 0 < mk.sum() < mk.size and int(counts[i]) == int(mk.sum())
                assert bool((dense[i][..., 5].cpu()[torch.from_numpy(mk)].view(torch.int32) == 0).all())
        else:
            assert not counts.cpu().numpy().any()
        bias[tag] = [p.grad.detach().clone().view(na, attrs) for n, p in m.named_parameters() if n.endswith("bias") and p.numel() == na * attrs]
        assert len(bias[tag]) == 3
    for a, b in zip(bias["rows"], bias["plain"]):
        assert not torch.equal(a[:, 5], b[:, 5])                    # the feature reaches the weights
        assert torch.equal(a[:, 6:].view(torch.int32), b[:, 6:].view(torch.int32))      # the class channels do not notice
