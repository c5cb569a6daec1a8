"""The Gaussian box regressions of the fused loss on the GPU: modes 3 KLD, 4 GWD, 5 ProbIoU of csrc/loss.hip
(ComputeKLDLoss / ComputeGWDLoss / ComputeProbIoULoss) against tests/gauss_loss_ref.py in float64.  NO REFERENCE ORACLE EXISTS for these
modes — the reference has no code for them; the definitions are this build's, and tests/test_gauss_loss_cpu.py ties the
restatement to the textbook matrix forms.

Bounds.  Loss items 1e-4 relative; every gradient rtol 5e-3 / atol 5e-7 (those of the smooth-L1-IoU extra mode).  The absolute part is
loose at the size of a box-term gradient (box / n per match), so the box channels are held separately: per scale and per channel
(x, y, w, h, theta) the largest difference over the matched cells is at most 1e-3 of the channel's largest float64 gradient.  float32
autograd of the same formulas on these exact inputs differs from float64 by at most 5.9e-6 of that maximum; the older dual-number kernels
are held to 2e-3 per element against their fixtures."""
import numpy as np
import pytest
import torch

from oracle import ref_ops
from tests import gauss_loss_ref as G
from ryolov4_amd.synth import CFG, HYP, synth_targets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CLASSES = {"kld": "ComputeKLDLoss", "gwd": "ComputeGWDLoss", "probiou": "ComputeProbIoULoss"}
# (nc, B, S, per_image, seed) -> matches per scale (counted on the CPU with oracle.ref_ops.build_targets; asserted below so that a silent
# change of the inputs cannot empty the test).  Cells matched more than once per scale: 0/4/3, 20/52/36, 4/15/0.
CASES = {
    (2, 2, 64, 6, 5): (108, 96, 32),
    (16, 2, 128, 20, 5): (436, 434, 168),
    (1, 1, 160, 12, 7): (116, 114, 20),            # nc = 1: no class term
    (16, 1, 64, 0, 0): (0, 0, 0),                  # no targets
}
BIG = (16, 2, 128, 20, 5)


class _Model:
    def __init__(self, nc):
        self.anchors, self.nc = ref_ops.make_anchors(CFG, "kfiou"), nc


def _crit(kind, nc, hyp=HYP):
    from ryolov4_amd.lib import loss as L
    return getattr(L, CLASSES[kind])(_Model(nc), hyp)


_INPUTS, _REFS = {}, {}


def _inputs(case):
    if case not in _INPUTS:
        nc, B, S, per, seed = case
        tg = synth_targets(B, per, nc, False, seed, img_size=S, edge_cases=True) if per else torch.zeros((0, 7))
        g = torch.Generator().manual_seed(9)
        outs = [torch.randn(B, 18, S // s, S // s, nc + 6, generator=g).half().float() for s in (8, 16, 32)]
        _INPUTS[case] = (outs, tg)
    return _INPUTS[case]


def _ref(kind, case):
    """float64 loss items, gradients and matched-cell masks of the restatement; computed once per (loss, case) and never modified."""
    key = (kind, case)
    if key not in _REFS:
        outs, tg = _inputs(case)
        nc = case[0]
        o = [x.double().requires_grad_() for x in outs]
        loss, items = G.compute_gauss_loss(kind, o, tg, _Model(nc).anchors, nc, HYP)
        loss.backward()
        tgt = ref_ops.build_targets([(x.shape[2], x.shape[3]) for x in outs], tg, _Model(nc).anchors, "kfiou")
        masks = []
        for x, m in zip(outs, tgt):
            mk = torch.zeros(x.shape[:4], dtype=torch.bool)
            mk[m["b"], m["a"], m["gj"], m["gi"]] = True
            masks.append(mk)
        _REFS[key] = ({k: float(v.detach()) for k, v in items.items()}, [x.grad.clone() for x in o], masks,
                      tuple(int(m["b"].numel()) for m in tgt))
    return _REFS[key]


def _run(crit, case):
    outs, tg = _inputs(case)
    o = [x.to(DEV).requires_grad_() for x in outs]
    loss, items = crit(o, tg.to(DEV))
    loss.backward()
    return loss, dict(items), [x.grad for x in o]


@pytest.mark.parametrize("case", list(CASES), ids=lambda c: "nc{}_B{}_S{}_per{}".format(*c[:4]))
@pytest.mark.parametrize("kind", list(CLASSES))
def test_kernel_vs_fp64_restatement(kind, case):
    it_ref, g_ref, masks, n_match = _ref(kind, case)
    assert n_match == CASES[case], n_match
    crit = _crit(kind, case[0])
    assert set(crit.loss_items) == {"reg_loss", "conf_loss", "cls_loss", "total_loss"}
    loss, items, grads = _run(crit, case)
    assert tuple(len(r) for r in crit.debug_matches()) == CASES[case]
    for k in crit.KEYS:
        print(kind, case, k, items[k], it_ref[k])
        assert abs(items[k] - it_ref[k]) < 1e-4 * max(1.0, abs(it_ref[k])), (k, items[k], it_ref[k])
    assert abs(float(loss) - it_ref["total_loss"]) < 1e-4 * max(1.0, abs(it_ref["total_loss"]))
    if case[3]:
        assert items["reg_loss"] > 0
    worst = 0.0
    for i, (a, b, mk) in enumerate(zip(grads, g_ref, masks)):
        a = a.cpu()
        assert bool(torch.isfinite(a).all())
        if mk.any():
            for c in range(5):                                   # the box term: x, y, w, h, theta of the matched cells
                col, ref = a[..., c][mk].double(), b[..., c][mk]
                top = float(ref.abs().max())
                err = float((col - ref).abs().max())
                print(kind, case, "scale", i, "channel", c, "max |ref|", top, "max err / max |ref|", err / top)
                worst = max(worst, err / top)
                assert top > 0 and err <= 1e-3 * top, (kind, i, c, err, top)
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=5e-3, atol=5e-7, err_msg=f"{kind} grad{i}")
    print(kind, case, "worst box-channel error / channel maximum:", worst)


@pytest.mark.parametrize("kind", list(CLASSES))
def test_assignment_and_class_term_are_kfiou_s(kind):
    """Only the regression term (and with it the objectness target) is new: the match records equal ComputeKFIoULoss's bit for bit, the class
    term agrees, the regression term does not."""
    from ryolov4_amd.lib import loss as L
    outs, tg = _inputs(BIG)
    o = [x.to(DEV) for x in outs]
    res = {}
    for name, crit in (("kfiou", L.ComputeKFIoULoss(_Model(BIG[0]), HYP)), (kind, _crit(kind, BIG[0]))):
        with torch.no_grad():
            _, items = crit(o, tg.to(DEV))
        res[name] = (dict(items), crit.debug_matches())
    for a, b in zip(res["kfiou"][1], res[kind][1]):
        assert a.shape[0] > 0 and np.array_equal(a, b)
    kf, new = res["kfiou"][0], res[kind][0]
    assert kf["cls_loss"] > 0 and abs(new["cls_loss"] - kf["cls_loss"]) <= 1e-6 * max(1.0, abs(kf["cls_loss"]))
    assert new["reg_loss"] > 0 and abs(new["reg_loss"] - kf["reg_loss"]) > 1e-3 * kf["reg_loss"]


@pytest.mark.parametrize("kind", list(CLASSES))
def test_objectness_target_is_the_similarity_of_the_last_writer(kind):
    """obj = 1, box = cls = 0 leaves the objectness BCE against score = max(1 - L, 0) alone; 108 of the matches of this case share their cell
    with another, so the value depends on which of them wrote last."""
    hyp = dict(HYP, obj=1.0, box=0.0, cls=0.0)
    outs, tg = _inputs(BIG)
    nc = BIG[0]
    o64 = [x.double().requires_grad_() for x in outs]
    l_ref, it_ref = G.compute_gauss_loss(kind, o64, tg, _Model(nc).anchors, nc, hyp)
    l_ref.backward()
    loss, items, grads = _run(_crit(kind, nc, hyp), BIG)
    ref = float(it_ref["conf_loss"].detach())
    assert items["reg_loss"] == 0 and items["cls_loss"] == 0
    assert ref > 0 and abs(items["conf_loss"] - ref) < 1e-4 * max(1.0, abs(ref)), (items["conf_loss"], ref)
    for a, b in zip(grads, o64):                                # only the objectness channel carries a gradient now
        np.testing.assert_allclose(a.cpu().numpy(), b.grad.numpy(), rtol=5e-3, atol=5e-7)
        assert float(a[..., :5].abs().max()) == 0 and float(a[..., 6:].abs().max()) == 0 and float(a[..., 5].abs().max()) > 0


@pytest.mark.parametrize("kind", list(CLASSES))
def test_two_calls_are_bit_identical(kind):
    crit = _crit(kind, BIG[0])
    l1, it1, g1 = _run(crit, BIG)
    l2, it2, g2 = _run(_crit(kind, BIG[0]), BIG)
    assert torch.equal(l1, l2) and it1 == it2
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)


def test_mode_outside_0_to_5_is_refused():
    """A LossParams that a call has just run with, then mode = 6 (it used to run as kfiou): every entry point that reads the mode answers
    'invalid argument' before anything is launched."""
    from ryolov4_amd import hip
    from ryolov4_amd.engine import structs as S
    crit = _crit("probiou", 2)
    outs, tg = _inputs((2, 2, 64, 6, 5))
    o, tg = [x.to(DEV) for x in outs], tg.to(DEV)               # (kept alive: the struct holds raw pointers)
    with torch.no_grad():
        crit(o, tg)
    torch.cuda.synchronize()
    p = crit._last_params
    lib = hip.lib()
    need, own, cnt, rec = S.Z(), (S.P * 3)(), (S.P * 3)(), (S.P * 3)()
    assert p.mode == 5 and lib.ryolo_loss_workspace_bytes(p, need) == 0 and lib.ryolo_loss_owner_grids(p, own) == 0
    for mode in (6, -1, 1 << 20):
        p.mode = mode
        rcs = [lib.ryolo_loss_workspace_bytes(p, need), lib.ryolo_loss(p, hip.stream()), lib.ryolo_loss_owner_grids(p, own),
               lib.ryolo_loss_match_records(p, cnt, rec)]
        assert rcs == [1] * 4, (mode, rcs)                         # 1 = RY_ERR_ARG
    p.mode = 6
    with pytest.raises(RuntimeError, match="invalid argument"):
        hip.call("ryolo_loss", p, hip.stream())


@pytest.mark.parametrize("kind", list(CLASSES))
def test_five_sgd_steps_through_the_engine(kind):
    """Yolo(kfiou) yolov4, batch 4 at 128x128, train.py's N(0, 0.02) init, five SGD steps on one fixed batch: finite gradients and losses, the
    last loss below the first, and the head backward took the loss's compact gradient handoff."""
    import bench
    from ryolov4_amd.lib.loss import make_loss
    from ryolov4_amd.model.yolo import Yolo
    from ryolov4_amd.synth import synth_batch
    torch.manual_seed(42)
    m = Yolo(2, CFG, "kfiou", "yolov4")
    m.apply(bench.weights_init_normal)
    m.to(DEV).train()
    rt = m.runtime()
    crit = make_loss(kind, m, HYP)
    imgs, tg = synth_batch(4, 128, 2, False, seed=42)
    imgs, tg = imgs.to(DEV), tg.to(DEV)
    losses = []
    for _ in range(5):
        loss, items = crit(m(imgs, training=True), tg)
        assert crit._compact is not None
        assert items["reg_loss"] > 0
        loss.backward()
        assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
        rt.sgd_step(0.01)
        losses.append(float(loss.detach()))
    print(kind, losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
