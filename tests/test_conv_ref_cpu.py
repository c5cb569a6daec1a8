"""CPU: tests/conv_ref.py (the float64 interpreter of ConvGemmParams that the direct convolution tests compare the kernels with), the
engine's tap tables (engine/graph.py: _taps_fwd, _taps_dgrad_s1, _classes_dgrad_s2, _taps_dgrad_s2d) and the tables the GPU cases build for
themselves (tests/conv_gemm_cases.py: dgrad_s2_classes, s2d_taps) against torch itself in float64:
forward convolutions against F.conv2d, data gradients against the autograd of F.conv2d.  Integer operands: every comparison is exact."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as CR


def _operands(NB, Cin, Cout, H, W, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-8, 9, (NB, H, W, Cin), generator=g).double()
    w = torch.randint(-3, 4, (Cout, Cin, k, k), generator=g).double()
    return x, w, g


def _engine():
    from ryolov4_amd.engine import graph
    return graph


@pytest.mark.parametrize("k,s,pad", [(1, 1, 0), (3, 1, 1), (3, 2, 1), (1, 2, 0)])
@pytest.mark.parametrize("H,W", [(7, 9), (8, 6), (13, 13), (1, 1), (2, 3)])
def test_forward_taps_against_conv2d(k, s, pad, H, W):
    x, w, _ = _operands(2, 5, 7, H, W, k, 1)
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    ref = F.conv2d(x.permute(0, 3, 1, 2), w, stride=s, padding=pad).permute(0, 2, 3, 1)
    for taps in (CR.taps_forward(k, pad), _engine()._taps_fwd(k, pad)):
        r = CR.conv_gemm_ref(x, CR.pack_forward(w), OH=OH, OW=OW, sh=s, sw=s, classes=[(taps, 0, 0)], epi=CR.EPI_F32_BIAS)
        assert torch.equal(r["out"].double(), ref)
        assert bool((r["writes"] == 1).all())
    assert sorted(CR.taps_forward(k, pad)) == sorted(_engine()._taps_fwd(k, pad))


def _dgrad_autograd(NB, Cin, Cout, H, W, k, s, pad, dy, w):
    x = torch.zeros(NB, Cin, H, W, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, stride=s, padding=pad)
    y.backward(dy.permute(0, 3, 1, 2))
    return x.grad.permute(0, 2, 3, 1)


@pytest.mark.parametrize("k,pad", [(1, 0), (3, 1)])
@pytest.mark.parametrize("H,W", [(7, 9), (8, 6), (1, 1), (2, 3)])
def test_stride1_data_gradient_taps_against_autograd(k, pad, H, W):
    NB, Cin, Cout = 2, 5, 7
    dy, w, _ = _operands(NB, Cout, Cout, H, W, k, 2)
    w = w[:, :Cin].contiguous()
    ref = _dgrad_autograd(NB, Cin, Cout, H, W, k, 1, pad, dy, w)
    taps = _engine()._taps_dgrad_s1(k, pad)
    r = CR.conv_gemm_ref(dy, CR.pack_dgrad(w), OH=H, OW=W, classes=[(taps, 0, 0)], epi=CR.EPI_F32_BIAS)
    assert torch.equal(r["out"].double(), ref)


def _class_recipe(source):
    if source == "engine":
        return _engine()._classes_dgrad_s2(3, 1)
    from tests.conv_gemm_cases import dgrad_s2_classes
    return dgrad_s2_classes()


def _s2d_recipe(source):
    if source == "engine":
        return _engine()._taps_dgrad_s2d()
    from tests.conv_gemm_cases import s2d_taps
    return s2d_taps()


@pytest.mark.parametrize("source", ["engine", "gpu-cases"])
@pytest.mark.parametrize("OH,OW", [(1, 1), (3, 5), (4, 6), (13, 13), (6, 7)])
def test_stride2_four_class_recipe_against_autograd(OH, OW, source):
    """dY grids with odd and even sides (the recipe needs an even input map: H = 2 OH).  Every pixel of the full grid is written once."""
    NB, Cin, Cout, k, pad = 2, 5, 7, 3, 1
    H, W = 2 * OH, 2 * OW
    dy, w, _ = _operands(NB, Cout, Cout, OH, OW, k, 3)
    w = w[:, :Cin].contiguous()
    ref = _dgrad_autograd(NB, Cin, Cout, H, W, k, 2, pad, dy, w)
    classes = _class_recipe(source)
    assert sorted(len(t) for t, _, _ in classes) == [1, 2, 2, 4]
    r = CR.conv_gemm_ref(dy, CR.pack_dgrad(w), OH=OH, OW=OW, classes=classes, oh_mul=2, ow_mul=2, OHf=H, OWf=W, epi=CR.EPI_F32_BIAS)
    assert torch.equal(r["out"].double(), ref)
    assert bool((r["writes"] == 1).all())


@pytest.mark.parametrize("source", ["engine", "gpu-cases"])
@pytest.mark.parametrize("OH,OW", [(1, 1), (3, 5), (4, 6), (7, 7)])
def test_space_to_depth_recipe_against_autograd(OH, OW, source):
    NB, Cin, Cout = 2, 8, 6
    H, W = 2 * OH, 2 * OW
    dy, _, g = _operands(NB, Cout, Cout, OH, OW, 3, 4)
    w = torch.randint(-3, 4, (Cout, Cin, 3, 3), generator=g).double()
    ref = _dgrad_autograd(NB, Cin, Cout, H, W, 3, 2, 1, dy, w)
    r = CR.conv_gemm_ref(dy, CR.pack_s2d(w), OH=OH, OW=OW, classes=[(_s2d_recipe(source), 0, 0)], oh_mul=2, ow_mul=2, OHf=H, OWf=W,
                         epi=CR.EPI_F32_BIAS, s2d_cin=Cin)
    assert torch.equal(r["out"].double(), ref)
    assert bool((r["writes"] == 1).all())


def test_epilogue_roundings():
    """The documented roundings on values chosen by hand: ties go to even, the accumulate and pool steps round a second time."""
    x = torch.tensor([257.0, 258.0, 259.0, 1.0]).view(1, 1, 4, 1).repeat(1, 2, 1, 32)[..., :32] / 32.0      # 32 channels summing to 257, 258, 259, 1
    w = torch.ones(8, 1, 32)
    taps = [(0, 0, 0)]
    r = CR.conv_gemm_ref(x, w, OH=2, OW=4, classes=[(taps, 0, 0)])
    assert r["out"][0, 0, :, 0].tolist() == [256.0, 258.0, 260.0, 1.0]                       # 257 -> 256 (even), 259 -> 260
    old = torch.full((1, 2, 4, 8), 1.0)
    r = CR.conv_gemm_ref(x, w, OH=2, OW=4, classes=[(taps, 0, 0)], epi=CR.EPI_ACCUM, old=old)
    assert r["out"][0, 0, :, 0].tolist() == [256.0, 260.0, 260.0, 2.0]                       # 256 + 1 -> 256, 258 + 1 -> 260, 260 + 1 -> 260
    idx = torch.tensor([[0, 3]], dtype=torch.uint8).view(1, 1, 2, 1).expand(1, 1, 2, 8).contiguous()
    dz = torch.full((1, 1, 2, 8), 3.0)
    r = CR.conv_gemm_ref(x, w, OH=2, OW=4, classes=[(taps, 0, 0)], pool_idx=idx, pool_dz=dz)
    assert r["out"][0, 0, :, 0].tolist() == [260.0, 258.0, 260.0, 1.0]                       # window (0, 0): pixel (0, 0) gets 256 + 3 -> 260 (tie to even)
    assert r["out"][0, 1, :, 0].tolist() == [256.0, 258.0, 260.0, 4.0]                       # window (0, 1), offset 3: pixel (1, 3)
    r = CR.conv_gemm_ref(x, w, OH=2, OW=4, classes=[(taps, 0, 0)], epi=CR.EPI_STATS, tile_rows=4)
    assert r["s1"][0].item() == 2 * (256 + 258 + 260 + 1) and r["s2"][0].item() == 2 * (256 ** 2 + 258 ** 2 + 260 ** 2 + 1)
    assert r["t1"].shape == (2, 8) and r["t1"][1, 0].item() == 256 + 258 + 260 + 1
    b = torch.arange(8.0)
    r = CR.conv_gemm_ref(x, w, OH=2, OW=4, classes=[(taps, 0, 0)], epi=CR.EPI_F32_BIAS, bias=b)
    assert r["out"].dtype == torch.float32 and r["out"][0, 0, 0].tolist() == (257.0 + b).tolist()


def test_lattices_and_their_proof():
    g = torch.Generator().manual_seed(5)
    for kind, K in (("exact", 2304), ("round", 2304), ("round", 32)):
        x, w = CR.lattice(kind, K, g, (1, 8, 8, K // 9 if K > 64 else K), (16, 9 if K > 64 else 1, K // 9 if K > 64 else K))
        taps = CR.taps_forward(3, 1) if K > 64 else [(0, 0, 0)]
        r = CR.conv_gemm_ref(x, w, OH=8, OW=8, classes=[(taps, 0, 0)], epi=CR.EPI_STATS)
        CR.prove_exact(r, stats_exact=kind == "exact")
        inexact = (r["out"].double() != r["y"][0]).double().mean().item()
        assert (inexact == 0.0) if kind == "exact" else (inexact > 0.1)
    x, w = CR.lattice("round", 2304, g, (1, 4, 4, 2304), (8, 9, 2304))                       # K = 20736: past the proof's bound
    r = CR.conv_gemm_ref(x, w, OH=4, OW=4, classes=[(CR.taps_forward(3, 1), 0, 0)])
    with pytest.raises(AssertionError, match="test bug"):
        CR.prove_exact(r)
    x, w = CR.lattice("exact", 288, g, (64, 40, 40, 32), (8, 9, 32), M=64 * 40 * 40)         # thinned weights keep 102 400 rows exact
    r = CR.conv_gemm_ref(x, w, OH=40, OW=40, classes=[(CR.taps_forward(3, 1), 0, 0)], epi=CR.EPI_STATS)
    CR.prove_exact(r, stats_exact=True)
