"""The tapped LDS-DMA weight-gradient kernel (wgrad_taps_dma_kernel, csrc/conv.hip: stride-2 3x3 layers and every other tapped / strided
layer with more than 64 output channels that the halo-ring kernel does not take) through the C ABI against torch's fp32 conv weight gradient
on the same bf16 operands (model/utils.py:6-32 Conv with stride 2; model/utils.py:146-160 MaxConv's strided branch).  Odd maps (the last
output row / column reads padding), Cin = 32 / 64 (two or four taps per 128-column tile), Cout not a multiple of 32, channel strides
wider than the tensors, accumulation into an existing gradient, a 1x3 tap row.  Dispatch is asserted.  Tolerance 2e-5 relative: the operands are the same bf16 values, so what remains is fp32
accumulation against float64 — measured 2e-7 ... 4e-7 on every case (r05; against torch's fp32 MIOpen gradient, whose solver and rounding vary from box
to box, the tests had to allow 2e-3 and still failed once on a cold box).  A norm over a whole gradient cannot see one pixel dropped for one element:
exactness at the boundaries (K-range ends, image seams, padding rows, ragged tiles, stale split-K slabs, dW2) is pinned bit for bit on integer
lattices in tests/test_gpu_wgrad_lattice.py; these cases keep fp32 rounding at workload sizes in check."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _run(B, H, W, Cin, Cout, k=(3, 3), stride=2, ldx_extra=0, ldy_extra=0, seed=0, expect=2):
    from ryolov4_amd import hip
    from ryolov4_amd.engine import structs as S
    hip.lib()
    S.check_layouts()
    dev = "cuda:0"
    g = torch.Generator().manual_seed(seed)
    kh, kw = k
    ph, pw = (kh - 1) // 2, (kw - 1) // 2
    OH, OW = (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1
    ldX, coutp = Cin + ldx_extra, ((Cout + 7) // 8) * 8
    ldY = coutp + ldy_extra
    x = torch.randn(B * H * W, ldX, generator=g).to(torch.bfloat16).to(dev)
    dy = torch.zeros(B * OH * OW, ldY, dtype=torch.bfloat16)
    dy[:, :Cout] = (torch.randn(B * OH * OW, Cout, generator=g) * 0.1).to(torch.bfloat16)
    dy[:, coutp:] = 3.0                                               # neighbouring slice of a concat buffer: must be ignored
    dy = dy.to(dev)
    dw0 = torch.randn(Cout, Cin, kh * kw, generator=g).to(dev)
    dw = dw0.clone()
    zeros = torch.zeros(256, dtype=torch.uint8, device=dev)
    p = S.WgradParams()
    p.dY, p.ldY, p.Cout, p.CoutPad = dy.data_ptr(), ldY, Cout, coutp
    p.X, p.NB, p.IH, p.IW, p.Cin, p.ldX = x.data_ptr(), B, H, W, Cin, ldX
    p.OH, p.OW, p.sh, p.sw, p.ntaps = OH, OW, stride, stride, kh * kw
    for r in range(kh):
        for s in range(kw):
            p.dh[r * kw + s], p.dw[r * kw + s] = r - ph, s - pw
    p.dW, p.zeros = dw.data_ptr(), zeros.data_ptr()
    kern, sk, ws = S.I(), S.I(), S.Z()
    hip.call("ryolo_conv_wgrad_kernel", p, kern)
    assert kern.value == expect, f"dispatch picked kernel {kern.value} for this shape"
    hip.call("ryolo_conv_wgrad_plan", p, sk, ws)
    work = torch.empty(ws.value, dtype=torch.uint8, device=dev)
    p.partial = work.data_ptr()
    hip.call("ryolo_conv_wgrad", p, hip.stream())
    torch.cuda.synchronize()
    from tests.wgrad_ref import wgrad_fp64
    ref = wgrad_fp64(x, dy, B, H, W, Cin, Cout, kh, kw, stride, ph, pw).float()    # float64 products on the same bf16 operands (tests/wgrad_ref.py)
    got = dw - dw0                                                    # the kernel ACCUMULATES into the gradient
    err = float((got - ref).norm() / ref.norm())
    assert err < 2e-5, f"relative error {err:.3e} (max abs {float((got - ref).abs().max()):.3e}, reference norm {float(ref.norm()):.3e})"
    # per-tap check: a wrong tap offset on one tap hides inside a norm over nine
    for t in range(kh * kw):
        assert float((got[:, :, t] - ref[:, :, t]).norm() / ref[:, :, t].norm()) < 4e-5, f"tap {t}"
    assert bool(torch.isfinite(dw).all())


@pytest.mark.parametrize("B,H,W,Cin,Cout", [
    (8, 64, 64, 64, 128),         # two taps per 128-column tile, last tile half empty (18 chunks)
    (8, 50, 50, 128, 128),        # one tap per tile
    (4, 50, 50, 256, 256),        # two output-channel tiles, two column tiles per tap
    (16, 33, 47, 64, 72),         # odd map (last output row / column touch the padding), Cout not a multiple of 32
    (6, 25, 25, 32, 96),          # four taps per tile, output rows shorter than a 32-pixel step
    (2, 26, 26, 512, 512),        # the deepest stride-2 layer's shape
])
def test_taps_dma_wgrad_stride2_3x3(B, H, W, Cin, Cout):
    _run(B, H, W, Cin, Cout)


def test_taps_dma_wgrad_concat_slices():
    _run(8, 64, 64, 64, 128, ldx_extra=96, ldy_extra=64, seed=4)
    _run(4, 40, 40, 128, 200, ldx_extra=32, ldy_extra=16, seed=5)


def test_taps_dma_wgrad_other_tap_sets():
    _run(4, 40, 40, 64, 128, k=(1, 3), stride=1, seed=6)             # a 1x3 row of taps, stride 1 (not a 3x3: the ring kernel does not take it)
    _run(4, 40, 40, 64, 128, k=(3, 3), stride=1, seed=7)             # a 3x3 stride-1 layer too small for the halo-ring kernel (conv3x3.hip: w3_geometry)
    _run(4, 40, 40, 64, 128, k=(1, 1), stride=2, seed=8)             # strided pointwise (one tap, every other pixel)


def test_small_cout_stays_on_the_generic_kernel():
    _run(4, 40, 40, 32, 64, seed=9, expect=0)


# ---- the stride-2 shapes that round 5's parity-plane ring kernel (retired in r06: parity-green, +15-25 % alone, step-neutral at every grid size; git
# history keeps csrc/conv3x3s2_wgrad8.hip) was tested on stay as cases of the shipped tapped LDS-DMA kernel: odd maps, concat strides, long K ranges.
STRIDE2_CASES = [
    (32, 100, 100, 64, 128, 0, 0),     # 50 x 50 output
    (48, 51, 47, 64, 200, 0, 0),       # odd map, ragged second output tile
    (16, 200, 200, 64, 128, 0, 0),     # 100 x 100 output
    (64, 80, 80, 32, 96, 0, 0),        # a single 32-channel chunk, 96 output channels
    (64, 26, 26, 256, 256, 0, 0),      # 13 x 13 output: a K range crosses many images
    (32, 100, 100, 64, 128, 96, 64),   # concat slices: channel strides wider than the tensors
    (48, 51, 47, 64, 200, 32, 16),
]


@pytest.mark.parametrize("k", range(len(STRIDE2_CASES)))
def test_taps_dma_wgrad_stride2_more_shapes(k):
    B, H, W, Cin, Cout, lx, ly = STRIDE2_CASES[k]
    _run(B, H, W, Cin, Cout, ldx_extra=lx, ldy_extra=ly, seed=20 + k)
