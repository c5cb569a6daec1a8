"""Stride-1 max pools (SPP / SPPF / SPPCSPC windows 5, 9, 13): the separable row + column kernels against the direct k*k kernels
of the same library on inputs FULL of ties (values quantised to a few levels): outputs and argmax indices bit-identical (the
first-maximum rule in (dy, dx) scanning order is what routes the gradient, as in torch.nn.MaxPool2d), input gradients equal up to
the fp32 summation order before the bf16 rounding."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


def _pool(x, k, dz, separable):
    from ryolov4_amd import hip
    from ryolov4_amd.engine import structs as S
    hip.lib()
    S.check_layouts()
    B, H, W, Cc = x.shape
    M = B * H * W
    z = torch.empty(M, Cc, dtype=torch.bfloat16, device=x.device)
    idx = torch.empty(M, Cc, dtype=torch.uint8, device=x.device)
    dx = torch.zeros(M, Cc, dtype=torch.bfloat16, device=x.device)
    p = S.PoolParams()
    p.x, p.ldx, p.z, p.ldz = x.data_ptr(), Cc, z.data_ptr(), Cc
    p.NB, p.H, p.W, p.C, p.k, p.stride, p.pad, p.OH, p.OW = B, H, W, Cc, k, 1, k // 2, H, W
    p.idx = idx.data_ptr()
    keep = []
    if separable:
        keep = [torch.empty(M, Cc, dtype=torch.bfloat16, device=x.device), torch.empty(M, Cc, dtype=torch.uint8, device=x.device),
                torch.empty(M, Cc, dtype=torch.float32, device=x.device)]
        p.rowmax, p.rowidx, p.growws = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr()
    hip.call("ryolo_maxpool_fwd", p, hip.stream())
    p.dz, p.lddz, p.dx, p.lddx, p.accum = dz.data_ptr(), Cc, dx.data_ptr(), Cc, 0
    hip.call("ryolo_maxpool_bwd", p, hip.stream())
    torch.cuda.synchronize()
    return z, idx, dx


@pytest.mark.parametrize("k", [5, 9, 13])
@pytest.mark.parametrize("shape", [(2, 25, 25, 64), (3, 13, 19, 40), (1, 7, 5, 8)])
def test_separable_pool_equals_direct(k, shape):
    B, H, W, Cc = shape
    g = torch.Generator().manual_seed(k)
    x = (torch.randint(0, 6, (B, H, W, Cc), generator=g).float() * 0.25 - 0.5).to(torch.bfloat16).cuda()      # 6 levels: ties everywhere
    dz = torch.randn(B * H * W, Cc, generator=g).to(torch.bfloat16).cuda()
    z0, i0, d0 = _pool(x, k, dz, False)
    z1, i1, d1 = _pool(x, k, dz, True)
    assert torch.equal(z0, z1)
    assert torch.equal(i0, i1), "argmax (first maximum in scanning order) differs"
    ref = torch.nn.functional.max_pool2d(x.float().permute(0, 3, 1, 2), k, 1, k // 2).permute(0, 2, 3, 1).reshape(-1, Cc)
    assert torch.equal(z1.float(), ref)
    assert torch.allclose(d0.float(), d1.float(), rtol=2 ** -7, atol=1e-2)


# ---- every pool path against the float64 reference of tests/ew_ref.py ---------------------------------------------------------------
# Forward values and first-maximum indices exact; the gradient on lattice values (multiples of 2^-2, |.| <= 2: every fp32 sum exact)
# bit-identical to the exact sum rounded once, with and without accumulate.  All four operands are slices (ld > C) with sentinel columns.
SENT = -77.0


def _slab(n, Cc, ld, c0, fill=None):
    buf = torch.full((n, ld), SENT, dtype=torch.bfloat16, device="cuda")
    if fill is not None:
        buf[:, c0:c0 + Cc] = fill
    return buf, buf[:, c0:c0 + Cc]


def _outside(buf, c0, Cc):
    b = buf.clone()
    b[:, c0:c0 + Cc] = SENT
    return bool((b == SENT).all())


def _pool_ref_case(NB, H, W, Cc, k, stride, pad, separable, accum, seed, chunk=None):
    from ryolov4_amd import hip
    from ryolov4_amd.engine import structs as S
    from tests import ew_ref as R
    hip.lib()
    S.check_layouts()
    g = torch.Generator(device="cuda").manual_seed(seed)
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    M, MO = NB * H * W, NB * OH * OW
    lat = lambda n: (torch.randint(-8, 9, (n, Cc), generator=g, device="cuda").float() * 0.25).to(torch.bfloat16)     # noqa: E731
    xb, x = _slab(M, Cc, Cc + 8, 8, (torch.randint(0, 6, (M, Cc), generator=g, device="cuda").float() * 0.25 - 0.5).to(torch.bfloat16))
    zb, z = _slab(MO, Cc, Cc + 16, 16)
    idx = torch.full((MO, Cc), 255, dtype=torch.uint8, device="cuda")
    p = S.PoolParams()
    p.x, p.ldx, p.z, p.ldz = x.data_ptr(), Cc + 8, z.data_ptr(), Cc + 16
    p.NB, p.H, p.W, p.C, p.k, p.stride, p.pad, p.OH, p.OW = NB, H, W, Cc, k, stride, pad, OH, OW
    p.idx = idx.data_ptr()
    keep = []
    if separable:
        keep = [torch.empty(M, Cc, dtype=torch.bfloat16, device="cuda"), torch.empty(M, Cc, dtype=torch.uint8, device="cuda"),
                torch.empty(M, Cc, dtype=torch.float32, device="cuda")]
        p.rowmax, p.rowidx, p.growws = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr()
    hip.call("ryolo_maxpool_fwd", p, hip.stream())
    torch.cuda.synchronize()
    tag = f"pool NB={NB} H={H} W={W} C={Cc} k={k} s={stride} separable={separable} accum={accum}"
    assert _outside(zb, 16, Cc) and _outside(xb, 8, Cc), f"{tag}: forward wrote outside its slice"
    zr, ir = R.maxpool(x.view(NB, H, W, Cc), k, stride, pad, rows_per_chunk=chunk)
    assert torch.equal(z.float().view(NB, OH, OW, Cc), zr), f"{tag}: pooled values"
    assert torch.equal(idx.view(NB, OH, OW, Cc).long(), ir), f"{tag}: argmax (first maximum in (dy, dx) order)"
    del zr
    dzb, dz = _slab(MO, Cc, Cc + 24, 8, lat(MO))
    e = lat(M)
    dxb, dx = _slab(M, Cc, Cc + 32, 24, e)
    p.dz, p.lddz, p.dx, p.lddx, p.accum = dz.data_ptr(), Cc + 24, dx.data_ptr(), Cc + 32, accum
    hip.call("ryolo_maxpool_bwd", p, hip.stream())
    torch.cuda.synchronize()
    assert _outside(dxb, 24, Cc) and _outside(dzb, 8, Cc), f"{tag}: backward wrote outside its slice"
    want = R.maxpool_bwd(ir, dz.view(NB, OH, OW, Cc), H, W, k, stride, pad).view(M, Cc)
    if accum:
        want += e.double()
    assert torch.equal(dx, R.round_bf16(want)), f"{tag}: gradient ({int((dx != R.round_bf16(want)).sum())} elements differ)"


@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("Cc", [8, 24, 1032])
def test_maxconv_k2s2_vs_fp64(Cc, accum):
    """MaxConv's k2 s2 pad 0, odd H / W (floor mode: the last input row / column belongs to no window and gets no gradient)."""
    for j, (NB, H, W) in enumerate(((2, 9, 11), (1, 3, 5), (3, 16, 7))):
        _pool_ref_case(NB, H, W, Cc, 2, 2, 0, False, accum, seed=10 * j + Cc + accum)


@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("separable", [False, True])
@pytest.mark.parametrize("k", [5, 9, 13])
def test_spp_pool_vs_fp64(k, separable, accum):
    for j, (NB, H, W, Cc) in enumerate(((2, 13, 11, 8), (1, 7, 20, 24), (2, 10, 9, 1032))):
        _pool_ref_case(NB, H, W, Cc, k, 1, k // 2, separable, accum, seed=100 * k + 10 * j + 2 * separable + accum)


@pytest.mark.parametrize("k,stride,separable", [(2, 2, False), (5, 1, True), (5, 1, False)])
def test_pool_large_more_than_2_24_pixels(k, stride, separable):
    """NB * H * W > 2^24 at C = 8: the integer branch of split_pixel (forward over outputs at k5 s1, backward over inputs in both)."""
    _pool_ref_case(1, 4100, 4100, 8, k, stride, k // 2 if stride == 1 else 0, separable, 1, seed=k + separable, chunk=256)
