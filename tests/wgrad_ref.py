"""float64 reference for the weight-gradient C-ABI tests: dW[co, ci, tap] = sum_p dY[p, co] * X[in(p, tap), ci] as one float64 matrix product per
tap (rocBLAS dgemm on the device).  The tests used torch's fp32 conv2d backward (MIOpen) until r05: its solver — and with it its rounding — is chosen by
a benchmark at first use on a fresh box, and one cold-box run of the suite put a layer 2e-3 away from it once; a float64 product has no such freedom.

Also the integer lattices of the bit-exact weight-gradient tests (tests/wgrad_cases.py) and the proof, from the reference alone, that every fp32 sum a
kernel can form on them is exact.  The rule is the forward tests' (tests/conv_ref.py): products of small integers are exact and a sum of exact terms is
exact in ANY order — split into K ranges, slabs, reduce lanes, and finally added to the gradient the kernels accumulate into — while the sum of the
terms' magnitudes stays below conv_ref.ABS_LIMIT.  So dW must equal dW0 + the float64 gradient, bit for bit, whatever the split."""
import torch

from tests import conv_ref as CR

MAG_TARGET = 2.0 ** 15       # the lattices keep max(mag) below this: with |dW0| <= 64 the whole accumulation stays under conv_ref.ABS_LIMIT = 2^16
DW0_MAX = 64


def wgrad_fp64(x, dy, B, H, W, Cin, Cout, kh, kw, stride, ph, pw):
    """x [B*H*W, >= Cin] bf16, dy [B*OH*OW, >= Cout] bf16 (NHWC rows) -> [Cout, Cin, kh*kw] float64."""
    OH, OW = (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1
    xd = x[:, :Cin].double().view(B, H, W, Cin)
    xp = torch.zeros(B, H + 2 * ph + stride, W + 2 * pw + stride, Cin, dtype=torch.float64, device=x.device)
    xp[:, ph:ph + H, pw:pw + W] = xd
    g = dy[:, :Cout].double().view(B * OH * OW, Cout)
    out = torch.empty(Cout, Cin, kh * kw, dtype=torch.float64, device=x.device)
    for r in range(kh):
        for s in range(kw):
            xs = xp[:, r:r + stride * OH:stride, s:s + stride * OW:stride][:, :OH, :OW].reshape(B * OH * OW, Cin)
            out[:, :, r * kw + s] = g.t() @ xs
    return out


def out_size(H, W, kh, kw, stride):
    ph, pw = (kh - 1) // 2, (kw - 1) // 2
    return (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1


def wgrad_fp64_mag(x, dy, B, H, W, Cin, Cout, kh, kw, stride, ph, pw):
    """(dW, mag), both [Cout, Cin, kh*kw] float64: the gradient and, with the same gathers (conv_ref._gather: pixel (oh * stride + r - ph,
    ow * stride + s - pw), zero outside the image), mag[co, ci, tap] = sum_p |dY[p, co]| * |X[in(p, tap), ci]| — the bound of the exactness proof."""
    OH, OW = (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1
    xd = x[:, :Cin].double().view(B, H, W, Cin)
    g = dy[:, :Cout].double().view(B * OH * OW, Cout)
    gt, gat = g.t().contiguous(), g.abs().t().contiguous()
    out = torch.empty(Cout, Cin, kh * kw, dtype=torch.float64, device=x.device)
    mag = torch.empty_like(out)
    for r in range(kh):
        for s in range(kw):
            xs = CR._gather(xd, OH, OW, stride, stride, r - ph, s - pw).reshape(B * OH * OW, Cin)
            out[:, :, r * kw + s] = gt @ xs
            mag[:, :, r * kw + s] = gat @ xs.abs()
    return out, mag


def prove_exact_wgrad(mag, dw0):
    """Raises unless the reference itself shows that every fp32 sum is exact: the magnitudes of all terms of an element plus the gradient it
    is added to stay below conv_ref.ABS_LIMIT lattice units.  A failure is a bug of the test, never of the kernel."""
    m = float(mag.max()) + float(dw0.abs().max())
    if not m < CR.ABS_LIMIT:
        raise AssertionError(f"test bug: max(mag) + max|dW0| = {m} lattice units, not below 2^16: the fp32 sums are not provably exact")


def wgrad_lattice(gen, M_in, M_out, Cin, Cout, CoutPad, ldX, ldY, ntaps, keep=None):
    """Lattice operands on the CPU: x [M_in, ldX] bf16 with integers in [-2, 2] in every column (columns >= Cin are a neighbouring concat slice),
    dy [M_out, ldY] bf16 with integers in {-1, 0, 1} in columns [0, Cout) and >= CoutPad and zeros in [Cout, CoutPad) (the ABI requires them),
    dw0 [Cout, Cin, ntaps] fp32 with integers in [-64, 64].  dy[:, :Cout] is thinned (more zeros) only as far as MAG_TARGET needs: an element
    sums M_out terms of mean magnitude E|dy| * E|x| = (2/3) * (6/5), and the largest of ~10^5 elements lies a few standard deviations
    (sqrt(M * 4/3) each) above the mean, hence the margin.  No blind pixels: every row of dy[:, :Cout] and of x[:, :Cin] keeps a non-zero."""
    x = torch.randint(-2, 3, (M_in, ldX), generator=gen).float()
    dy = torch.randint(-1, 2, (M_out, ldY), generator=gen).float()
    if keep is None:
        mean = M_out * (2.0 / 3.0) * (6.0 / 5.0)
        keep = min(1.0, (MAG_TARGET - 6.0 * (M_out * 4.0 / 3.0) ** 0.5) / mean)
    if keep < 1.0:
        dy[:, :Cout] *= (torch.rand(M_out, Cout, generator=gen) < keep).float()
    dy[:, Cout:CoutPad] = 0.0
    if ldY > CoutPad:
        z = dy[:, CoutPad:]
        z[z == 0] = 1.0
    if ldX > Cin:
        z = x[:, Cin:]
        z[z == 0] = 2.0
    for t, C in ((dy, Cout), (x, Cin)):
        blind = (t[:, :C] != 0).sum(1) == 0
        n = int(blind.sum())
        if n:
            col = torch.randint(0, C, (n,), generator=gen)
            t[blind.nonzero().view(-1), col] = (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float()
    dw0 = torch.randint(-DW0_MAX, DW0_MAX + 1, (Cout, Cin, ntaps), generator=gen).float()
    return x.to(torch.bfloat16), dy.to(torch.bfloat16), dw0


def assert_no_blind_pixels(x, dy, Cin, Cout):
    """Condition of the lattice tests: every pixel contributes to some element, so a dropped pixel changes an integer."""
    assert bool((dy[:, :Cout] != 0).any(1).all()), "test bug: a pixel row of dY is all zero"
    assert bool((x[:, :Cin] != 0).any(1).all()), "test bug: a pixel row of X is all zero"
