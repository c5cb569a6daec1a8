"""float64 reference of the first layer's three entry points (`ryolo_stem3x3_fwd`, `ryolo_stem3x3_wgrad` with y != null, `ryolo_stem3x3_bwd`),
written from the comments of include/ryolo_params.h with plain torch gathers and matrix products; it shares no code with csrc/stem.hip.
tests/test_stem_ref_cpu.py proves it against torch's float64 conv2d and autograd.  Every function works on the device of its inputs.

Roundings mirrored (each one documented by the header, no other):
  image            fp32 -> bf16, round to nearest even, before anything else (the kernels pack fp32 pixels with pack_bf2)
  epilogue 0 / 1   bf16(y); statistics are sums of the STORED values and of their squares
  epilogue 2       bf16(act(y * scale + shift)) of the accumulator;  epilogue 5: the same on bf16(y)
  fused wgrad      dy = bf16(sc*g + A*y + B), g = dz * act'(sc*y + sh), A = -sc*invstd*mx, B = sc*(invstd*mx*mean - mg)
  fused backward   y recomputed and rounded to bf16 for u, g, S0, S1; Yx = W . XX with the unrounded y; G from bf16(g); the result rounded
                   once to fp32 and added to what the gradient tensors held

Also the lattices of tests/test_gpu_stem_lattice.py and the proofs, from the reference alone, that every sum a kernel can form on them is
exact in any order (the rule of tests/conv_ref.py and tests/wgrad_ref.py).  A failed proof raises "test bug": it is never the kernel's."""
from fractions import Fraction

import torch
import torch.nn.functional as F

from tests import conv_ref as CR
from tests import ew_ref as R

EPI_RAW, EPI_STATS, EPI_AFFINE_ACT, EPI_AFFINE_ACT_R = 0, 1, 2, 5
SUM_LIMIT = 2.0 ** 24         # magnitude sums of G, XX, S0, S1 of the fused backward (lattice units)
DW0_MAX = 64


def rne_image(img):
    """fp32 image -> the bf16 values the kernels multiply, as float64."""
    return img.to(torch.float32).to(torch.bfloat16).double()


def patches(x):
    """x [B, 3, H, W] float64 -> im2col rows [B*H*W, 27], k = (r*3 + s)*3 + c, zero padding."""
    B, C, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    cols = [xp[:, :, r:r + H, s:s + W] for r in range(3) for s in range(3)]            # tap r*3 + s: [B, 3, H, W]
    return torch.stack(cols, 1).permute(0, 3, 4, 1, 2).reshape(B * H * W, 27)


def pack_weights(w, dtype=torch.bfloat16):
    """torch weights [Cout][3][3][3] -> the packed [32][32] image of the ABI (rows >= Cout and columns >= 27 zero)."""
    wf = torch.zeros(32, 32, dtype=torch.float64, device=w.device)
    wf[:w.shape[0], :27] = w.double().permute(0, 2, 3, 1).reshape(w.shape[0], 27)
    return wf.to(dtype)


# ------------------------------------------------------------------------------------------------ forward
def forward(img, wf, Cout, epi, scale=None, shift=None, act=0):
    """Returns a dict: y [M, Cout] float64 accumulator, mag = sum |x*w| per output, sq = sum y^2 per column, out (bf16 for epilogues 0 / 1,
    float64 UNROUNDED act(u) for 2 / 5 with u and ew_ref's fp32 evaluation bound), s1 / s2 / a1 / a2 the statistics of the stored values."""
    P = patches(rne_image(img))
    w = wf[:Cout, :27].double()
    y = P @ w.t()
    res = {"y": y, "mag": P.abs() @ w.abs().t(), "sq": (y * y).sum(0)}
    yb = R.round_bf16(y)
    if epi in (EPI_RAW, EPI_STATS):
        res["out"] = yb
        st = yb.double()
        res["s1"], res["s2"], res["a1"], res["a2"] = st.sum(0), (st * st).sum(0), st.abs().sum(0), (st * st).sum(0)
    elif epi in (EPI_AFFINE_ACT, EPI_AFFINE_ACT_R):
        co = torch.stack([torch.zeros_like(scale), torch.ones_like(scale), scale, shift]).double()
        z, bound, u, _ = R.bn_act_fwd(yb.double() if epi == EPI_AFFINE_ACT_R else y, co, act)
        res["out"], res["bound"], res["u"] = z, bound, u
    else:
        raise ValueError(epi)
    return res


def leaky_bits(u):
    """bf16 LeakyReLU(0.1) of an exactly known fp32 u: the product with fp32(0.1) rounded once to fp32, then once to bf16."""
    u32 = u.to(torch.float32)
    assert torch.equal(u32.double(), u.double()), "test bug: u is not an fp32 value"
    return torch.where(u32 > 0, u32, torch.tensor(0.1, dtype=torch.float32, device=u.device) * u32).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ fused weight gradient (y != null)
def wgrad_fused(img, dz, y, co, bco, act):
    """dz, y [M, 32] (the bf16 operands' values), co [4][32], bco [2][32].  Returns dW [32][27] float64 (k = tap*3 + c) and a dict with
    dy64 (unrounded), dyb (bf16), g, u, the terms of dy and mag = sum_p |dyb| |patch|."""
    mu, is_, sc, sh = co.double()
    mg, mx = bco.double()
    y, dz = y.double(), dz.double()
    u = sc * y + sh
    _, d = R.act64(u, act)
    g = dz * d
    A, Bc = -sc * is_ * mx, sc * (is_ * mx * mu - mg)
    terms = (sc * g, A * y, Bc.expand_as(y))
    dy64 = terms[0] + terms[1] + terms[2]
    dyb = R.round_bf16(dy64)
    P = patches(rne_image(img))
    return dyb.double().t() @ P, {"dy64": dy64, "dyb": dyb, "g": g, "u": u, "d": d, "terms": terms, "A": A, "B": Bc, "P": P,
                                  "mag": dyb.double().abs().t() @ P.abs()}


# ------------------------------------------------------------------------------------------------ fused backward
def _recompute(img, wf, co, dz, act):
    mu, is_, sc, sh = co.double()
    P = patches(rne_image(img))
    w = wf[:, :27].double()
    y = P @ w.t()
    yb = R.round_bf16(y).double()
    u = sc * yb + sh
    _, d = R.act64(u, act)
    return P, w, y, yb, u, d, dz.double() * d


def backward_by_definition(img, dz, wf, co, act, frozen):
    """The layer's gradients from the definition: y stored as bf16, BatchNorm backward (batch statistics: dy = sc*(g - mean g -
    xhat * mean(g*xhat)); frozen: dy = sc*g), then the convolution's weight gradient dW = sum_p dy_p (x) patch_p.  Float64 (dWk [32][27], dgamma, dbeta)."""
    mu, is_, sc, sh = co.double()
    P, w, y, yb, u, d, g = _recompute(img, wf, co, dz, act)
    M = P.shape[0]
    xhat = (yb - mu) * is_
    S0, gx = g.sum(0), (g * xhat).sum(0)
    dy = sc * g if frozen else sc * (g - S0 / M - xhat * (gx / M))
    return dy.t() @ P, gx, S0


def backward_by_formula(img, dz, wf, co, act, frozen):
    """The header's rearrangement: dW = sc*G + A*(W.XX) + B*X1, S0 / S1 with the bf16-rounded y, Yx = W . XX with the unrounded one.  (The kernel
    packs g to bf16 for G: no difference for the linear activation on a lattice, a term of the bound otherwise.)  Returns (dWk, dgamma, dbeta, parts)."""
    mu, is_, sc, sh = co.double()
    P, w, y, yb, u, d, g = _recompute(img, wf, co, dz, act)
    M = float(P.shape[0])
    S0, S1 = g.sum(0), (g * yb).sum(0)
    G, XX, X1 = g.t() @ P, P.t() @ P, P.sum(0)
    gx = is_ * (S1 - mu * S0)
    mg = torch.zeros_like(S0) if frozen else S0 / M
    mx = torch.zeros_like(S0) if frozen else gx / M
    Yx = w @ XX
    A, Bc = -sc * is_ * mx, sc * (is_ * mx * mu - mg)
    t = (sc[:, None] * G, A[:, None] * Yx, Bc[:, None] * X1[None, :])
    parts = {"P": P, "w": w, "y": y, "yb": yb, "u": u, "d": d, "g": g, "S0": S0, "S1": S1, "G": G, "XX": XX, "X1": X1, "Yx": Yx, "A": A, "B": Bc,
             "gx": gx, "mg": mg, "mx": mx, "terms": t,
             "mag": {"G": g.abs().t() @ P.abs(), "XX": P.abs().t() @ P.abs(), "S0": g.abs().sum(0), "S1": (g * yb).abs().sum(0)}}
    return (t[0] + t[1]) + t[2], gx, S0, parts


def accumulate(old, exact64):
    """What an accumulating output holds afterwards: the exact value rounded once to fp32, then an fp32 += onto the old value."""
    return old + exact64.to(torch.float32)


# ------------------------------------------------------------------------------------------------ lattices
def lattice(kind, B, H, W, gen, Cout=32):
    """(img fp32 [B, 3, H, W], w float64 [Cout][3][3][3]) on the CPU.
      "exact"  image integers in [-2, 2], weights in {-1, 0, 1}, thinned with zeros until the expected column sum of y^2 fits
               conv_ref.SQ_LIMIT with a factor 2 to spare (as conv_ref.lattice does)
      "round"  image in [-16, 16], weights in [-8, 8], the ranges of conv_ref.lattice for K <= 64: a third of the outputs need rounding, ties
               included.  (With [-8, 8] x [-3, 3] the 27-term sums have a standard deviation of 51 and no output of any case reached 256,
               the first value bf16 cannot hold: nothing was rounded.)
      "frac"   the exact lattice plus, on every non-zero pixel, an offset of -2/8 ... 4/8 of its bf16 ulp: fp32 values that are no bf16
               values (as the workload's k/255), exact ties among them (+4/8 everywhere, -2/8 under a power of two); round-to-nearest-even
               gives the lattice value back, truncation or round-half-up does not.
    No image pixel is all zero in its three channels."""
    M = B * H * W
    if kind in ("exact", "frac"):
        img = torch.randint(-2, 3, (B, 3, H, W), generator=gen).double()
        w = torch.randint(-1, 2, (Cout, 3, 3, 3), generator=gen).double()
        keep = min(1.0, (CR.SQ_LIMIT / 2) / (M * 27 * 2.0 * (2.0 / 3.0)))
        if keep < 1.0:
            w = w * (torch.rand(w.shape, generator=gen) < keep).double()
    elif kind == "round":
        img = torch.randint(-16, 17, (B, 3, H, W), generator=gen).double()
        w = torch.randint(-8, 9, (Cout, 3, 3, 3), generator=gen).double()
    else:
        raise ValueError(kind)
    blind = (img != 0).sum(1) == 0                                                     # [B, H, W]
    img[:, 0][blind] = 1.0
    if kind == "frac":
        j = torch.randint(-2, 5, img.shape, generator=gen).double()
        img = img + torch.sign(img) * j / 8.0 * R.bf16_ulp(img)                      # offsets in magnitude (zero pixels stay zero)
    img32 = img.to(torch.float32)
    assert torch.equal(img32.double(), img), "test bug: the lattice image is not an fp32 image"
    return img32, w


def dz_lattice(M, ld, gen, keep=1.0):
    """dz [M, ld] bf16: integers in {-1, 0, 1} in the 32 channels (no pixel row all zero), non-zero lattice values in the columns beyond."""
    dz = torch.randint(-1, 2, (M, ld), generator=gen).float()
    if keep < 1.0:
        dz[:, :32] *= (torch.rand(M, 32, generator=gen) < keep).float()
    z = dz[:, 32:]
    z[z == 0] = 1.0
    blind = ((dz[:, :32] != 0).sum(1) == 0).nonzero().view(-1)
    if len(blind):
        dz[blind, torch.randint(0, 32, (len(blind),), generator=gen)] = 1.0
    return dz.to(torch.bfloat16)


def bn_lattice(gen, C=32):
    """co [4][C] float64 with mean in [-1, 2], invstd and gamma in {1/2, 1, 2}: scale = gamma*invstd a power of two, shift = beta - mean*scale
    with an integer beta in [-2, 2]."""
    mu = torch.randint(-1, 3, (C,), generator=gen).double()
    is_ = 2.0 ** torch.randint(-1, 2, (C,), generator=gen).double()
    gam = 2.0 ** torch.randint(-1, 2, (C,), generator=gen).double()
    beta = torch.randint(-2, 3, (C,), generator=gen).double()
    sc = gam * is_
    return torch.stack([mu, is_, sc, beta - mu * sc])


def dw0_lattice(gen):
    """Start values of the accumulating outputs: integers in [-64, 64] (dW [32][3][3][3], dgamma, dbeta)."""
    r = lambda *s: torch.randint(-DW0_MAX, DW0_MAX + 1, s, generator=gen).float()
    return r(32, 3, 3, 3), r(32), r(32)


# ------------------------------------------------------------------------------------------------ proofs
def _bug(msg):
    raise AssertionError("test bug: " + msg)


def assert_no_blind_pixels(img, dz=None):
    if not bool((rne_image(img) != 0).any(1).all()):
        _bug("an image pixel is zero in all three channels")
    if dz is not None and not bool((dz[:, :32] != 0).any(1).all()):
        _bug("a pixel row of dz is all zero")


def prove_forward(res, stats_exact=False):
    """sum |x*w| < conv_ref.ABS_LIMIT per output; for exact statistics every output a bf16 value and the column sums of y^2 < conv_ref.SQ_LIMIT."""
    m = float(res["mag"].max())
    if not m < CR.ABS_LIMIT:
        _bug(f"sum |x w| = {m}, not below 2^16: the fp32 sums are not provably exact")
    if stats_exact:
        if not torch.equal(R.round_bf16(res["y"]).double(), res["y"]):
            _bug("an output of the exact lattice is not a bf16 value")
        q = float(res["sq"].max())
        if not q < CR.SQ_LIMIT:
            _bug(f"column sum of y^2 = {q}, not below 2^24: partial statistics are not provably exact")


def _is_pow2_or_small_int(t):
    """Every element is a power of two or an integer of at most 64 in magnitude."""
    t = t.double().abs()
    pow2 = torch.exp2(torch.round(torch.log2(t.clamp_min(2.0 ** -60)))) == t
    return bool((pow2 | ((t == t.round()) & (t <= 64))).all())


def _frac(t):
    return [Fraction(float(v)) for v in t.reshape(-1).tolist()]


def prove_backward(parts, co, count, frozen, exact_lattice):
    """The conditions under which the fused backward is exact: magnitude sums of G, XX, S0, S1 below 2^24; every y a bf16 value on the exact
    lattice; with batch statistics a power-of-two count and power-of-two / small-integer coefficients; and, in exact rational arithmetic on
    the 32 x 27 results, A, B, the three terms of dW and their sum in any order exactly representable in float64."""
    for name, m in parts["mag"].items():
        if not float(m.max()) + DW0_MAX < SUM_LIMIT:
            _bug(f"magnitude sum of {name} = {float(m.max())}, not below 2^24")
    if not float((parts["P"].abs() @ parts["w"].abs().t()).max()) < CR.ABS_LIMIT:
        _bug("sum |x w| of the recompute not below 2^16")
    if exact_lattice and not torch.equal(parts["yb"], parts["y"]):
        _bug("a recomputed y of the exact lattice is not a bf16 value")
    if not _is_pow2_or_small_int(co[:3]):                                              # the shift enters through act' alone
        _bug("mean, invstd or scale is neither a power of two nor a small integer")
    if not torch.equal(co.to(torch.float32).double(), co.double()):
        _bug("a BatchNorm coefficient is not an fp32 value")
    if not frozen and (count & (count - 1)) != 0:
        _bug(f"batch statistics over {count} pixels: not a power of two")
    mu, is_, sc, _ = (_frac(v) for v in co.double())
    S0, S1 = _frac(parts["S0"]), _frac(parts["S1"])
    G, Yx, X1 = _frac(parts["G"]), _frac(parts["Yx"]), _frac(parts["X1"])
    A64, B64 = _frac(parts["A"]), _frac(parts["B"])
    t64 = [_frac(t.expand(32, 27)) for t in parts["terms"]]
    for c in range(32):
        gx = is_[c] * (S1[c] - mu[c] * S0[c])
        mg = Fraction(0) if frozen else S0[c] / count
        mx = Fraction(0) if frozen else gx / count
        A, B = -sc[c] * is_[c] * mx, sc[c] * (is_[c] * mx * mu[c] - mg)
        if A != A64[c] or B != B64[c] or gx != Fraction(float(parts["gx"][c])):
            _bug(f"channel {c}: A, B or dgamma is not exact in float64")
        for k in range(27):
            i = c * 27 + k
            ex = (sc[c] * G[i], A * Yx[i], B * X1[k])
            if any(ex[j] != t64[j][i] for j in range(3)):
                _bug(f"(co, k) = ({c}, {k}): a term of dW is not exact in float64")
            a, b, d = (float(v) for v in ex)
            if not (Fraction((a + b) + d) == Fraction((a + d) + b) == Fraction((b + d) + a) == sum(ex)):
                _bug(f"(co, k) = ({c}, {k}): the sum of the three terms is not exact in float64 in every order")


def prove_dy_exact(info, quantum):
    """Fused weight gradient with the linear activation: every term of dy = sc*g + A*y + B is a multiple of `quantum` and the sum of their
    magnitudes stays below 2^24 quanta (so the fp32 expression is exact however it is contracted or associated); values both on and off
    the bf16 grid occur; and the sum over pixels of |bf16(dy)| |patch| stays below conv_ref.ABS_LIMIT quanta."""
    tot = 0
    for t in info["terms"]:
        q = t / quantum
        if not torch.equal(q, q.round()):
            _bug("a term of dy is not a multiple of the quantum")
        tot = tot + q.abs()
    if not float(tot.max()) < 2.0 ** 24:
        _bug("sum of the magnitudes of dy's terms not below 2^24 quanta")
    on = info["dyb"].double() == info["dy64"]
    if not (bool(on.any()) and bool((~on).any()) and bool((on & (info["dy64"] != 0)).any())):
        _bug("dy must have values both on and off the bf16 grid")
    m = float(info["mag"].max()) / quantum
    if not m < CR.ABS_LIMIT:
        _bug(f"sum |dy| |patch| = {m} quanta, not below 2^16")
