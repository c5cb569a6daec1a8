"""float64 reference of `ryolo_conv_gemm`, written from the comments of include/ryolo_params.h: it interprets the fields of ConvGemmParams
(operand A [NB, IH, IW, Cin], packed weights [Nout][wtaps][Cin], iteration grid OH x OW with strides sh / sw, the tap classes with their
(dh, dw, widx) tables and (oh_add, ow_add), the full output grid oh_mul / ow_mul / OHf / OWf, the epilogue and its operands) with plain
torch gathers and matmuls.  It shares no code with the kernels or with engine/graph.py; tests/test_conv_ref_cpu.py proves it, and the
engine's tap tables, against torch's own conv2d and its autograd.

Also the integer lattices of the direct convolution tests and the proof, from the reference alone, that every fp32 sum a kernel can form
on them is exact: products of small integers are exact, and a sum of exact terms is exact in ANY order while the sum of their absolute
values stays inside the accumulator's mantissa — so the kernel output must equal the float64 result rounded once, bit for bit.

Roundings mirrored (each one documented by the kernels, no other):
  raw            bf16(y)
  accumulate     bf16(bf16(y) + old)
  pool gradient  bf16(bf16(y) + dz where selected), then the accumulate step if asked
  statistics     sums of the STORED bf16 values and of their squares
  EPI_F32_BIAS   y + bias in fp32
  EPI_AFFINE_ACT act(y * scale + shift) in float64 (ew_ref.act64); the caller applies the one-ulp + evaluation bound of ew_ref."""
import torch

from tests import ew_ref as R

EPI_RAW, EPI_STATS, EPI_AFFINE_ACT, EPI_F32_BIAS, EPI_ACCUM = 0, 1, 2, 3, 4
ABS_LIMIT = 2.0 ** 16        # sum |x * w| per output: fp32 keeps 24 bits, eight bits of slack for an adder that aligns to its largest addend
SQ_LIMIT = 2.0 ** 24         # sum of y^2 over all rows of a column (lattice units): every partition into partial rows is then exact


# ------------------------------------------------------------------------------------------------ tap tables (written independently of the engine)
def taps_forward(k, pad):
    """y[oh][ow] = sum_{r, c} x[oh * s - pad + r][ow * s - pad + c] * w[r][c]: offset (r - pad, c - pad), weight slot r * k + c."""
    out = []
    for r in range(k):
        for c in range(k):
            out.append((r - pad, c - pad, r * k + c))
    return out


def pack_forward(w):
    """torch weights [Cout][Cin][k][k] -> [Cout][k * k][Cin]."""
    Cout, Cin, k, _ = w.shape
    return w.permute(0, 2, 3, 1).reshape(Cout, k * k, Cin).contiguous()


def pack_dgrad(w):
    """torch weights [Cout][Cin][k][k] -> the data-gradient image [Cin][k * k][Cout] (GEMM input channels = Cout)."""
    Cout, Cin, k, _ = w.shape
    return w.permute(1, 2, 3, 0).reshape(Cin, k * k, Cout).contiguous()


def pack_s2d(w):
    """ryolo_pack_s2d as documented in csrc/conv.hip: [4 * Cin][4][Cout], row (2 ph + pw) * Cin + ci, tap 2 da + db holds
    W[co][ci][ph + 1 - 2 da][pw + 1 - 2 db] (zero outside the 3x3 kernel)."""
    Cout, Cin = w.shape[:2]
    out = torch.zeros(4 * Cin, 4, Cout, dtype=w.dtype, device=w.device)
    for ph in range(2):
        for pw in range(2):
            for da in range(2):
                for db in range(2):
                    r, s = ph + 1 - 2 * da, pw + 1 - 2 * db
                    if 0 <= r < 3 and 0 <= s < 3:
                        out[(2 * ph + pw) * Cin:(2 * ph + pw + 1) * Cin, 2 * da + db] = w[:, :, r, s].t()
    return out


# ------------------------------------------------------------------------------------------------ the GEMM itself
def _gather(A, OH, OW, sh, sw, dh, dw):
    """A [NB, IH, IW, C] -> [NB, OH, OW, C]: pixel (oh * sh + dh, ow * sw + dw), zero outside the image."""
    NB, IH, IW, C = A.shape
    ih = torch.arange(OH, device=A.device) * sh + dh
    iw = torch.arange(OW, device=A.device) * sw + dw
    okh, okw = (ih >= 0) & (ih < IH), (iw >= 0) & (iw < IW)
    g = A[:, ih.clamp(0, IH - 1)][:, :, iw.clamp(0, IW - 1)]
    return g * (okh.view(1, OH, 1, 1) & okw.view(1, 1, OW, 1)).to(A.dtype)


def class_sums(A, W, OH, OW, sh, sw, taps):
    """(y, sum |a * w|) of one tap class on its iteration grid, both float64 [NB, OH, OW, Nout]."""
    A, W = A.double(), W.double()
    y = mag = None
    for dh, dw, wi in taps:
        g = _gather(A, OH, OW, sh, sw, dh, dw)
        t = g @ W[:, wi].t()
        m = g.abs() @ W[:, wi].abs().t()
        y = t if y is None else y + t
        mag = m if mag is None else mag + m
    return y, mag


def conv_gemm_ref(A, W, *, OH, OW, sh=1, sw=1, classes, oh_mul=1, ow_mul=1, OHf=None, OWf=None, epi=EPI_RAW, old=None,
                  scale=None, shift=None, act=0, bias=None, pool_idx=None, pool_dz=None, s2d_cin=0, tile_rows=None):
    """A [NB, IH, IW, Cin], W [Nout, wtaps, Cin] (any float dtype holding the exact operand values), classes = [(taps, oh_add, ow_add)] with
    taps = [(dh, dw, widx)].  `old` [NB, OHf, OWf, C] is the output buffer's content before the launch (C = Nout, or s2d_cin for the
    depth-to-space store); pool_idx [NB, OH/2, OW/2, Nout] uint8 and pool_dz of the same shape select the fused MaxPool2d(2, 2) gradient.
    Returns a dict:
      out      [NB, OHf, OWf, C]: bf16 (raw / statistics / accumulate), float32 (EPI_F32_BIAS), float64 (EPI_AFFINE_ACT, unrounded);
               positions no class writes keep `old`
      writes   int64 [NB, OHf, OWf, C]: how many (class, row, column) stores land on each element
      mag      the largest sum |a * w| of any output (exactness proof)
      y        float64 accumulator values per class, [NB, OH, OW, Nout]
      u, bound EPI_AFFINE_ACT: the activation's argument and the fp32 evaluation bound of ew_ref.bn_act_fwd (out = act64(u), unrounded)
      s1, s2   EPI_STATS: float64 column sums of the stored bf16 values / of their squares, [Nout]; a1, a2 the sums of their magnitudes;
               with tile_rows also t1, t2 [tiles][Nout]: the same over each run of tile_rows consecutive GEMM rows."""
    NB = A.shape[0]
    Nout = W.shape[0]
    OHf = OH if OHf is None else OHf
    OWf = OW if OWf is None else OWf
    C = s2d_cin if s2d_cin else Nout
    dev = A.device
    res = {"y": [], "mag": 0.0}
    odt = torch.float32 if epi == EPI_F32_BIAS else (torch.float64 if epi == EPI_AFFINE_ACT else torch.bfloat16)
    out = torch.zeros(NB, OHf, OWf, C, dtype=odt, device=dev) if old is None else old.to(odt).clone()
    old64 = out.double()
    writes = torch.zeros(NB, OHf, OWf, C, dtype=torch.int64, device=dev)
    for taps, oh_add, ow_add in classes:
        y, mag = class_sums(A, W, OH, OW, sh, sw, taps)
        res["y"].append(y)
        res["mag"] = max(res["mag"], float(mag.max()))
        if epi == EPI_F32_BIAS:
            v = y if bias is None else y + bias.double().view(1, 1, 1, Nout)
            v = v.to(torch.float32)
        elif epi == EPI_AFFINE_ACT:
            co = torch.stack([torch.zeros_like(scale), torch.ones_like(scale), scale, shift]).double()
            v, bound, u, eu = R.bn_act_fwd(y.reshape(-1, Nout), co, act)
            v = v.view(y.shape)
            res["u"], res["bound"] = u.view(y.shape), bound.view(y.shape)
        else:
            v = R.round_bf16(y)
            if pool_idx is not None:
                hh = torch.arange(OH, device=dev).view(1, OH, 1, 1)
                ww = torch.arange(OW, device=dev).view(1, 1, OW, 1)
                want = ((hh % 2) * 2 + (ww % 2)).to(torch.uint8)
                sel = pool_idx.repeat_interleave(2, 1).repeat_interleave(2, 2) == want
                dz = pool_dz.double().repeat_interleave(2, 1).repeat_interleave(2, 2)
                v = R.round_bf16(v.double() + torch.where(sel, dz, torch.zeros_like(dz)))
            if epi == EPI_STATS:
                st = v.double().reshape(-1, Nout)
                res["s1"], res["s2"] = st.sum(0), (st * st).sum(0)
                res["a1"], res["a2"] = st.abs().sum(0), (st * st).sum(0)
                if tile_rows:
                    pad = (-st.shape[0]) % tile_rows
                    sp = torch.cat([st, torch.zeros(pad, Nout, dtype=st.dtype, device=dev)]).view(-1, tile_rows, Nout)
                    res["t1"], res["t2"] = sp.sum(1), (sp * sp).sum(1)
        # scatter to the full grid
        oh = torch.arange(OH, device=dev) * oh_mul + oh_add
        ow = torch.arange(OW, device=dev) * ow_mul + ow_add
        blocks = [(0, 0, slice(0, Nout))] if not s2d_cin else [(q >> 1, q & 1, slice(q * s2d_cin, (q + 1) * s2d_cin)) for q in range(4)]
        for qh, qw, cols in blocks:
            okr, okc = (oh + qh) < OHf, (ow + qw) < OWf      # (depth-to-space onto an odd map: the last row / column has no 2a + 1 partner)
            rr = (oh + qh)[okr].view(-1, 1).expand(int(okr.sum()), int(okc.sum()))
            cc = (ow + qw)[okc].view(1, -1).expand(int(okr.sum()), int(okc.sum()))
            vv = v[..., cols][:, okr][:, :, okc]
            if epi == EPI_ACCUM:
                vv = R.round_bf16(vv.double() + old64[:, rr, cc])
            out[:, rr, cc] = vv.to(odt)
            writes[:, rr, cc] += 1
    res["out"], res["writes"] = out, writes
    return res


# ------------------------------------------------------------------------------------------------ lattices
def lattice(kind, K, gen, xshape, wshape, M=None, x_exp=0):
    """Integer operands (times 2^x_exp on x) that bf16 holds exactly.
      "exact"  x in [-2, 2], w in {-1, 0, 1}: every output is itself a bf16 value (checked by prove_exact); the weights are thinned (more
               zeros) past K = 2304 and, when M rows are given, until the expected column sum of y^2 fits SQ_LIMIT with a factor 2 to spare
      "round"  x in [-8, 8], w in [-3, 3] (K <= 64: x in [-16, 16], w in [-8, 8]): a third of the outputs need rounding, about a fifth
               are exact ties between two bf16 values."""
    if kind == "exact":
        x = torch.randint(-2, 3, xshape, generator=gen).double()
        w = torch.randint(-1, 2, wshape, generator=gen).double()
        keep = min(1.0, 2304.0 / K)                  # |y| <= 256 was checked up to K = 2304: longer reductions keep that many live terms
        if M is not None:
            keep = min(keep, (SQ_LIMIT / 2) / (M * K * 2.0 * (2.0 / 3.0)))
        if keep < 1.0:
            w = w * (torch.rand(wshape, generator=gen) < keep).double()
    elif kind == "round":
        xr, wr = (16, 8) if K <= 64 else (8, 3)
        x = torch.randint(-xr, xr + 1, xshape, generator=gen).double()
        w = torch.randint(-wr, wr + 1, wshape, generator=gen).double()
    else:
        raise ValueError(kind)
    return x * 2.0 ** x_exp, w


def prove_exact(res, x_exp=0, stats_exact=False):
    """Raises unless the reference itself shows that every fp32 sum is exact: sum |x * w| < 2^16 lattice units per output and, for
    exact statistics, every output a bf16 value and the column sums of y^2 below 2^24 lattice units.  A failure is a bug of the test."""
    unit = 2.0 ** x_exp
    if not res["mag"] / unit < ABS_LIMIT:
        raise AssertionError(f"test bug: sum |x w| = {res['mag'] / unit} lattice units, not below 2^16: the fp32 sums are not provably exact")
    if stats_exact:
        y = res["y"][0]
        if not torch.equal(R.round_bf16(y).double(), y):
            raise AssertionError("test bug: an output of the exact lattice is not a bf16 value")
        q = float(((y / unit) ** 2).reshape(-1, y.shape[-1]).sum(0).max())
        if not q < SQ_LIMIT:
            raise AssertionError(f"test bug: column sum of y^2 = {q} lattice units, not below 2^24: partial statistics are not provably exact")
