"""(shared case runner of tests/test_gpu_conv_gemm_generic.py and of the lattice modes of the other direct convolution tests; not collected on
its own)  One `ryolo_conv_gemm` launch through the C ABI on integer-lattice operands against tests/conv_ref.py: the kernel output must equal
the float64 reference rounded once, BIT FOR BIT (conv_ref.prove_exact shows per case, from the reference alone, that every fp32 sum is exact).

Memory discipline of every case: A, W, the output, pool_dz, pool_idx and the statistics are slices of larger allocations.  The unused channels
of A (ldA > Cin), the guard rows around A and the guard elements around W hold bf16 NaN: a stray read that reaches an accumulator poisons the
output.  Output padding channels (ld > C), guard rows and the rows of a strided grid that no class owns must come back unchanged."""
import math
import os

import pytest
import torch

from tests import conv_ref as CR
from tests import ew_ref as R

DEV = "cuda:0"
GUARD = 3                 # guard rows before and after every row-major operand
SENTINEL = -24576.0       # raw-store prefill of the owned region: a bf16 / fp32 value no lattice output reaches (checked)


def fwd_classes(k, pad):
    return [(CR.taps_forward(k, pad), 0, 0)]


def _rows(n, ld, dtype, fill):
    full = torch.full((GUARD + n + GUARD, ld), fill, dtype=dtype, device=DEV)
    return full, full[GUARD:GUARD + n]


def _noise(shape, gen, dtype, lo=-32, hi=32):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(dtype).to(DEV)


def describe(kern):
    return f"family {kern & 0xff}" + (f" tile {((kern >> 12) & 15) * 64}x{((kern >> 16) & 15) * 32}{' T1' if kern & 0x100 else ''}" if kern & 0xff == 0 else "")


def run_lattice(*, NB, IH, IW, Cin, Nout, wtaps, OH, OW, stride=1, classes, full=None, epi=0, pipe=0x001, kind="round", ldA_extra=8,
                ldC_extra=8, s2d_cin=0, pool=False, bias=False, act=0, expect=0, tile=None, t1=None, seed=0, weights=None, x_exp=None, tally=None,
                partial_grid=False, edge_col=False, what=""):
    """classes = [(taps, oh_add, ow_add)]; full = (oh_mul, ow_mul, OHf, OWf) or None (identity grid); weights = optional function
    (generator, kind, K) -> float64 [Nout][wtaps][Cin] (packings that are not a plain random image); tile = (rows, cols) the plan must
    announce for family 0, t1 = whether it must announce the 1x1 instantiation.  partial_grid: the classes own only part of the full grid
    (every element written at most once, some never: those must come back unchanged); otherwise every element must be owned exactly once.
    edge_col (family 0): the case must contain a tile whose first row is an output pixel of the LAST reachable column of an image row
    (tile_start_columns; proven here from M, OW and the plan's tile rows).  Returns (output buffer, statistics buffer, the plan's kernel word)."""
    from ryolov4_amd import hip
    from ryolov4_amd.engine import structs as S
    hip.lib()
    S.check_layouts()
    g = torch.Generator(device="cpu").manual_seed(seed)
    oh_mul, ow_mul, OHf, OWf = full if full is not None else (1, 1, OH, OW)
    K = max(len(t) for t, _, _ in classes) * Cin
    M = NB * OH * OW
    exact_stats = epi == S.EPI_STATS and kind == "exact"
    if x_exp is None:
        x_exp = 0
        if epi == S.EPI_AFFINE_ACT:                     # activations want |u| of order 1: scale x by the power of two nearest 1 / std(y)
            ex2, ew2 = (2.0, 2.0 / 3.0) if kind == "exact" else ((24.0, 4.0) if K > 64 else (272.0 / 3.0, 24.0))       # E[x^2], E[w^2] of the lattice
            x_exp = -int(round(0.5 * math.log2(K * ex2 * ew2)))
    x, w = CR.lattice(kind, K, g, (NB, IH, IW, Cin), (Nout, wtaps, Cin), M=M if exact_stats else None, x_exp=x_exp)
    if weights is not None:
        w = weights(g, kind, K)
    unit = 2.0 ** x_exp
    C = s2d_cin if s2d_cin else Nout
    ldA, ldC = Cin + ldA_extra, C + ldC_extra
    P = NB * OHf * OWf
    f32out = epi == S.EPI_F32_BIAS
    odt = torch.float32 if f32out else torch.bfloat16

    # ---- operands: slices of larger allocations
    abuf, a = _rows(NB * IH * IW, ldA, torch.bfloat16, float("nan"))
    a[:, :Cin] = x.view(-1, Cin).to(torch.bfloat16).to(DEV)
    wbuf = torch.full((64 + w.numel() + 64,), float("nan"), dtype=torch.bfloat16, device=DEV)
    wbuf[64:64 + w.numel()] = w.reshape(-1).to(torch.bfloat16).to(DEV)
    obuf, o = _rows(P, ldC, odt, 0.0)
    obuf.copy_((_noise(obuf.shape, g, torch.float32).double() * unit).to(odt))
    if epi != S.EPI_ACCUM:
        o[:, :C] = SENTINEL
    before = obuf.clone()
    zeros = torch.zeros(256, dtype=torch.uint8, device=DEV)
    p = S.ConvGemmParams()
    p.A, p.NB, p.IH, p.IW, p.Cin, p.ldA = a.data_ptr(), NB, IH, IW, Cin, ldA
    p.W, p.Nout, p.wtaps = wbuf.data_ptr() + 128, Nout, wtaps
    p.OH, p.OW, p.sh, p.sw = OH, OW, stride, stride
    p.oh_mul, p.ow_mul, p.OHf, p.OWf = oh_mul, ow_mul, OHf, OWf
    p.nclasses = len(classes)
    for i, (taps, oa, wa) in enumerate(classes):
        tc = p.cls[i]
        tc.ntaps, tc.oh_add, tc.ow_add = len(taps), oa, wa
        for t, (dh, dw, wi) in enumerate(taps):
            tc.dh[t], tc.dw[t], tc.widx[t] = dh, dw, wi
    p.epi, p.out, p.ldC = epi, o.data_ptr(), ldC
    p.zeros, p.pipe, p.s2d_cin = zeros.data_ptr(), pipe, s2d_cin
    p.a_bytes, p.w_bytes = abuf.numel() * 2, w.numel() * 2
    kw = {}
    keep = []
    if epi == S.EPI_AFFINE_ACT:
        if act == R.LINEAR:                             # u = y * 2^k + lattice shift: exact in fp32, so the output is bit-identical
            sc = torch.exp2(torch.randint(-1, 2, (Nout,), generator=g).float())
            sf = torch.randint(-8, 9, (Nout,), generator=g).float() * unit
        else:
            sc = torch.rand(Nout, generator=g) + 0.5
            sf = torch.rand(Nout, generator=g) * 2.0 - 1.0
        co = torch.stack([sc, sf]).to(DEV)
        keep.append(co)
        p.scale, p.shift, p.act = co.data_ptr(), co.data_ptr() + 4 * Nout, act
        kw.update(scale=co[0], shift=co[1], act=act)
    if bias:
        b = torch.randn(Nout, generator=g).to(DEV)
        keep.append(b)
        p.bias = b.data_ptr()
        kw.update(bias=b)
    if pool:
        PH, PW = OH // 2, OW // 2
        ldp = Nout + 8
        ibuf, pi = _rows(NB * PH * PW, ldp, torch.uint8, 0xFF)
        pi[:, :Nout] = torch.randint(0, 4, (NB * PH * PW, Nout), generator=g, dtype=torch.uint8).to(DEV)
        zbuf, pz = _rows(NB * PH * PW, ldp, torch.bfloat16, float("nan"))
        pz[:, :Nout] = (_noise((NB * PH * PW, Nout), g, torch.float32, -8, 8).double() * unit).to(torch.bfloat16)
        keep += [ibuf, zbuf]
        p.pool_idx, p.pool_dz, p.pool_ldi, p.pool_ld = pi.data_ptr(), pz.data_ptr(), ldp, ldp
        kw.update(pool_idx=pi[:, :Nout].reshape(NB, PH, PW, Nout), pool_dz=pz[:, :Nout].reshape(NB, PH, PW, Nout))
        pool_before = (ibuf.clone(), zbuf.clone())

    # ---- the plan: which kernel, which tile
    rows, kern = S.I(), S.I()
    hip.call("ryolo_conv_gemm_plan", p, rows, kern)
    kv = kern.value
    assert kv & 0xff == expect, f"{what}: routed to kernel family {kv & 0xff}, expected {expect} ({kv:#x})"
    tile_rows = None
    if expect == 0:
        tile_rows = ((kv >> 12) & 15) * 64
        if tile is not None:
            assert (tile_rows, ((kv >> 16) & 15) * 32) == tuple(tile), f"{what}: plan announces {describe(kv)}, expected tile {tile}"
        if t1 is not None:
            assert bool(kv & 0x100) == bool(t1), f"{what}: plan announces {describe(kv)}, expected T1 = {t1}"
        if edge_col:
            cols, want = tile_start_columns(M, OW, tile_rows)
            assert want in cols and len(cols) > 1, (f"test bug: {what}: no {tile_rows}-row tile of {M} rows starts at column {want} of OW = {OW} "
                                                    f"(tiles start at columns {sorted(cols)})")
    sbuf = torch.full((2 + max(rows.value, 1) + 2, 2, Nout), 7.0, device=DEV)
    stats = sbuf[2:2 + rows.value]
    if epi == S.EPI_STATS:
        p.stats = stats.data_ptr()

    # ---- the reference (float64, on the device) and the proof that the lattice is exact for this case
    xd, wd = a[:, :Cin].double().view(NB, IH, IW, Cin), wbuf[64:64 + w.numel()].double().view(Nout, wtaps, Cin)
    old = o[:, :C].clone().view(NB, OHf, OWf, C)
    ref = CR.conv_gemm_ref(xd, wd, OH=OH, OW=OW, sh=stride, sw=stride, classes=classes, oh_mul=oh_mul, ow_mul=ow_mul, OHf=OHf, OWf=OWf,
                           epi=epi, old=old, s2d_cin=s2d_cin, tile_rows=tile_rows, **kw)
    CR.prove_exact(ref, x_exp, stats_exact=exact_stats)
    if partial_grid:
        assert int(ref["writes"].max()) == 1 and int(ref["writes"].min()) == 0, f"test bug: {what}: not a partially owned grid"
    else:
        assert bool((ref["writes"] == 1).all()), f"test bug: {what}: the classes do not cover every element of the full grid exactly once"
    if epi != S.EPI_ACCUM:
        top = max(float(y.abs().max()) for y in ref["y"])
        assert top + 64 * unit < -SENTINEL, f"test bug: |y| reaches {top}, the sentinel is not out of range"

    # ---- launch (accumulate / statistics: twice from the same state, the bits must repeat)
    runs = []
    for _ in range(2 if epi in (S.EPI_ACCUM, S.EPI_STATS) else 1):
        obuf.copy_(before)
        stats.fill_(float("nan"))
        hip.call("ryolo_conv_gemm", p, hip.stream())
        torch.cuda.synchronize()
        runs.append((obuf.clone(), sbuf.clone()))
    if len(runs) == 2:
        it = torch.int32 if f32out else torch.int16
        assert torch.equal(runs[0][0].view(it), runs[1][0].view(it)), f"{what}: two launches store different output bits"
        assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32)), f"{what}: two launches store different statistics bits"

    # ---- memory discipline
    it = torch.int32 if f32out else torch.int16                     # every comparison below is on the BITS (+0.0 and -0.0 differ)
    ob, bb = obuf.view(it), before.view(it)
    assert torch.equal(ob[:GUARD], bb[:GUARD]) and torch.equal(ob[GUARD + P:], bb[GUARD + P:]), f"{what}: guard rows of the output changed"
    assert torch.equal(ob[GUARD:GUARD + P, C:], bb[GUARD:GUARD + P, C:]), f"{what}: wrote outside its channel slice (ld > C)"
    seven = torch.full((), 7.0, device=DEV).view(torch.int32)
    assert bool((sbuf[:2].view(torch.int32) == seven).all()) and bool((sbuf[2 + rows.value:].view(torch.int32) == seven).all()), \
        f"{what}: wrote outside the announced statistics rows"
    if pool:
        assert torch.equal(ibuf, pool_before[0]) and torch.equal(zbuf.view(torch.int16), pool_before[1].view(torch.int16)), f"{what}: pool operands changed"

    # ---- values
    got = o[:, :C].reshape(NB, OHf, OWf, C)
    exp = ref["out"]
    if epi == S.EPI_AFFINE_ACT:
        gd = got.double()
        lin_exact = act == R.LINEAR
        same = got.view(torch.int16) == R.round_bf16(exp).view(torch.int16)
        if lin_exact:
            assert bool(same.all()), f"{what}: linear epilogue with exact u: {int((~same).sum())} of {same.numel()} elements differ from the reference rounded once"
        ok = (gd - exp).abs() <= R.bf16_ulp(exp) + ref["bound"]
        assert bool(ok.all()), (f"{what}: {int((~ok).sum())} of {ok.numel()} elements past one bf16 ulp + the fp32 evaluation bound; worst "
                                f"{float(((gd - exp).abs() - R.bf16_ulp(exp) - ref['bound']).max()):.3g} past it")
        if tally is not None:
            tally.same += int(same.sum())
            tally.n += same.numel()
        else:
            assert int(same.sum()) >= 0.99 * same.numel(), f"{what}: only {int(same.sum())} of {same.numel()} elements are bit-identical to the reference"
    else:
        bad = got.contiguous().view(it) != exp.contiguous().view(it)
        if bool(bad.any()):
            idx = bad.nonzero()[0].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} output elements differ from the float64 reference rounded once "
                                 f"({describe(kv)}); first at (img, row, col, channel) = {idx}: got {float(got[tuple(idx)])}, expected "
                                 f"{float(exp[tuple(idx)])}; pixels touched: {int(bad.any(-1).sum())}")
    if epi == S.EPI_STATS:
        assert bool(torch.isfinite(stats).all()), f"{what}: a partial-statistics row the plan announced was not written"
        s1, s2 = stats[:, 0].double().sum(0), stats[:, 1].double().sum(0)
        if exact_stats:
            assert torch.equal(s1, ref["s1"]) and torch.equal(s2, ref["s2"]), f"{what}: column sums differ from the exact reference sums"
            if expect == 0:
                assert rows.value == ref["t1"].shape[0]
                assert torch.equal(stats[:, 0].double(), ref["t1"]) and torch.equal(stats[:, 1].double(), ref["t2"]), \
                    f"{what}: a statistics row is not the sum over its own tile of {tile_rows} pixels"
        else:
            eps = 2.0 ** -24
            assert bool(((s1 - ref["s1"]).abs() <= M * eps * ref["a1"]).all()) and bool(((s2 - ref["s2"]).abs() <= M * eps * ref["a2"]).all()), \
                f"{what}: column sums outside the fp32 summation bound"
            if expect == 0:
                sp = exp.double().reshape(-1, Nout)
                padn = (-sp.shape[0]) % tile_rows
                sp = torch.cat([sp, torch.zeros(padn, Nout, dtype=sp.dtype, device=DEV)]).view(-1, tile_rows, Nout)
                assert bool(((stats[:, 0].double() - ref["t1"]).abs() <= tile_rows * eps * sp.abs().sum(1)).all()) and \
                    bool(((stats[:, 1].double() - ref["t2"]).abs() <= tile_rows * eps * (sp * sp).sum(1)).all()), \
                    f"{what}: a statistics row is outside the fp32 summation bound of its own tile"
    return obuf, sbuf, kv


class Tally:
    """Bit-identical elements over the cases of one test (ew_ref's 99 % rule for the activation epilogue)."""

    def __init__(self):
        self.same, self.n = 0, 0

    def check(self, what):
        assert self.n and self.same >= 0.99 * self.n, f"{what}: only {self.same} of {self.n} elements are bit-identical to the reference"


# ------------------------------------------------------------------------------------------------ geometry helpers
def fwd(NB, H, W, Cin, Nout, k=3, s=1, **kw):
    """Forward convolution k x k, stride s, pad (k - 1) / 2."""
    pad = (k - 1) // 2
    OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
    return run_lattice(NB=NB, IH=H, IW=W, Cin=Cin, Nout=Nout, wtaps=k * k, OH=OH, OW=OW, stride=s, classes=fwd_classes(k, pad), **kw)


def tile_start_columns(M, OW, tile_rows):
    """Columns (ow of the tile's first GEMM row) at which the tiles of tile_rows rows start, and the last column such tiles can reach at all:
    tile k starts at row k * tile_rows, i.e. at column k * tile_rows mod OW, always a multiple of g = gcd(tile_rows, OW) — OW - 1 for odd OW,
    OW - g for even OW (where OW - 1 is unreachable by arithmetic: g is even)."""
    cols = {(k * tile_rows) % OW for k in range((M + tile_rows - 1) // tile_rows)}
    return cols, OW - math.gcd(tile_rows, OW)


def dgrad_s2_classes():
    """The four output-parity classes of the 3x3 stride-2 pad-1 data gradient, derived here from the forward relation x row = 2 oh - 1 + r
    (tests/test_conv_ref_cpu.py checks this recipe, s2d_taps below and the engine's own tables against autograd)."""
    out = []
    for ph in (0, 1):
        for pw in (0, 1):
            taps = []
            for r in range(3):
                for c in range(3):
                    if (ph + 1 - r) % 2 == 0 and (pw + 1 - c) % 2 == 0:
                        taps.append(((ph + 1 - r) // 2, (pw + 1 - c) // 2, r * 3 + c))
            out.append((taps, ph, pw))
    return out


def dgrad_s2(NB, OH, OW, Cout, Cin, only=None, **kw):
    """Stride-2 data gradient in four parity classes: dY [NB, OH, OW, Cout] -> dx [NB, 2 OH, 2 OW, Cin].  only = indices of the classes to
    launch (a subset leaves the other parities of the full grid unowned: partial_grid)."""
    classes = dgrad_s2_classes()
    if only is not None:
        classes = [classes[i] for i in only]
    return run_lattice(NB=NB, IH=OH, IW=OW, Cin=Cout, Nout=Cin, wtaps=9, OH=OH, OW=OW, classes=classes, full=(2, 2, 2 * OH, 2 * OW),
                       partial_grid=only is not None, **kw)


def s2d_taps():
    """2 x 2 taps over the dY grid, weight slot 2 da + db of the ryolo_pack_s2d image (include/ryolo_params.h, s2d_cin)."""
    return [(da, db, 2 * da + db) for da in (0, 1) for db in (0, 1)]


def s2d(NB, OH, OW, Cout, cin, H=None, W=None, **kw):
    """The same gradient as ONE stride-1 GEMM with the depth-to-space store (weights: the ryolo_pack_s2d image of a lattice kernel) onto a
    map of H x W = 2 OH x 2 OW pixels (or one less: kernels that take odd maps drop the missing last row / column)."""
    def weights(g, kind, K):
        _, w = CR.lattice(kind, K, g, (1,), (Cout, cin, 3, 3))
        return CR.pack_s2d(w)
    return run_lattice(NB=NB, IH=OH, IW=OW, Cin=Cout, Nout=4 * cin, wtaps=4, OH=OH, OW=OW, classes=[(s2d_taps(), 0, 0)],
                       full=(2, 2, H or 2 * OH, W or 2 * OW), s2d_cin=cin, weights=weights, **kw)


# ------------------------------------------------------------------------------------------------ the knobs read once per process
# (run by tests/test_gpu_conv_gemm_generic.py in child processes; the expectations follow the knobs of the environment)
CHILD = os.environ.get("RYOLO_CONV_GEMM_CHILD") == "1"
_T1_ON = os.environ.get("RYOLO_GEMM_T1", "1") != "0"
_N64_ALL = os.environ.get("RYOLO_GEMM_N64") == "2"
_DEEP = os.environ.get("RYOLO_GEMM_DEEP", "1")
child_only = pytest.mark.skipif(not CHILD, reason="run through tests/test_gpu_conv_gemm_generic.py (the knobs are read once per process)")


@pytest.mark.gpu
@child_only
@pytest.mark.parametrize("epi", [0, 4])
def test_child_class_order(epi):
    """RYOLO_GEMM_CLS_CHUNK: classes on blockIdx.z (0) or chunks of 16 tiles — 118 and 15 tiles per class at Nout = 32 (last chunk of 6; a
    single chunk shorter than the chunk length), 235 at Nout = 128."""
    for NB, OH, OW, Cout, Nout in ((3, 100, 100, 32, 32), (3, 13, 13, 64, 32), (1, 25, 19, 64, 128), (3, 100, 100, 32, 128), (1, 60, 7, 64, 32)):
        for pipe in (0x001, 0x000):
            dgrad_s2(NB, OH, OW, Cout, Nout, epi=epi, pipe=pipe, tile=(256, 32) if Nout == 32 else (128, 128), seed=OW + epi,
                     what=f"child dgrad {NB}x{OH}x{OW} Nout={Nout} epi={epi} pipe={pipe}")
    dgrad_s2(2, 7, 9, 64, 21, epi=3, bias=True, pipe=0x001, ldC_extra=3, tile=(256, 32), seed=3, what="child f32 classes")


@pytest.mark.gpu
@child_only
@pytest.mark.parametrize("epi", [0, 1, 4])
def test_child_pointwise_and_wide_tiles(epi):
    """RYOLO_GEMM_T1=0: 1x1 layers run the tap-table instantiations; RYOLO_GEMM_N64=2: 33 ... 64 columns run 256x64 tiles on every grid
    of the LDS-DMA mainloop unless the layer takes 64-channel stages."""
    n64 = (256, 64) if _N64_ALL else (128, 64)
    for Cin, Nout, tile in ((32, 8, (256, 32)), (96, 40, n64), (64, 64, n64), (320, 64, n64)):
        fwd(3, 11, 7, Cin, Nout, k=1, epi=epi, pipe=0x001, tile=tile, t1=_T1_ON, seed=Cin + Nout, what=f"child 1x1 {Cin}->{Nout} epi={epi}")
    fwd(2, 13, 13, 32, 64, epi=epi, pipe=0x001, tile=n64, t1=False, seed=1, what=f"child 3x3 32->64 epi={epi}")
    fwd(2, 13, 13, 96, 40, s=2, epi=epi, pipe=0x001, tile=n64, t1=False, seed=2, what=f"child 3x3 s2 96->40 epi={epi}")
    fwd(2, 13, 13, 64, 64, epi=epi, pipe=0x001, tile=(128, 64), t1=False, seed=3, what=f"child 3x3 64->64 (64-channel stages) epi={epi}")
    fwd(2, 13, 13, 64, 64, epi=epi, pipe=0x000, tile=(128, 64), t1=False, seed=4, what=f"child 3x3 64->64 register-staged epi={epi}")


@pytest.mark.gpu
@child_only
@pytest.mark.parametrize("epi", [0, 1, 4])
def test_child_forced_ring_depth(epi):
    """RYOLO_GEMM_DEEP=4 / 6 puts that ring on every identity-grid launch of more than 64 columns: nk below the ring depth (1, 2, 3, 5 steps),
    at it, past it; T1 (unless switched off) and 3x3; one and several column tiles; > 512 tiles."""
    assert _DEEP in ("4", "6")
    for Cin in (32, 64, 96, 160, 128, 192, 384):
        fwd(3, 11, 7, Cin, 136, k=1, epi=epi, pipe=0x001, tile=(128, 128), t1=_T1_ON, seed=Cin + epi, what=f"child ring {_DEEP} 1x1 nk={Cin // 32} epi={epi}")
    fwd(2, 13, 13, 32, 72, epi=epi, pipe=0x001, tile=(128, 128), t1=False, seed=5, what=f"child ring {_DEEP} 3x3 nk=9 epi={epi}")
    fwd(2, 13, 13, 64, 200, s=2, epi=epi, pipe=0x001, tile=(128, 128), t1=False, seed=6, what=f"child ring {_DEEP} 3x3 s2 nk=18 epi={epi}")
    fwd(3, 113, 113, 64, 136, k=1, epi=epi, pipe=0x001, tile=(128, 128), t1=_T1_ON, seed=7, what=f"child ring {_DEEP} 600 tiles epi={epi}")
