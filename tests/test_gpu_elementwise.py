"""BatchNorm finalize, BatchNorm + activation forward / backward and the nearest 2x upsample of csrc/elementwise.hip through the C ABI,
against the float64 references of tests/ew_ref.py.

Two kinds of input in every family:
  lattice  values on a coarse dyadic grid (multiples of 2^-2, |.| <= 2; ACT_LINEAR, scale 1, shift 0 where sums must be exact) so that
           every fp32 sum the kernels can form is exact in any order: the device results must be BIT-IDENTICAL to the float64 reference
           rounded once — a lost, doubled or misaddressed row or channel shows at any size;
  random   normal data with per-channel offsets and scales (one case with |mean| / std = 16), u over about +-30 (past Mish's 20 cut-off
           and SiLU's saturation), all four activations: bf16 outputs within one bf16 ulp of the reference plus the fp32 evaluation
           bound of the kernel's own formula, element by element (ew_ref.py states each bound), and at least 99 % of them bit-identical
           to the reference rounded once (a rounding-mode slip shows there); fp32 reductions within 1e-5 of their absolute sums.
Every operand is a slice (own ld, c0, one sentinel row above and below) of a wider buffer; the sentinels must survive.

Tests named *large* run at real-layer sizes in this process only; test_forced_paths reruns everything else in ONE child process with
the grids capped (grid-stride loops) and the fold thresholds lowered (tests/test_gpu_pool.py runs there too)."""
import os
import subprocess
import sys

import pytest
import torch

from tests import ew_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -77.0                # bf16- and fp32-exact sentinel
LATTICE_UNITS = 2 ** 24     # an fp32 partial of lattice products (multiples of 2^-4) stays exact below 2^24 units


def _lib():
    from ryolov4_amd import hip
    from ryolov4_amd.engine import structs as S
    hip.lib()
    S.check_layouts()
    return hip, S


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


class Slab:
    """Rows [1, M] x columns [c0, c0 + C) of an [M + 2, ld] buffer filled with SENT: `v` is the operand, `ptr` what the kernel gets."""

    def __init__(self, M, C, ld, c0, dtype=torch.bfloat16, fill=None):
        assert ld % 8 == 0 and c0 % 8 == 0 and c0 + C <= ld
        self.buf = torch.full((M + 2, ld), SENT, dtype=dtype, device="cuda")
        self.v = self.buf[1:M + 1, c0:c0 + C]
        if fill is not None:
            self.v.copy_(fill)
        self.ptr = self.buf.data_ptr() + (ld + c0) * self.buf.element_size()     # (an empty view's data_ptr() may be null)
        self.c0, self.C = c0, C

    def intact(self):
        b = self.buf.clone()
        b[1:b.shape[0] - 1, self.c0:self.c0 + self.C] = SENT
        return bool((b == SENT).all())


def _lattice(shape, g):
    return (torch.randint(-8, 9, shape, generator=g, device="cuda").float() * 0.25).to(torch.bfloat16)


def _normal(M, C, g, gain, off_scale=1.0):
    """y = offset_c + std_c * t, t ~ N(0, 1) clipped to +-4, |offset| / std up to off_scale, and [4][C] fp32 BatchNorm coefficients for
    that distribution (mean = offset, invstd = 1 / std, gamma in [0.5, gain], beta in [-3, 3]): u = gamma * t + beta.  (The distribution's
    statistics rather than the batch's: at M = 1 the batch statistics would make every u a cancellation.)"""
    std = torch.rand(C, generator=g, device="cuda") * 1.5 + 0.25
    off = (torch.rand(C, generator=g, device="cuda") * 2 - 1) * off_scale * std
    t = torch.randn(M, C, generator=g, device="cuda").clamp(-4, 4)
    gamma = torch.rand(C, generator=g, device="cuda") * (gain - 0.5) + 0.5
    beta = torch.rand(C, generator=g, device="cuda") * 6 - 3
    invstd = 1.0 / std
    sc = gamma * invstd
    return (off + std * t).to(torch.bfloat16), torch.stack([off, invstd, sc, beta - off * sc]).contiguous()


def _lattice_coeffs(C, g):
    """mean a multiple of 2^-4 in [-1, 1], invstd in {0.5, 1, 2}, scale 1, shift 0: gx = invstd * (S1 - mean * S0) is exact in double."""
    mean = torch.randint(-16, 17, (C,), generator=g, device="cuda").float() / 16
    invstd = 2.0 ** torch.randint(-1, 2, (C,), generator=g, device="cuda").float()
    return torch.stack([mean, invstd, torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")]).contiguous()


class Tally:
    """Bit-identical elements over all cases of a test (a case of 8 elements says little about a 99 % rate on its own)."""

    def __init__(self):
        self.same, self.n = 0, 0

    def check(self, what, min_exact=0.99):
        assert self.n == 0 or self.same >= min_exact * self.n, f"{what}: only {self.same} of {self.n} elements are bit-identical to the reference"


def _check_bf16(got, ref, bound, what, tally, exempt=None):
    """|got - ref| <= 1 bf16 ulp(ref) + bound per element; the elements equal to ref rounded once are counted in tally."""
    if got.numel() == 0:
        return
    gd, rd = got.double(), ref.double()
    ok = (gd - rd).abs() <= R.bf16_ulp(rd) + bound
    if exempt is not None:
        ok |= exempt
    assert bool(ok.all()), (f"{what}: {int((~ok).sum())} of {ok.numel()} elements out of bound; worst "
                            f"{float(((gd - rd).abs() - R.bf16_ulp(rd) - bound).max()):.3g} past it")
    tally.same += int((got == R.round_bf16(ref)).sum())
    tally.n += got.numel()


def _check_kinks(exempt, what):
    if exempt is not None and exempt.numel():
        frac = float(exempt.double().mean())
        assert frac < 1e-4, f"{what}: {frac:.2e} of the elements sit on LeakyReLU's kink"


# ------------------------------------------------------------------------------------------------ BatchNorm forward finalize
def _finalize_case(rows, C, ld, c0, count, running, momentum, seed):
    hip, _ = _lib()
    g = _gen(seed)
    tail = 64
    # partial rows [rows][2][ld]: integer sums s_r in [-8, 8] and sums of squares q_r >= s_r^2; count >= rows, a power of two
    s = torch.randint(-8, 9, (rows, ld), generator=g, device="cuda").float()
    q = s * s + torch.randint(0, 17, (rows, ld), generator=g, device="cuda").float()
    part = torch.full((rows + tail + 4, 2, ld), SENT, device="cuda")
    part[:rows, 0], part[:rows, 1] = s, q
    before = part[:rows].clone()
    gamma = torch.rand(C, generator=g, device="cuda") * 2 - 0.5
    beta = torch.rand(C, generator=g, device="cuda") * 2 - 1
    rm = torch.randn(C, generator=g, device="cuda") if running else None
    rv = torch.rand(C, generator=g, device="cuda") + 0.5 if running else None
    rm0, rv0 = (rm.clone(), rv.clone()) if running else (None, None)
    co = torch.full((4 * C + 8,), SENT, device="cuda")
    hip.call("ryolo_bn_finalize_slice", part.data_ptr(), rows, ld, c0, C, float(count), 1e-5, momentum, gamma.data_ptr(), beta.data_ptr(),
             rm.data_ptr() if running else None, rv.data_ptr() if running else None, co.data_ptr(), hip.stream())
    torch.cuda.synchronize()
    tag = f"rows={rows} C={C} ld={ld} c0={c0} count={count}"
    assert torch.equal(part[:rows], before), f"{tag}: partial rows modified"
    assert bool((part[rows + tail:] == SENT).all()), f"{tag}: wrote past the {tail}-row fold scratch"
    assert bool((co[4 * C:] == SENT).all()), f"{tag}: wrote past coeffs[4][C]"
    mean, invstd, sc, sh, run = R.bn_finalize(part[:rows], c0, C, count, 1e-5, momentum, gamma, beta, rm0, rv0)
    got = co[:4 * C].view(4, C)
    for i, (name, ref) in enumerate((("mean", mean), ("invstd", invstd), ("scale", sc), ("shift", sh))):
        assert torch.equal(got[i], ref), f"{tag}: {name} not bit-identical ({int((got[i] != ref).sum())} channels differ)"
    if running:
        # fp32 update (1 - m) * r + m * x: two roundings of terms bounded by their absolute values
        for name, dev, ref, old in (("running_mean", rm, run[0], rm0), ("running_var", rv, run[1], rv0)):
            mag = (1 - momentum) * old.double().abs() + momentum * ref.double().abs() + ref.double().abs()
            assert bool(((dev.double() - ref).abs() <= 2.0 ** -22 * mag).all()), f"{tag}: {name}"


@pytest.mark.parametrize("rows", [1, 256, 257, 4096, 4097, 40000])
def test_bn_finalize_slice_lattice(rows):
    """rows <= 256: 32 channels per workgroup; 257 ... 4096: 8 channels x 128 row lanes; more: fold_rows pass into the scratch tail first."""
    count = 4 * (1 << (rows - 1).bit_length())
    _finalize_case(rows, 40, 56, 8, count, False, 0.1, seed=rows)
    _finalize_case(rows, 24, 64, 16, count, True, 0.1, seed=rows + 1)
    _finalize_case(rows, 136, 136, 0, count, True, 0.03, seed=rows + 2)


def test_bn_finalize_count_one():
    """count = 1: the unbiased-variance guard (no division by count - 1 = 0)."""
    _finalize_case(1, 32, 48, 8, 1, True, 0.1, seed=7)


def test_bn_eval_coeffs_slice_writes_only_its_columns():
    hip, _ = _lib()
    g = _gen(11)
    for C, ld, c0 in ((40, 64, 8), (300, 320, 16), (8, 8, 0)):
        gamma = torch.rand(C, generator=g, device="cuda") * 2 - 0.5
        beta = torch.rand(C, generator=g, device="cuda") * 2 - 1
        rm = torch.randn(C, generator=g, device="cuda") * 4
        rv = torch.rand(C, generator=g, device="cuda") * 3 + 1e-3
        co = torch.full((4, ld), SENT, device="cuda")
        hip.call("ryolo_bn_eval_coeffs_slice", gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1e-5, C, co.data_ptr(), ld, c0,
                 hip.stream())
        torch.cuda.synchronize()
        out = co.clone()
        out[:, c0:c0 + C] = SENT
        assert bool((out == SENT).all()), f"C={C} ld={ld} c0={c0}: wrote outside columns [c0, c0 + C)"
        got = co[:, c0:c0 + C].double()
        invstd = 1.0 / torch.sqrt(rv.double() + float(torch.tensor(1e-5, dtype=torch.float32)))
        sc = gamma.double() * invstd
        assert torch.equal(co[0, c0:c0 + C], rm)
        # fp32 formula: sqrt, divide, multiply (and an fma for the shift) — a few roundings of 2^-24
        assert bool(((got[1] - invstd).abs() <= 2.0 ** -22 * invstd).all())
        assert bool(((got[2] - sc).abs() <= 2.0 ** -21 * sc.abs()).all())
        sh = beta.double() - rm.double() * sc
        assert bool(((got[3] - sh).abs() <= 2.0 ** -21 * (beta.double().abs() + (rm.double() * sc).abs())).all())


# ------------------------------------------------------------------------------------------------ BatchNorm + activation forward
def _fwd_case(act, two, res, M, C, seed, tally, off_scale=1.0):
    hip, S = _lib()
    g = _gen(seed)
    gain = 3.75 if two else 7.5          # |u| up to about 30 either way
    y, co1 = _normal(M, C, g, gain, off_scale)
    y1 = Slab(M, C, C + 16, 8, fill=y)
    y2, co2 = None, None
    if two:
        y, co2 = _normal(M, C, g, gain, off_scale)
        y2 = Slab(M, C, C + 8, 0, fill=y)
    r = Slab(M, C, C + 24, 16, fill=torch.randn(M, C, generator=g, device="cuda").to(torch.bfloat16) * 4) if res else None
    z = Slab(M, C, C + 32, 24)
    p = S.BnActParams()
    p.y1, p.ld1, p.co1 = y1.ptr, C + 16, co1.data_ptr()
    if two:
        p.y2, p.ld2, p.co2 = y2.ptr, C + 8, co2.data_ptr()
    if res:
        p.res, p.ldr = r.ptr, C + 24
    p.z, p.ldz, p.M, p.C, p.act = z.ptr, C + 32, M, C, act
    hip.call("ryolo_bn_act_fwd", p, hip.stream())
    torch.cuda.synchronize()
    tag = f"fwd act={act} y2={two} res={res} M={M} C={C}"
    assert z.intact(), f"{tag}: wrote outside the z slice"
    for s in (y1, y2, r):
        assert s is None or s.intact()
    if M == 0:
        return
    ref, bound, u, eu = R.bn_act_fwd(y1.v, co1, act, y2.v if two else None, co2, r.v if res else None)
    kink = R.leaky_kink(u, eu, act)
    _check_kinks(kink, tag)
    _check_bf16(z.v, ref, bound, tag, tally, exempt=kink)


FWD_COMBOS = [(a, y2, res) for a in R.ACTS for y2 in (0, 1) for res in (0, 1)]


@pytest.mark.parametrize("act,two,res", FWD_COMBOS)
def test_bn_act_fwd(act, two, res):
    """Every (act x second branch x residual) instantiation; C = 2056 runs the cb loop twice (second pass one column wide); c8 = 3, 5, 48
    leave threads idle; M = 0 returns without a launch."""
    seed = 100 * act + 10 * two + res
    t = Tally()
    for C in (8, 24, 40, 64, 384, 1024, 2056):
        for M in (1, 7, 257):
            _fwd_case(act, two, res, M, C, seed + C + M, t)
    _fwd_case(act, two, res, 0, 64, seed, t)
    _fwd_case(act, two, res, 2000, 96, seed + 5, t, off_scale=16.0)        # |mean| / std = 16
    t.check(f"fwd act={act} y2={two} res={res}")


@pytest.mark.parametrize("act,two,res", FWD_COMBOS)
def test_bn_act_fwd_large(act, two, res):
    t = Tally()
    _fwd_case(act, two, res, 1_300_000, 64, 7 + act + two + res, t)
    t.check("fwd large")


# ------------------------------------------------------------------------------------------------ BatchNorm + activation backward
def _bwd_case(act, two, dres, accum, frozen, M, C, seed, tally, lattice=False, stats_only=False, off_scale=1.0):
    hip, S = _lib()
    g = _gen(seed)
    tag = f"bwd act={act} y2={two} dres={dres} accum={accum} frozen={frozen} M={M} C={C} lattice={lattice} stats_only={stats_only}"
    K = 3 if two else 2
    co2, y2 = None, None
    if lattice:
        co1, co2 = _lattice_coeffs(C, g), (_lattice_coeffs(C, g) if two else None)
        y1 = Slab(M, C, C + 8, 8, fill=_lattice((M, C), g))
        y2 = Slab(M, C, C + 16, 0, fill=_lattice((M, C), g)) if two else None
        dz = Slab(M, C, C + 24, 8, fill=_lattice((M, C), g))
    else:
        gain = 3.75 if two else 7.5
        y, co1 = _normal(M, C, g, gain, off_scale)
        y1 = Slab(M, C, C + 8, 8, fill=y)
        if two:
            y, co2 = _normal(M, C, g, gain, off_scale)
            y2 = Slab(M, C, C + 16, 0, fill=y)
        dz = Slab(M, C, C + 24, 8, fill=torch.randn(M, C, generator=g, device="cuda").to(torch.bfloat16))
    dy1 = None if stats_only else Slab(M, C, C + 16, 16)
    dy2 = Slab(M, C, C + 8, 0) if two else None
    dres0 = (_lattice((M, C), g) if lattice else torch.randn(M, C, generator=g, device="cuda").to(torch.bfloat16)) if dres else None
    dr = Slab(M, C, C + 40, 32, fill=dres0) if dres else None
    nblk, rpb = S.I(), S.I()
    if M > 0:
        hip.call("ryolo_bn_act_bwd_blocks", M, C, nblk, rpb)
    tail = 64                                                            # fold scratch rows the caller appends (engine/graph.py)
    part = torch.full(((nblk.value + tail + 2) * K * C,), SENT, device="cuda")
    start = [torch.randn(C, generator=g, device="cuda") for _ in range(4)]      # dgamma1, dbeta1, dgamma2, dbeta2 accumulate onto these
    if lattice:
        # the widest fp32 partial a workgroup forms: rows_per_block x max |g * y| = 4, in units of 2^-4
        assert rpb.value * 4 * 16 < LATTICE_UNITS, f"{tag}: lattice sums would not be exact"
    p = S.BnActParams()
    p.y1, p.ld1, p.co1 = y1.ptr, C + 8, co1.data_ptr()
    if two:
        p.y2, p.ld2, p.co2, p.dy2, p.lddy2 = y2.ptr, C + 16, co2.data_ptr(), dy2.ptr, C + 8
    p.M, p.C, p.act = M, C, act
    p.dz, p.lddz = dz.ptr, C + 24
    if dy1 is not None:
        p.dy1, p.lddy1 = dy1.ptr, C + 16
    if dres:
        p.dres, p.lddres, p.dres_accum = dr.ptr, C + 40, accum
    p.partial = part.data_ptr()

    def run():
        dg = [s.clone() for s in start]
        bco = torch.full((3 * C + 8,), SENT, device="cuda")
        if dres:
            dr.v.copy_(dres0)
        hip.call("ryolo_bn_act_bwd", p, dg[0].data_ptr(), dg[1].data_ptr(), dg[2].data_ptr() if two else None, dg[3].data_ptr() if two else None,
                 bco.data_ptr(), frozen, hip.stream())
        torch.cuda.synchronize()
        return [bco] + dg + [s.buf.clone() for s in (dy1, dy2, dr) if s is not None]

    first, second = run(), run()
    for x0, x1 in zip(first, second):          # deterministic, atomic-free reductions: bit-identical across runs
        it = torch.int32 if x0.dtype == torch.float32 else torch.int16
        assert torch.equal(x0.view(it), x1.view(it)), f"{tag}: two runs differ"
    bco, dg = first[0], first[1:5]
    for sl in (y1, y2, dz, dy1, dy2, dr):
        assert sl is None or sl.intact(), f"{tag}: wrote outside a slice"
    assert bool((part[(nblk.value + tail) * K * C:] == SENT).all()), f"{tag}: wrote past the partial rows + fold scratch"
    if M == 0:
        assert bool((bco == SENT).all()) and all(torch.equal(x, s) for x, s in zip(dg, start)), f"{tag}: M = 0 must write nothing"
        return
    assert bool((bco[K * C:] == SENT).all()), f"{tag}: wrote past bco[K][C]"
    if not two:
        assert torch.equal(dg[2], start[2]) and torch.equal(dg[3], start[3])

    ref = R.bn_act_bwd(dz.v, y1.v, co1, act, frozen, y2.v if two else None, co2)
    got_bco = bco[:K * C].view(K, C)
    if frozen:
        assert bool((got_bco == 0).all()), f"{tag}: bco must be zero when frozen"
    branches = [(y1, co1, dy1)] + ([(y2, co2, dy2)] if two else [])
    if lattice:
        # exact sums: dbeta / dgamma = fp32(start + fp32(exact sum)), bco = the kernel's double S * (1/M) rounded once
        for i, gx in enumerate(ref["gx"]):
            assert torch.equal(dg[2 * i + 1], R.f32(start[2 * i + 1].double() + R.f32(ref["S0"]).double())), f"{tag}: dbeta{i + 1}"
            assert torch.equal(dg[2 * i], R.f32(start[2 * i].double() + R.f32(gx).double())), f"{tag}: dgamma{i + 1}"
        assert torch.equal(got_bco, ref["bco"]), f"{tag}: bco"
    else:
        _check_kinks(ref["kink"], tag)
        # fp32 sums within 1e-5 of the absolute sums, plus the kernel's evaluation error of g (ref["eg"]):
        #   dbeta: 1e-5 * sum|g| + sum eg;  dgamma: invstd * (1e-5 * sum |g| (|y| + |mean|) + sum eg (|y| + |mean|))
        ga, eg = ref["g"].abs(), ref["eg"]
        b_beta = 1e-5 * ga.sum(0) + eg.sum(0)
        for i, ((y, co, _), gx) in enumerate(zip(branches, ref["gx"])):
            w = y.v.double().abs() + co[0].double().abs()
            b_gam = co[1].double() * (1e-5 * (ga * w).sum(0) + (eg * w).sum(0))
            for name, j, want, b in (("dbeta", 2 * i + 1, ref["S0"], b_beta), ("dgamma", 2 * i, gx, b_gam)):
                tot = start[j].double() + want
                err = (dg[j].double() - tot).abs() - b - 2.0 ** -23 * (start[j].double().abs() + want.abs())
                assert bool((err <= 0).all()), f"{tag}: {name}{i + 1} {float(err.max()):.3g} past its bound"
            if not frozen:
                want = torch.stack([ref["S0"], gx]) / M
                err = (got_bco[[0, i + 1]].double() - want).abs() - torch.stack([b_beta, b_gam]) / M - 2.0 ** -23 * want.abs()
                assert bool((err <= 0).all()), f"{tag}: bco {float(err.max()):.3g} past its bound"
    if stats_only:
        return
    # apply pass: the float64 formula with the coefficients the kernel produced (checked above), kink elements exempt
    mg = got_bco[0].double()
    for i, (y, co, out) in enumerate(branches):
        want, bound = R.apply_ref(ref["g"], y.v, co, mg, got_bco[i + 1].double())
        bound = bound + co[2].double().abs() * ref["eg"]
        _check_bf16(out.v, want, bound, f"{tag}: dy{i + 1}", tally, exempt=None if lattice else ref["kink"])
    if dres:
        want = dz.v.double() + (dres0.double() if accum else 0.0)
        if lattice:
            assert torch.equal(dr.v, R.round_bf16(want)), f"{tag}: dres"
        else:
            _check_bf16(dr.v, want, 2.0 ** -24 * want.abs(), f"{tag}: dres", tally)


# M for C = 64 (32 row lanes): 1 -> one lane 1 row, the rest none; 40 -> 2 / 1 rows; 70 -> 3 / 2 rows.  C = 2056 (one row lane, 257
# column groups: two cb passes): 38407 rows -> 1280 workgroups of 31 rows (odd), the last one 29.  M = 0: nothing written.
BWD_CASES = [  # C, M, dres, accum, frozen
    (64, 1, 1, 0, 0), (64, 40, 0, 0, 1), (64, 70, 1, 1, 0), (64, 96, 1, 1, 1), (24, 7, 1, 0, 0), (40, 257, 0, 0, 0), (384, 1000, 1, 1, 0),
    (8, 3000, 0, 0, 0), (1024, 50, 1, 0, 1), (2056, 38407, 1, 1, 0), (64, 0, 1, 1, 0),
]


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("two", [0, 1])
def test_bn_act_bwd_random(act, two):
    """All 8 reduce instantiations; the apply pass with and without the residual gradient (all 16 apply instantiations over the two dres
    values), accumulate 0 / 1, frozen statistics; every case twice, bit-identical."""
    t = Tally()
    for j, (C, M, dres, accum, frozen) in enumerate(BWD_CASES):
        _bwd_case(act, two, dres, accum, frozen, M, C, 1000 * act + 100 * two + j, t)
        _bwd_case(act, two, 1 - dres, accum, 1 - frozen, M, C, 1000 * act + 100 * two + j + 50, t)
    _bwd_case(act, two, 1, 1, 0, 3000, 96, 77 + act, t, off_scale=16.0)          # |mean| / std = 16
    if not two:
        _bwd_case(act, 0, 0, 0, 0, 3000, 64, 78 + act, t, stats_only=True)       # dy1 == null: statistics only
    t.check(f"bwd act={act} y2={two}")


@pytest.mark.parametrize("two", [0, 1])
def test_bn_act_bwd_lattice(two):
    """Exact sums: dbeta, dgamma (accumulated onto non-zero starts), bco bit-identical at every lane / block shape."""
    t = Tally()
    for j, (C, M, dres, accum, frozen) in enumerate(BWD_CASES):
        _bwd_case(R.LINEAR, two, dres, accum, frozen, M, C, 5000 + 100 * two + j, t, lattice=True)
        _bwd_case(R.LINEAR, two, 1 - dres, 1 - accum, 1 - frozen, M, C, 5050 + 100 * two + j, t, lattice=True)
    if not two:
        _bwd_case(R.LINEAR, 0, 0, 0, 0, 3000, 40, 5999, t, lattice=True, stats_only=True)
    t.check(f"bwd lattice y2={two}")


def test_bn_act_bwd_lattice_large():
    """A real layer: 64 images x 400^2 at C = 32 (1280 workgroups of 8000 rows: the 8-channel finalize)."""
    t = Tally()
    _bwd_case(R.LINEAR, 0, 1, 1, 0, 64 * 400 * 400, 32, 6001, t, lattice=True)
    t.check("bwd lattice large")


def test_bn_act_bwd_random_large():
    t = Tally()
    _bwd_case(R.MISH, 0, 0, 0, 0, 64 * 400 * 400, 32, 6002, t)
    t.check("bwd random large")


# ------------------------------------------------------------------------------------------------ nearest 2x upsample
def _up_case(NB, H, W, C, accum, lattice, seed, tally):
    hip, S = _lib()
    g = _gen(seed)
    mk = (lambda n: _lattice((n, C), g)) if lattice else (lambda n: torch.randn(n, C, generator=g, device="cuda").to(torch.bfloat16))
    n1, n2 = NB * H * W, NB * 4 * H * W
    tag = f"upsample NB={NB} H={H} W={W} C={C} accum={accum} lattice={lattice}"
    x = Slab(n1, C, C + 8, 8, fill=mk(n1))
    z = Slab(n2, C, C + 24, 16)
    p = S.UpParams()
    p.x, p.ldx, p.z, p.ldz, p.NB, p.H, p.W, p.C, p.accum = x.ptr, C + 8, z.ptr, C + 24, NB, H, W, C, 0
    hip.call("ryolo_upsample2x_fwd", p, hip.stream())
    torch.cuda.synchronize()
    assert z.intact() and x.intact(), f"{tag}: forward wrote outside its slice"
    assert torch.equal(z.v.view(NB, 2 * H, 2 * W, C), R.upsample2x(x.v.view(NB, H, W, C))), f"{tag}: forward"
    # backward: x = dz (2H x 2W), z = dx (H x W)
    dz = Slab(n2, C, C + 16, 0, fill=mk(n2))
    e = mk(n1)
    dx = Slab(n1, C, C + 32, 24, fill=e)
    q = S.UpParams()
    q.x, q.ldx, q.z, q.ldz, q.NB, q.H, q.W, q.C, q.accum = dz.ptr, C + 16, dx.ptr, C + 32, NB, H, W, C, accum
    hip.call("ryolo_upsample2x_bwd", q, hip.stream())
    torch.cuda.synchronize()
    assert dx.intact() and dz.intact(), f"{tag}: backward wrote outside its slice"
    want = R.upsample2x_bwd(dz.v.view(NB, 2 * H, 2 * W, C)).view(n1, C) + (e.double() if accum else 0.0)
    if lattice:
        assert torch.equal(dx.v, R.round_bf16(want)), f"{tag}: backward"
    else:
        # fp32 sum of <= 5 terms: 2^-22 of their absolute sum before the one rounding
        mag = R.upsample2x_bwd(dz.v.view(NB, 2 * H, 2 * W, C).abs()).view(n1, C) + (e.double().abs() if accum else 0.0)
        _check_bf16(dx.v, want, 2.0 ** -22 * mag, f"{tag}: backward", tally)


@pytest.mark.parametrize("accum", [0, 1])
@pytest.mark.parametrize("lattice", [True, False])
def test_upsample2x(accum, lattice):
    t = Tally()
    for j, (NB, H, W, C) in enumerate(((2, 13, 20, 64), (1, 1, 1, 8), (3, 7, 5, 24), (2, 25, 25, 2056), (1, 40, 41, 384))):
        _up_case(NB, H, W, C, accum, lattice, 300 + 10 * j + accum + 2 * lattice, t)
    t.check("upsample backward")


# ------------------------------------------------------------------------------------------------ forced paths
def test_forced_paths():
    """All cases above except the *large* ones, and tests/test_gpu_pool.py, in ONE child process (the knobs are read once per process):
    RYOLO_BN_RED_BLOCKS=8192 + RYOLO_BN_FOLD_DIRECT=256 put the fold pass in front of both finalize kernels at moderate M
    (C = 2056, 38407 rows: 4801 reduce workgroups); RYOLO_EW_GRID=3 / RYOLO_EW_GRID2=2 make every thread of the forward, apply, pool and
    upsample kernels walk many rows through its grid-stride loop."""
    import gc
    gc.collect()
    torch.cuda.empty_cache()                       # the child process cannot reuse this process's cached blocks
    env = dict(os.environ, RYOLO_BN_RED_BLOCKS="8192", RYOLO_BN_FOLD_DIRECT="256", RYOLO_EW_GRID="3", RYOLO_EW_GRID2="2")
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_elementwise.py", "tests/test_gpu_pool.py", "-q", "-m", "gpu", "-x",
                        "-k", "not large and not forced_paths", "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout
