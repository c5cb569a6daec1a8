"""Harness and case tables of the bit-exact first-layer tests (tests/test_gpu_stem_lattice.py on the GPU, tests/test_stem_ref_cpu.py for the
reference, the proofs and the grid facts).  Reference and proofs: tests/stem_ref.py.

Every operand is a slice of a larger allocation, as tests/wgrad_cases.py does it: the image lies inside an fp32 buffer whose remainder is NaN,
dz / dY / y between NaN guard rows with lattice values in the columns beyond the 32 channels, `out` is pre-filled with a guard value (wider
than Cout: the columns beyond must come back unchanged), the statistics rows the plan names are NaN between guard rows (the engine sums all
of them, so every one must be written), the workspace is the planned byte count, all NaN, between guard bands, and the accumulating outputs
start from integers in [-64, 64] between guards and are run twice from the same start.  Every comparison is on the bits."""
import collections
import functools

import torch

from tests import ew_ref as R
from tests import stem_ref as SR
from tests import wgrad_cases as WC

# ------------------------------------------------------------------------------------------------ shapes (B, H, W)
LDS_SHAPES = [(2, 16, 32), (3, 17, 32), (2, 1, 64), (2, 8, 128), (2, 5, 96)]        # W % 32 == 0: LDS-patch forward, fused backward
LARGE = (1, 331, 800)                                                                # the workload's width: three tiles per wave
GATHER_SHAPES = [(3, 17, 17), (2, 9, 48), (1, 5, 16), (2, 5, 1)]                    # W % 32 != 0: register-gather forward
WGRAD_SHAPES = [(2, 32, 48), (3, 17, 16), (2, 16, 32)]                              # W % 16 == 0: fused weight gradient
POW2_COUNT = [(2, 16, 32), (2, 8, 128)]                                              # batch statistics are exact: count 2^10, 2^11
KINDS = ("exact", "round", "frac")


def sid(shape):
    return "x".join(map(str, shape))


# ------------------------------------------------------------------------------------------------ launch arithmetic of csrc/stem.hip, restated
def cdiv(a, b):
    return -(-a // b)


Grid = collections.namedtuple("Grid", "blocks waves tiles per_wave busy ragged idle")


def lds_grid(M, per_cu):
    """LDS-patch kernels (forward per_cu = 4, fused backward 3): one workgroup per 256 pixels up to 256 * per_cu, four waves each; every wave
    owns ceil(tiles / waves) consecutive 32-pixel tiles.  busy = waves with at least one tile, ragged = tiles of the last busy wave when
    that is fewer than per_wave (else 0), idle = waves without a tile."""
    blocks = max(1, min(cdiv(M, 256), 256 * per_cu))
    waves, tiles = 4 * blocks, M // 32
    per = cdiv(tiles, waves)
    busy = cdiv(tiles, per)
    return Grid(blocks, waves, tiles, per, busy, tiles % per, waves - busy)


def gather_blocks(M):
    """Register-gather forward and the weight gradient: one workgroup per 1024 pixels, at most 2048."""
    return max(1, min(cdiv(M, 1024), 2048))


def seam_inside_a_range(shape, per_cu):
    """Some wave's tile range of the column-major walk holds tiles of two images."""
    B, H, W = shape
    g = lds_grid(B * H * W, per_cu)
    per_image = H * (W // 32)
    return any(u // per_image != (min(u + g.per_wave, g.tiles) - 1) // per_image for u in range(0, g.tiles, g.per_wave))


# ------------------------------------------------------------------------------------------------ operands and references (cached per case)
def _gen(*key):
    return torch.Generator().manual_seed(sum(map(ord, repr(key))))


@functools.lru_cache(maxsize=None)
def fwd_operands(shape, kind, Cout=32):
    """(img fp32 [B, 3, H, W], wf bf16 [32][32]) on the CPU.  Rows >= Cout of wf hold ones: no kernel may read them."""
    B, H, W = shape
    img, w = SR.lattice(kind, B, H, W, _gen("fwd", shape, kind, Cout), Cout)
    wf = SR.pack_weights(w, torch.float64)
    wf[Cout:, :27] = 1.0
    return img, wf.to(torch.bfloat16)


def affine_coefficients(shape, act):
    """scale, shift [32] fp32: power-of-two scale and integer shift, so u = y*scale + shift is exact in fp32.  Linear: scale in {1/4 ... 2};
    the others 2^-6 ... 2^-4, which brings the rounding lattice's |y| (hundreds) to both sides of Mish's cut-off at u = 20."""
    g = _gen("affine", shape, act)
    e = torch.randint(-2, 2, (32,), generator=g) if act == R.LINEAR else torch.randint(-6, -3, (32,), generator=g)
    return torch.exp2(e.float()), torch.randint(-3, 4, (32,), generator=g).float()


@functools.lru_cache(maxsize=16)
def fwd_reference(shape, kind, Cout, epi, act, device):
    img, wf = fwd_operands(shape, kind, Cout)
    sc, sh = affine_coefficients(shape, act)
    res = SR.forward(img.to(device), wf.to(device), Cout, epi, sc[:Cout].to(device), sh[:Cout].to(device), act)
    SR.assert_no_blind_pixels(img)
    SR.prove_forward(res, stats_exact=kind != "round")
    if epi in (2, 5):
        u = res["u"]
        assert torch.equal(u.to(torch.float32).double(), u), "test bug: u is not exact in fp32"
    return res


@functools.lru_cache(maxsize=None)
def wgrad_operands(shape):
    """Fused weight gradient: image on the exact lattice; dz in {-1, 0, 1} (ld 48); y (ld 40) integers in [-2, 2] with one value in two hundred an
    even integer in +-[256, 500]; sc in {1/2, 1}, invstd 1, mean in [-1, 2], integer shift; bco: mg in {-1, 0, 1}, mx = +-1/2.  Then A = -sc*invstd*mx is
    +-1/4 or +-1/2 and B a multiple of 1/4: every term of dy is a multiple of 1/4, small values lie on the bf16 grid, and A*y + B + sc*g
    beyond 64 (bf16 spacing 1/2, beyond 128: 1) falls between grid points, exact ties included."""
    B, H, W = shape
    M = B * H * W
    g = _gen("wgrad", shape)
    img, _ = SR.lattice("exact", B, H, W, g)
    dz = SR.dz_lattice(M, 48, g)
    y = torch.randint(-2, 3, (M, 40), generator=g).float()
    big = torch.rand(M, 40, generator=g) < 0.005
    y = torch.where(big, torch.randint(128, 251, (M, 40), generator=g).float() * 2 * (torch.randint(0, 2, (M, 40), generator=g) * 2 - 1).float(), y)
    sc = torch.exp2(torch.randint(-1, 1, (32,), generator=g).float())
    mu = torch.randint(-1, 3, (32,), generator=g).float()
    co = torch.stack([mu, torch.ones(32), sc, torch.randint(-2, 3, (32,), generator=g).float()])
    bco = torch.stack([torch.randint(-1, 2, (32,), generator=g).float(), (torch.randint(0, 2, (32,), generator=g) * 2 - 1).float() * 0.5])
    return img, dz, y.to(torch.bfloat16), co, bco


@functools.lru_cache(maxsize=None)
def bwd_operands(shape, kind):
    """(img, wf, dz [M][40], co [4][32] fp32, (dW0, dgamma0, dbeta0)) on the CPU."""
    B, H, W = shape
    g = _gen("bwd", shape, kind)
    img, w = SR.lattice(kind, B, H, W, g)
    return img, SR.pack_weights(w), SR.dz_lattice(B * H * W, 40, g), SR.bn_lattice(g).float(), SR.dw0_lattice(g)


def nonlinear_coefficients(shape):
    """Frozen BatchNorm for the Mish / SiLU backward: scale 2^-3 ... 2^-1 and an integer shift, so u = scale*y + shift is exact in fp32 and
    the exact lattice's |y| <= 54 covers |u| <= 30."""
    g = _gen("bwd-act", shape)
    sc = torch.exp2(torch.randint(-3, 0, (32,), generator=g).float())
    return torch.stack([torch.zeros(32), torch.ones(32), sc, torch.randint(-2, 3, (32,), generator=g).float()])


# ------------------------------------------------------------------------------------------------ buffers
DEVICE = "cuda:0"
OUT_GUARD = 24832.0             # a bf16 value no lattice output reaches (|y| <= 27 * 16 * 8 = 3456, |u| <= 2 * 3456 + 3)
IMG_PAD = 4096                  # fp32 NaN on both sides of the image (a multiple of 4: the image stays 16-byte aligned)
GUARD_ROWS = 8


def _lib():
    from ryolov4_amd import hip
    from ryolov4_amd.engine import structs as S
    hip.lib()
    S.check_layouts()
    return hip, S


def image_slice(img):
    n = img.numel()
    buf = torch.full((IMG_PAD + n + IMG_PAD,), float("nan"), dtype=torch.float32, device=DEVICE)
    buf[IMG_PAD:IMG_PAD + n] = img.reshape(-1).to(DEVICE)
    return buf, buf[IMG_PAD:IMG_PAD + n].view(img.shape)


def rows_slice(t, fill=float("nan")):
    """[M, ld] -> (buffer [guard rows | M | guard rows], the payload view)."""
    M, ld = t.shape
    buf = torch.full((GUARD_ROWS + M + GUARD_ROWS, ld), fill, dtype=t.dtype, device=DEVICE)
    buf[GUARD_ROWS:GUARD_ROWS + M] = t.to(DEVICE)
    return buf, buf[GUARD_ROWS:GUARD_ROWS + M]


def guards_intact(buf, fill):
    g = torch.cat([buf[:GUARD_ROWS].reshape(-1), buf[-GUARD_ROWS:].reshape(-1)])
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


def workspace(nbytes):
    assert nbytes % 4 == 0
    ng = WC.WS_GUARD_BYTES // 4
    work = torch.full((ng + nbytes // 4 + ng,), float("nan"), dtype=torch.float32, device=DEVICE)
    return work, ng


def workspace_guards_intact(work, ng):
    return bool(torch.isnan(work[:ng]).all()) and bool(torch.isnan(work[-ng:]).all())


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ------------------------------------------------------------------------------------------------ forward
def launch_forward(shape, img_view, wf, Cout, epi, *, with_out=True, scale=None, shift=None, act=0, ldC=40):
    """One `ryolo_stem3x3_fwd`.  Returns (out [M, Cout] bf16 or None, statistics rows [rows, 2, Cout] or None); asserts the guards."""
    hip, S = _lib()
    B, H, W = shape
    M = B * H * W
    p = S.StemParams()
    p.img, p.NB, p.H, p.W = img_view.data_ptr(), B, H, W
    p.wf, p.Cout, p.epi, p.act, p.ldC = wf.data_ptr(), Cout, epi, act, ldC
    obuf = out = sbuf = None
    if with_out:
        obuf, out = rows_slice(torch.full((M, ldC), OUT_GUARD, dtype=torch.bfloat16), OUT_GUARD)
        p.out = out.data_ptr()
    if epi == 1:
        rows = S.I()
        hip.call("ryolo_stem3x3_plan", B, H, W, Cout, rows, None)
        sbuf, st = rows_slice(torch.full((rows.value, 2 * Cout), float("nan")), WC.GUARD)
        p.stats = st.data_ptr()
    if scale is not None:
        p.scale, p.shift = scale.data_ptr(), shift.data_ptr()
    hip.call("ryolo_stem3x3_fwd", p, hip.stream())
    torch.cuda.synchronize()
    stats = None
    if with_out:
        assert guards_intact(obuf, OUT_GUARD), "forward: wrote outside the rows of out"
        assert bool((out[:, Cout:] == OUT_GUARD).all()), "forward: wrote channels >= Cout of out"
    if epi == 1:
        assert guards_intact(sbuf, WC.GUARD), "forward: wrote outside the planned statistics rows"
        stats = st.view(-1, 2, Cout)
        assert not bool(torch.isnan(stats).any()), f"forward: {int(torch.isnan(stats).any(2).any(1).sum())} of {stats.shape[0]} planned statistics rows not written"
    return (out[:, :Cout] if with_out else None), stats


def _same_bits(what, shape, got, want):
    if not torch.equal(bits(got), bits(want)):
        raise AssertionError(f"{what}: " + WC.mismatch_report(bits(got), bits(want), pixel_grid=shape))


def check_statistics(what, stats, ref, M, exact):
    s1, s2 = stats[:, 0].double().sum(0), stats[:, 1].double().sum(0)
    if exact:
        assert torch.equal(s1, ref["s1"]) and torch.equal(s2, ref["s2"]), \
            f"{what}: column sums differ from the exact reference sums by at most {float((s1 - ref['s1']).abs().max())} / {float((s2 - ref['s2']).abs().max())}"
    else:
        eps = 2.0 ** -24
        assert bool(((s1 - ref["s1"]).abs() <= M * eps * ref["a1"]).all()) and bool(((s2 - ref["s2"]).abs() <= M * eps * ref["a2"]).all()), \
            f"{what}: column sums outside the fp32 summation bound"


def check_forward(shape, kind, Cout=32, epilogues=(0, 1, 2, 5)):
    """Epilogues 0 and 1 (with and without out) and the linear epilogues 2 and 5 of one (shape, lattice): bit-identical outputs, statistics exact
    (rounding lattice: within n * 2^-24 * sum |term|)."""
    B, H, W = shape
    M = B * H * W
    img, wf = fwd_operands(shape, kind, Cout)
    ibuf, iv = image_slice(img)
    wfd = wf.to(DEVICE)
    what = f"stem forward {sid(shape)} {kind} Cout {Cout}"
    ref = fwd_reference(shape, kind, Cout, 1, 0, DEVICE)
    if 0 in epilogues:
        out, _ = launch_forward(shape, iv, wfd, Cout, 0)
        _same_bits(what + " epilogue 0", shape, out, ref["out"])
    if 1 in epilogues:
        out, st = launch_forward(shape, iv, wfd, Cout, 1)
        _same_bits(what + " epilogue 1", shape, out, ref["out"])
        check_statistics(what + " epilogue 1", st, ref, M, kind != "round")
        _, st2 = launch_forward(shape, iv, wfd, Cout, 1, with_out=False)
        check_statistics(what + " epilogue 1 without out", st2, ref, M, kind != "round")
        assert torch.equal(bits(st), bits(st2)), f"{what}: the statistics-only pass differs from the storing pass"
    sc, sh = (t.to(DEVICE) for t in affine_coefficients(shape, R.LINEAR))
    z = {}
    for epi in (2, 5):
        if epi in epilogues:
            r = fwd_reference(shape, kind, Cout, epi, R.LINEAR, DEVICE)
            z[epi] = R.round_bf16(r["out"])
            out, _ = launch_forward(shape, iv, wfd, Cout, epi, scale=sc, shift=sh, act=R.LINEAR)
            _same_bits(what + f" epilogue {epi} linear", shape, out, z[epi])
    if kind == "round" and len(z) == 2:
        assert not torch.equal(bits(z[2]), bits(z[5])), "test bug: epilogues 2 and 5 agree everywhere on this lattice: the case cannot tell them apart"
    assert bool(torch.isnan(ibuf[:IMG_PAD]).all()) and bool(torch.isnan(ibuf[-IMG_PAD:]).all())


def check_forward_activation(shape, act, tally=None):
    """Epilogues 2 and 5 with Mish / LeakyReLU / SiLU on the rounding lattice, u exact in fp32.  LeakyReLU: bit-identical to the single rounding of
    the 0.1 product.  Mish / SiLU: within one bf16 ulp of the reference plus ew_ref's evaluation bound, at least 99 % bit-identical."""
    img, wf = fwd_operands(shape, "round")
    _, iv = image_slice(img)
    wfd = wf.to(DEVICE)
    sc, sh = (t.to(DEVICE) for t in affine_coefficients(shape, act))
    worst = 0.0
    for epi in (2, 5):
        r = fwd_reference(shape, "round", 32, epi, act, DEVICE)
        out, _ = launch_forward(shape, iv, wfd, 32, epi, scale=sc, shift=sh, act=act)
        what = f"stem forward {sid(shape)} epilogue {epi} act {act}"
        if act == R.LEAKY:
            _same_bits(what, shape, out, SR.leaky_bits(r["u"]))
            continue
        exp = r["out"]
        err, lim = (out.double() - exp).abs(), R.bf16_ulp(exp) + r["bound"]
        worst = max(worst, float((err / lim).max()))
        same = bits(out) == bits(R.round_bf16(exp))
        print(f"{what}: worst error / (one ulp + evaluation bound) = {float((err / lim).max()):.3f}, bit-identical {float(same.double().mean()):.4f}")
        assert bool((err <= lim).all()), f"{what}: {int((err > lim).sum())} of {err.numel()} elements past one bf16 ulp + the fp32 evaluation bound"
        assert int(same.sum()) >= 0.99 * same.numel(), f"{what}: only {int(same.sum())} of {same.numel()} elements are bit-identical to the reference"
    return worst


def check_argument_errors():
    """The refusals `ryolo_stem3x3_fwd` / `_bwd` / `_bwd_plan` document: nothing is launched."""
    hip, S = _lib()
    ARG, UNSUPPORTED = 1, 4
    img = torch.zeros(1, 3, 4, 32, device=DEVICE)
    wf = torch.zeros(32, 32, dtype=torch.bfloat16, device=DEVICE)
    out = torch.zeros(4 * 32 + 8, 40, dtype=torch.bfloat16, device=DEVICE)
    st = torch.zeros(64, 2, 32, device=DEVICE)

    def fwd(**kw):
        p = S.StemParams()
        p.img, p.NB, p.H, p.W, p.wf, p.Cout, p.epi, p.out, p.ldC, p.stats = img.data_ptr(), 1, 4, 32, wf.data_ptr(), 32, 0, out.data_ptr(), 40, st.data_ptr()
        for k, v in kw.items():
            setattr(p, k, v)
        return hip.lib().ryolo_stem3x3_fwd(p, hip.stream())
    assert fwd() == 0
    assert fwd(Cout=12) == UNSUPPORTED and fwd(Cout=40) == UNSUPPORTED and fwd(Cout=0) == UNSUPPORTED
    assert fwd(out=None) == ARG and fwd(out=None, epi=2) == ARG and fwd(out=None, epi=1) == 0
    assert fwd(out=out.data_ptr() + 8) == UNSUPPORTED and fwd(ldC=36) == UNSUPPORTED
    assert fwd(epi=3) == ARG and fwd(epi=1, stats=None) == ARG and fwd(epi=2) == ARG
    ws = S.Z()
    assert hip.lib().ryolo_stem3x3_bwd_plan(1, 4, 48, 32, ws) == UNSUPPORTED and hip.lib().ryolo_stem3x3_bwd_plan(1, 4, 32, 16, ws) == UNSUPPORTED
    assert hip.lib().ryolo_stem3x3_bwd_plan(1, 4, 32, 32, ws) == 0
    work = torch.zeros(ws.value // 4, device=DEVICE)
    dz = torch.zeros(4 * 32 + 8, 40, dtype=torch.bfloat16, device=DEVICE)
    co = torch.ones(4, 32, device=DEVICE)
    dW = torch.zeros(32, 27, device=DEVICE)

    def bwd(**kw):
        q = S.StemBwdParams()
        q.img, q.NB, q.H, q.W, q.dz, q.lddz, q.wf, q.co, q.act, q.frozen = img.data_ptr(), 1, 4, 32, dz.data_ptr(), 40, wf.data_ptr(), co.data_ptr(), 0, 1
        q.workspace, q.dW = work.data_ptr(), dW.data_ptr()
        for k, v in kw.items():
            setattr(q, k, v)
        return hip.lib().ryolo_stem3x3_bwd(q, hip.stream())
    assert bwd() == 0
    assert bwd(W=16) == UNSUPPORTED and bwd(lddz=36) == UNSUPPORTED and bwd(dz=dz.data_ptr() + 8) == UNSUPPORTED
    assert bwd(dW=None) == ARG and bwd(co=None) == ARG and bwd(workspace=None) == ARG
    torch.cuda.synchronize()


def run_no_lds():
    """(child process under RYOLO_STEM_NO_LDS=1) the register-gather kernel's `aligned` branch: the W % 32 == 0 shapes on the three lattices."""
    import time
    for shape in LDS_SHAPES:
        for kind in KINDS:
            t0 = time.perf_counter()
            check_forward(shape, kind)
            print(f"{sid(shape)} {kind}: ok, {time.perf_counter() - t0:.2f} s", flush=True)


# ------------------------------------------------------------------------------------------------ fused weight gradient
def launch_wgrad(shape, iv, dz, y, co, bco, act):
    """`ryolo_stem3x3_wgrad` with y != null -> scratch [32][32] fp32; guards asserted."""
    hip, S = _lib()
    B, H, W = shape
    wsb = S.Z()
    hip.call("ryolo_stem3x3_plan", B, H, W, 32, None, wsb)
    work, ng = workspace(wsb.value)
    scratch = torch.full((3, 32, 32), 3.0, device=DEVICE)
    q = S.StemWgradParams()
    q.img, q.NB, q.H, q.W = iv.data_ptr(), B, H, W
    q.dY, q.ldY, q.Cout, q.scratch, q.workspace = dz.data_ptr(), dz.stride(0), 32, scratch[1].data_ptr(), work.data_ptr() + 4 * ng
    q.y, q.ldy, q.act, q.co, q.bco = y.data_ptr(), y.stride(0), act, co.data_ptr(), bco.data_ptr()
    hip.call("ryolo_stem3x3_wgrad", q, hip.stream())
    torch.cuda.synchronize()
    assert bool((scratch[0] == 3.0).all()) and bool((scratch[2] == 3.0).all()), "fused wgrad: wrote outside the scratch"
    assert workspace_guards_intact(work, ng), "fused wgrad: wrote outside the planned workspace"
    return scratch[1]


def _report_dw(what, got, want):
    """got, want [32][27] fp32 (k = tap*3 + c)."""
    if not torch.equal(bits(got), bits(want)):
        v = lambda t: t.reshape(32, 9, 3).permute(0, 2, 1)
        raise AssertionError(f"{what}: " + WC.mismatch_report(v(got), v(want)))


def wgrad_reference(shape, act, device):
    img, dz, y, co, bco = wgrad_operands(shape)
    d = lambda t: t.to(device)
    ref, info = SR.wgrad_fused(d(img), d(dz)[:, :32], d(y)[:, :32], d(co), d(bco), act)
    SR.assert_no_blind_pixels(img, dz)
    assert torch.equal(info["u"].to(torch.float32).double(), info["u"]), "test bug: u is not exact in fp32"
    if act == R.LINEAR:
        SR.prove_dy_exact(info, 0.25)
    return ref, info


def check_wgrad(shape, act):
    """Linear: scratch[:, :27] equals the reference exactly.  Mish / SiLU: per element, from the reference alone, sum_p |patch| * (|sc| |dz| E_p +
    2^-9 |dy_p| + ew_ref's fp32 evaluation bound of sc*g + A*y + B) + n * 2^-24 * sum |term|, E_p = act_eval_rel(u) * max(|act'(u)|, 1),
    asserted at twice the bound.  Returns the worst error / bound."""
    img, dz, y, co, bco = wgrad_operands(shape)
    _, iv = image_slice(img)
    _, dzv = rows_slice(dz)
    _, yv = rows_slice(y)
    got = launch_wgrad(shape, iv, dzv, yv, co.to(DEVICE), bco.to(DEVICE), act)
    ref, info = wgrad_reference(shape, act, DEVICE)
    what = f"fused stem wgrad {sid(shape)} act {act}"
    assert float(got[:, 27:].abs().max()) == 0.0, f"{what}: padding columns of the scratch are not zero"
    if act == R.LINEAR:
        want = ref.float()
        assert torch.equal(want.double(), ref)
        _report_dw(what, got[:, :27], want)
        return 0.0
    sc = co[2].double().to(DEVICE)
    P, M = info["P"].abs(), info["P"].shape[0]
    E = R.act_eval_rel(info["u"], act) * info["d"].abs().clamp_min(1.0)
    mg, mx = bco[0].double().to(DEVICE), bco[1].double().to(DEVICE)
    _, apply_bound = R.apply_ref(info["g"], y[:, :32].to(DEVICE), co.to(DEVICE), mg, mx)
    per_px = sc.abs() * dz[:, :32].to(DEVICE).double().abs() * E + 2.0 ** -9 * info["dy64"].abs() + apply_bound
    tol = per_px.t() @ P + M * 2.0 ** -24 * info["mag"]
    ratio = float(((got[:, :27].double() - ref).abs() / tol.clamp_min(1e-30)).max())
    print(f"{what}: worst error / bound = {ratio:.3f}")
    assert ratio <= 2.0, f"{what}: {ratio:.3f} times the derived bound (asserted at 2)"
    return ratio


# ------------------------------------------------------------------------------------------------ fused backward
def launch_backward(shape, iv, dzv, wf, co, act, frozen, start):
    """`ryolo_stem3x3_bwd`, twice from the same start values -> (dW [32][27] in k order, dgamma, dbeta); guards asserted."""
    hip, S = _lib()
    B, H, W = shape
    wsb = S.Z()
    hip.call("ryolo_stem3x3_bwd_plan", B, H, W, 32, wsb)
    work, ng = workspace(wsb.value)
    wbuf, w0, wn = WC._guarded(0, 32, 0, 27, DEVICE)
    gbuf, g0, gn = WC._guarded(0, 2, 0, 32, DEVICE)
    q = S.StemBwdParams()
    q.img, q.NB, q.H, q.W = iv.data_ptr(), B, H, W
    q.dz, q.lddz, q.wf, q.co, q.act, q.frozen = dzv.data_ptr(), dzv.stride(0), wf.data_ptr(), co.data_ptr(), act, frozen
    q.workspace, q.dW = work.data_ptr() + 4 * ng, wbuf.data_ptr() + 4 * w0
    q.dgamma, q.dbeta = gbuf.data_ptr() + 4 * g0, gbuf.data_ptr() + 4 * (g0 + 32)
    first = None
    for launch in range(2):
        wbuf[w0:w0 + wn] = start[0].reshape(-1).to(DEVICE)
        gbuf[g0:g0 + 32], gbuf[g0 + 32:g0 + 64] = start[1].to(DEVICE), start[2].to(DEVICE)
        hip.call("ryolo_stem3x3_bwd", q, hip.stream())
        torch.cuda.synchronize()
        if launch:
            assert torch.equal(bits(wbuf), first[0]) and torch.equal(bits(gbuf), first[1]), "fused backward: the second launch from the same start differs from the first"
        first = (bits(wbuf).clone(), bits(gbuf).clone())
    assert bool((wbuf[:w0] == WC.GUARD).all()) and bool((wbuf[w0 + wn:] == WC.GUARD).all()), "fused backward: wrote outside dW"
    assert bool((gbuf[:g0] == WC.GUARD).all()) and bool((gbuf[g0 + gn:] == WC.GUARD).all()), "fused backward: wrote outside dgamma / dbeta"
    assert workspace_guards_intact(work, ng), "fused backward: wrote outside the planned workspace"
    dW = wbuf[w0:w0 + wn].view(32, 3, 9).permute(0, 2, 1).reshape(32, 27)            # torch layout [co][c][tap] -> k = tap*3 + c
    return dW, gbuf[g0:g0 + 32].clone(), gbuf[g0 + 32:g0 + 64].clone()


def backward_reference(shape, kind, frozen, device):
    """Linear activation.  Returns the expected (dW [32][27], dgamma, dbeta) after the accumulation, proven exact from the reference alone.
    Exact lattice: by definition (and identical to the header's formula); rounding lattice: the header's formula, which is the contract."""
    B, H, W = shape
    img, wf, dz, co, start = bwd_operands(shape, kind)
    d = lambda t: t.to(device)
    SR.assert_no_blind_pixels(img, dz)
    dWf, dgf, dbf, parts = SR.backward_by_formula(d(img), d(dz)[:, :32], d(wf), d(co), R.LINEAR, frozen)
    SR.prove_backward(parts, co, B * H * W, frozen, kind != "round")
    if kind != "round":
        dWd, dgd, dbd = SR.backward_by_definition(d(img), d(dz)[:, :32], d(wf), d(co), R.LINEAR, frozen)
        if not (torch.equal(dWd, dWf) and torch.equal(dgd, dgf) and torch.equal(dbd, dbf)):
            SR._bug("the definition and the header's formula differ on an exact lattice")
        dWf, dgf, dbf = dWd, dgd, dbd
    s = [d(t) for t in start]
    dW0k = s[0].view(32, 3, 9).permute(0, 2, 1).reshape(32, 27)
    return SR.accumulate(dW0k, dWf), SR.accumulate(s[1], dgf), SR.accumulate(s[2], dbf)


def check_backward(shape, kind, frozen):
    img, wf, dz, co, start = bwd_operands(shape, kind)
    _, iv = image_slice(img)
    _, dzv = rows_slice(dz)
    want = backward_reference(shape, kind, frozen, DEVICE)
    got = launch_backward(shape, iv, dzv, wf.to(DEVICE), co.to(DEVICE), R.LINEAR, frozen, start)
    what = f"fused stem backward {sid(shape)} {kind} frozen {frozen}"
    _report_dw(what + " dW", got[0], want[0])
    for name, a, b in (("dgamma", got[1], want[1]), ("dbeta", got[2], want[2])):
        bad = bits(a) != bits(b)
        assert not bool(bad.any()), f"{what} {name}: {int(bad.sum())} of 32 channels wrong, first {int(bad.nonzero()[0])}: expected {float(b[bad][0])}, got {float(a[bad][0])}"


def check_backward_activation(shape, act):
    """Mish / SiLU, frozen: dW = sc*G.  tol[co, k] = |sc| * sum_p |patch| * (|dz| E_p + 2^-9 |g_p|) + n * 2^-24 * sum |term|, E_p =
    act_eval_rel(u) * max(|act'(u)|, 1); dgamma / dbeta the same without the bf16 term.  Asserted at twice the bound."""
    img, wf, dz, _, start = bwd_operands(shape, "exact")
    co = nonlinear_coefficients(shape)
    _, iv = image_slice(img)
    _, dzv = rows_slice(dz)
    d = lambda t: t.to(DEVICE)
    dWf, dgf, dbf, p = SR.backward_by_formula(d(img), d(dz)[:, :32], d(wf), d(co), act, 1)
    assert torch.equal(p["u"].to(torch.float32).double(), p["u"]), "test bug: u is not exact in fp32"
    got = launch_backward(shape, iv, dzv, d(wf), d(co), act, 1, start)
    s = [d(t).double() for t in start]
    M = p["P"].shape[0]
    sc, is_, mu = d(co[2]).double(), d(co[1]).double(), d(co[0]).double()
    dza, P = d(dz)[:, :32].double().abs(), p["P"].abs()
    E = R.act_eval_rel(p["u"], act) * p["d"].abs().clamp_min(1.0)
    eps = 2.0 ** -24
    dW0k = s[0].view(32, 3, 9).permute(0, 2, 1).reshape(32, 27)
    want = (dW0k + dWf, s[1] + dgf, s[2] + dbf)
    store = [2.0 ** -23 * (w.abs() + o.abs()) for w, o in zip(want, (dW0k, s[1], s[2]))]      # the rounding to fp32 and the fp32 += onto the start value
    tol_w = sc.abs()[:, None] * ((dza * E + 2.0 ** -9 * p["g"].abs()).t() @ P) + M * eps * (sc.abs()[:, None] * (p["g"].abs().t() @ P)) + store[0]
    ym = p["yb"].abs() + mu.abs()                                                      # dgamma = invstd * (S1 - mean * S0): S1 and S0 are separate fp32 sums
    tol_g = is_.abs() * ((dza * E * ym).sum(0) + M * eps * (p["g"].abs() * ym).sum(0)) + store[1]
    tol_b = (dza * E).sum(0) + M * eps * p["g"].abs().sum(0) + store[2]
    ratios = {"dW": float(((got[0].double() - want[0]).abs() / tol_w).max()),
              "dgamma": float(((got[1].double() - want[1]).abs() / tol_g).max()),
              "dbeta": float(((got[2].double() - want[2]).abs() / tol_b).max())}
    print(f"fused stem backward {sid(shape)} act {act} frozen: worst error / bound {ratios}")
    for k, v in ratios.items():
        assert v <= 2.0, f"fused stem backward {sid(shape)} act {act} {k}: {v:.3f} times the derived bound (asserted at 2)"
    return ratios


# ------------------------------------------------------------------------------------------------ case tables (shared by the GPU file and the CPU proofs)
FORWARD_CASES = [(s, k) for s in LDS_SHAPES + GATHER_SHAPES for k in KINDS]
ACT_SHAPES = [(3, 17, 32), (2, 5, 96), (3, 17, 17), (2, 5, 1)]
COUT_SHAPES = [(2, 5, 96), (2, 9, 48)]                                               # one LDS shape, one gather shape
BACKWARD_CASES = ([(s, "exact", 1) for s in LDS_SHAPES + [LARGE]] + [(s, "exact", 0) for s in POW2_COUNT] + [((2, 16, 32), "round", 0)])
BACKWARD_ACT_SHAPES = [(3, 17, 32), (2, 5, 96)]
