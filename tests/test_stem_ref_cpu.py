"""CPU: what the bit-exact first-layer tests (tests/test_gpu_stem_lattice.py) stand on.

Reference: tests/stem_ref.py against torch's own float64 conv2d and float64 autograd through conv -> bf16 straight-through -> BatchNorm (batch
statistics / frozen) -> each of the four activations: `torch.equal` on the exact lattice with the linear activation, 1e-12 relative otherwise;
the fused weight gradient against ew_ref.apply_ref followed by wgrad_ref.wgrad_fp64; the definition and the header's formula of the fused
backward identical on the exact lattice.

Cases: every GPU case of tests/stem_cases.py passes its exactness proof, and the property it is listed for is asserted from the launch arithmetic
of csrc/stem.hip as stem_cases restates it (tiles per wave, idle waves, a ragged last range, interior column blocks): a case that stops
exercising what it is listed for fails here."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as CR
from tests import ew_ref as R
from tests import stem_cases as SC
from tests import stem_ref as SR
from tests import wgrad_ref as WR


def _close(a, b, what=""):
    err, ref = float((a - b).abs().max()), float(b.abs().max())
    assert err <= 1e-12 * max(ref, 1.0), f"{what}: {err} against {ref}"


def _act(u, act):
    return {R.MISH: F.mish, R.LEAKY: lambda t: F.leaky_relu(t, 0.1), R.SILU: F.silu}.get(act, lambda t: t * 1.0)(u)


# ------------------------------------------------------------------------------------------------ reference: forward
@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 4, 32), (2, 3, 1)], ids=SC.sid)
def test_forward_reference_equals_conv2d(shape, kind):
    B, H, W = shape
    img, w = SR.lattice(kind, B, H, W, torch.Generator().manual_seed(3 * W + len(kind)))
    wf = SR.pack_weights(w)
    x = img.to(torch.bfloat16).double()
    y = F.conv2d(x, w, padding=1).permute(0, 2, 3, 1).reshape(-1, 32)
    res = SR.forward(img, wf, 32, 1)
    assert torch.equal(res["y"], y) and torch.equal(res["out"], y.to(torch.bfloat16))
    st = y.to(torch.bfloat16).double()
    assert torch.equal(res["s1"], st.sum(0)) and torch.equal(res["s2"], (st * st).sum(0))
    assert torch.equal(res["mag"], F.conv2d(x.abs(), w.abs(), padding=1).permute(0, 2, 3, 1).reshape(-1, 32))
    assert torch.equal(res["sq"], (y * y).sum(0))
    assert torch.equal(SR.forward(img, wf, 16, 0)["out"], y[:, :16].to(torch.bfloat16))
    sc, sh = SC.affine_coefficients(shape, R.LINEAR)
    for act in R.ACTS:
        for epi, src in ((2, y), (5, st)):
            z = SR.forward(img, wf, 32, epi, sc, sh, act)["out"]
            want = _act(src * sc.double() + sh.double(), act)
            if act == R.LINEAR:
                assert torch.equal(z, want)
            else:
                _close(z, want, f"epilogue {epi} act {act}")
    if kind == "frac":                                                   # the image is no bf16 image, and only round-to-nearest-even gives the lattice back
        base, _ = SR.lattice("exact", B, H, W, torch.Generator().manual_seed(3 * W + len(kind)))
        assert torch.equal(x, base.double()) and not torch.equal(img.double(), x)
        trunc = (img.view(torch.int32) & -65536).view(torch.float32).double()
        half_up = ((img.view(torch.int32) + 0x8000) & -65536).view(torch.float32).double()
        assert not torch.equal(trunc, x) and not torch.equal(half_up, x)


def test_leaky_bits_is_the_single_rounding_of_the_product():
    u = torch.tensor([-3.0, -0.5, 0.0, 2.0, -648.0 / 16 - 3]).double()
    got = SR.leaky_bits(u).double()
    assert torch.equal(got[3:4], u[3:4]) and float(got[2]) == 0.0
    assert float((got[:2] - 0.1 * u[:2]).abs().max()) <= float(R.bf16_ulp(0.1 * u[:2]).max())


# ------------------------------------------------------------------------------------------------ reference: backward against autograd
def _autograd(img, w, dz, gamma, beta, act, frozen, mean=None, invstd=None):
    """float64 autograd through conv -> bf16 straight-through -> BatchNorm -> activation; returns (dW [32][27], dgamma, dbeta, co)."""
    B, _, H, W = img.shape
    w0 = w.clone().requires_grad_()
    gamma, beta = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    y = F.conv2d(img.to(torch.bfloat16).double(), w0, padding=1)
    yr = y + (y.to(torch.bfloat16).double() - y).detach()
    if not frozen:
        mean, var = yr.mean((0, 2, 3)), yr.var((0, 2, 3), unbiased=False)
        invstd = 1.0 / torch.sqrt(var + 1e-5)
    v = lambda t: t[None, :, None, None]
    u = (yr - v(mean)) * v(invstd * gamma) + v(beta)
    (_act(u, act) * dz.double().view(B, H, W, 32).permute(0, 3, 1, 2)).sum().backward()
    co = torch.stack([mean, invstd, gamma * invstd, beta - mean * gamma * invstd]).detach()
    return w0.grad.permute(0, 2, 3, 1).reshape(32, 27), gamma.grad, beta.grad, co


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("frozen", [0, 1])
@pytest.mark.parametrize("kind", ["exact", "round"])
def test_backward_reference_equals_autograd(kind, frozen, act):
    B, H, W = 2, 6, 32
    g = torch.Generator().manual_seed(11 + act)
    img, w = SR.lattice(kind, B, H, W, g)
    dz = SR.dz_lattice(B * H * W, 32, g)
    co0 = SR.bn_lattice(g)
    gamma, beta = co0[2] / co0[1], co0[3] + co0[0] * co0[2]
    dW, dg, db, co = _autograd(img, w, dz, gamma, beta, act, frozen, co0[0], co0[1])
    wf = SR.pack_weights(w)
    d1 = SR.backward_by_definition(img, dz, wf, co, act, frozen)
    d2 = SR.backward_by_formula(img, dz, wf, co, act, frozen)[:3]
    for d in (d1, d2):
        # the gradient of invstd*gamma w.r.t. gamma is invstd: autograd's dgamma is sum g*xhat as the reference states it
        if kind == "exact" and act == R.LINEAR and frozen:
            assert torch.equal(d[0], dW) and torch.equal(d[1], dg) and torch.equal(d[2], db)
        elif kind == "exact" or d is d1 or frozen:
            _close(d[0], dW, "dW"), _close(d[1], dg, "dgamma"), _close(d[2], db, "dbeta")
    if kind == "exact" and act == R.LINEAR and frozen:
        assert all(torch.equal(a, b) for a, b in zip(d1, d2))
    if kind == "exact":
        for a, b in zip(d1, d2):
            _close(a, b, "definition against formula")


def test_formula_uses_the_unrounded_y_in_yx():
    """On the rounding lattice with batch statistics the header's formula is NOT the definition (Yx = W . XX sums the unrounded y): the two
    references differ there, which is why the rounding-lattice GPU case is held to the formula."""
    g = torch.Generator().manual_seed(5)
    img, w = SR.lattice("round", 2, 16, 32, g)
    dz, co = SR.dz_lattice(1024, 32, g), SR.bn_lattice(g)
    a = SR.backward_by_definition(img, dz, SR.pack_weights(w), co, R.LINEAR, 0)
    b = SR.backward_by_formula(img, dz, SR.pack_weights(w), co, R.LINEAR, 0)
    assert not torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert not torch.equal(b[3]["y"], b[3]["yb"])


# ------------------------------------------------------------------------------------------------ reference: fused weight gradient
@pytest.mark.parametrize("act", R.ACTS)
def test_fused_wgrad_reference_equals_apply_then_wgrad(act):
    shape = (3, 17, 16)
    B, H, W = shape
    img, dz, y, co, bco = SC.wgrad_operands(shape)
    ref, info = SR.wgrad_fused(img, dz[:, :32], y[:, :32], co, bco, act)
    _, d = R.act64(co[2].double() * y[:, :32].double() + co[3].double(), act)
    dy, _ = R.apply_ref(dz[:, :32].double() * d, y[:, :32], co, bco[0].double(), bco[1].double())
    if act == R.LINEAR:
        assert torch.equal(dy, info["dy64"])
    else:
        _close(dy, info["dy64"], "dy")
    x = img.to(torch.bfloat16).permute(0, 2, 3, 1).reshape(-1, 3)
    dw = WR.wgrad_fp64(x, info["dyb"], B, H, W, 3, 32, 3, 3, 1, 1, 1)                  # [32, 3, 9]
    _close(ref, dw.permute(0, 2, 1).reshape(32, 27), "dW")
    if act == R.LINEAR:
        assert torch.equal(ref, dw.permute(0, 2, 1).reshape(32, 27))


# ------------------------------------------------------------------------------------------------ cases: proofs
@pytest.mark.parametrize("shape,kind", SC.FORWARD_CASES, ids=[f"{SC.sid(s)}-{k}" for s, k in SC.FORWARD_CASES])
def test_forward_case_is_provably_exact(shape, kind):
    img, wf = SC.fwd_operands(shape, kind)
    res = {e: SC.fwd_reference(shape, kind, 32, e, R.LINEAR, "cpu") for e in (1, 2, 5)}      # asserts the proof, no blind pixel, u exact
    y = res[1]["y"]
    assert torch.equal(wf[:, 27:].float(), torch.zeros(32, 5))
    if kind == "round":
        yb = res[1]["out"].double()
        ties = (y - yb).abs() == R.bf16_ulp(y) / 2
        assert float((yb != y).double().mean()) > 0.02 and int(ties.sum()) > 0, "the rounding lattice must round, ties included"
        assert not torch.equal(R.round_bf16(res[2]["out"]), R.round_bf16(res[5]["out"])), "epilogues 2 and 5 cannot be told apart"
    else:
        assert float(res[1]["sq"].max()) < CR.SQ_LIMIT and torch.equal(res[1]["out"].double(), y)
    if kind == "frac":
        assert not torch.equal(img.to(torch.bfloat16).float(), img)
    assert float(y.abs().max()) > 0


@pytest.mark.parametrize("shape", SC.ACT_SHAPES, ids=SC.sid)
def test_activation_case_has_an_exact_argument(shape):
    for act in (R.MISH, R.LEAKY, R.SILU):
        r = SC.fwd_reference(shape, "round", 32, 2, act, "cpu")
        assert float(r["u"].max()) > 2 and float(r["u"].min()) < -2              # both arms of LeakyReLU
        if shape[2] > 1:                                                           # (a one-column image sums 9 taps, not 27)
            assert float(r["u"].max()) > 20 and float(r["u"].min()) < -8         # both sides of Mish's cut-off


@pytest.mark.parametrize("shape", SC.COUT_SHAPES, ids=SC.sid)
@pytest.mark.parametrize("Cout", [8, 16, 24])
def test_narrow_case_is_provably_exact(shape, Cout):
    for kind in ("exact", "round"):
        r = SC.fwd_reference(shape, kind, Cout, 1, R.LINEAR, "cpu")
        assert r["out"].shape[1] == Cout
    assert bool((SC.fwd_operands(shape, "exact", Cout)[1][Cout:, :27] != 0).all())


@pytest.mark.parametrize("shape", SC.WGRAD_SHAPES, ids=SC.sid)
def test_fused_wgrad_case_is_provably_exact(shape):
    ref, info = SC.wgrad_reference(shape, R.LINEAR, "cpu")                             # asserts prove_dy_exact
    assert shape[2] % 16 == 0 and torch.equal(ref.float().double(), ref)
    ties = (info["dy64"] - info["dyb"].double()).abs() == R.bf16_ulp(info["dy64"]) / 2
    assert int(ties.sum()) > 0
    for act in (R.MISH, R.SILU):
        SC.wgrad_reference(shape, act, "cpu")


@pytest.mark.parametrize("shape,kind,frozen", SC.BACKWARD_CASES, ids=[f"{SC.sid(s)}-{k}-frozen{f}" for s, k, f in SC.BACKWARD_CASES])
def test_backward_case_is_provably_exact(shape, kind, frozen):
    dW, dg, db = SC.backward_reference(shape, kind, frozen, "cpu")                     # asserts the proof and definition == formula
    assert shape[2] % 32 == 0 and float(dW.abs().max()) > 64
    if not frozen:
        assert shape in SC.POW2_COUNT


def test_backward_proof_rejects_what_is_not_exact():
    shape = (2, 5, 96)                                                                 # 960 pixels: no power of two
    img, wf, dz, co, _ = SC.bwd_operands(shape, "exact")
    parts = SR.backward_by_formula(img, dz[:, :32], wf, co, R.LINEAR, 0)[3]
    with pytest.raises(AssertionError, match="test bug"):
        SR.prove_backward(parts, co, 960, 0, True)
    co3 = co.clone()
    co3[1] = 3.0 ** -0.5
    with pytest.raises(AssertionError, match="test bug"):
        SR.prove_backward(SR.backward_by_formula(img, dz[:, :32], wf, co3, R.LINEAR, 1)[3], co3, 960, 1, True)
    img_r, wf_r, dz_r, co_r, _ = SC.bwd_operands((2, 16, 32), "round")
    with pytest.raises(AssertionError, match="test bug"):
        SR.prove_backward(SR.backward_by_formula(img_r, dz_r[:, :32], wf_r, co_r, R.LINEAR, 0)[3], co_r, 1024, 0, True)


# ------------------------------------------------------------------------------------------------ cases: what each shape is listed for
def test_grid_facts():
    f = lambda s: SC.lds_grid(s[0] * s[1] * s[2], 4)
    b = lambda s: SC.lds_grid(s[0] * s[1] * s[2], 3)
    assert all(s[2] % 32 == 0 for s in SC.LDS_SHAPES + [SC.LARGE]) and all(s[2] % 32 != 0 for s in SC.GATHER_SHAPES)
    # one column block, both border pieces at once; 2^10 pixels
    assert (2, 16, 32) in SC.LDS_SHAPES and 2 * 16 * 32 == 2 ** 10
    # 51 tiles on 28 waves: 25 with two tiles, one with a single tile, two idle; image seams inside a range; odd H
    for g in (f((3, 17, 32)), b((3, 17, 32))):
        assert (g.tiles, g.waves, g.per_wave, g.busy, g.ragged, g.idle) == (51, 28, 2, 26, 1, 2)
    assert SC.seam_inside_a_range((3, 17, 32), 4) and SC.seam_inside_a_range((3, 17, 32), 3)
    # top and bottom border in the same tile
    assert (2, 1, 64) in SC.LDS_SHAPES
    # interior column blocks (neither the first nor the last of an image row)
    assert 128 // 32 >= 3 and 2 * 8 * 128 == 2 ** 11 and 96 // 32 >= 3 and (2 * 5 * 96) & (2 * 5 * 96 - 1)
    assert f((2, 8, 128)).per_wave == 2 and f((2, 8, 128)).idle == 0
    # the workload's width: three tiles per wave on both grids, a ragged last range, idle waves behind it
    for g, waves in ((f(SC.LARGE), 4096), (b(SC.LARGE), 3072)):
        assert (g.tiles, g.waves, g.per_wave, g.ragged) == (8275, waves, 3, 1) and g.idle > 0
    # gather kernel: tiles that straddle rows and images, a ragged last tile, a one-column image
    assert (3 * 17 * 17) % 32 and (17 * 17) % 32 and 48 % 32 and (1 * 5 * 16) % 32 == 16 and (2, 5, 1) in SC.GATHER_SHAPES
    assert all(SC.gather_blocks(s[0] * s[1] * s[2]) == 1 for s in SC.GATHER_SHAPES)
    assert all(s[2] % 16 == 0 for s in SC.WGRAD_SHAPES) and SC.gather_blocks(2 * 32 * 48) == 3          # three slabs through the fold
    assert set(SC.POW2_COUNT) <= set(SC.LDS_SHAPES)


def test_plan_agrees_with_the_restated_grid():
    """The statistics rows and workspace bytes the library plans are what the restated launch arithmetic gives (host only)."""
    from ryolov4_amd import hip
    from ryolov4_amd.engine import structs as S
    hip.lib()
    for s in SC.LDS_SHAPES + [SC.LARGE] + SC.GATHER_SHAPES:
        M = s[0] * s[1] * s[2]
        rows, ws = S.I(), S.Z()
        hip.call("ryolo_stem3x3_plan", *s, 32, rows, ws)
        import os
        lds = s[2] % 32 == 0 and not os.environ.get("RYOLO_STEM_NO_LDS")
        assert rows.value == (SC.lds_grid(M, 4).blocks if lds else SC.gather_blocks(M))
        assert ws.value == (SC.gather_blocks(M) + 64) * 1024 * 4
        if s[2] % 32 == 0:
            hip.call("ryolo_stem3x3_bwd_plan", *s, 32, ws)
            assert ws.value == (SC.lds_grid(M, 3).blocks + 64) * 2112 * 4
