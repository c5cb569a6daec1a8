"""CPU: what the bit-exact weight-gradient tests (tests/test_gpu_wgrad_lattice.py) stand on.

Reference: `wgrad_ref.wgrad_fp64_mag` equals torch's own float64 conv2d autograd exactly on lattices of every tap set the cases use; the
exactness proof (from the reference alone: sum of magnitudes + |dW0| < conv_ref.ABS_LIMIT) passes for every case of the tables of
tests/wgrad_cases.py, rejects a lattice that is too dense, and no case has a blind pixel.

Census: the case tables walked through `ryolo_conv_wgrad_variant` (host only) — default knobs in-process, every knob set in a child of its own,
as tests/test_routing_table_cpu.py does — land on the words the tables name, and their union is exactly the written-out list of instantiations
`wgrad_route`, `w3_geometry` and `w8_geometry` can choose (wgrad_cases.WORDS): a new instantiation without a case fails here."""
import os

import pytest
import torch

from tests import conv_ref as CR
from tests import wgrad_cases as WC
from tests import wgrad_ref as WR


# ------------------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize("k,stride", [((3, 3), 1), ((3, 3), 2), ((1, 3), 1), ((1, 1), 1), ((1, 1), 2)])
@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (1, 6, 4)])
def test_reference_equals_torch_autograd(k, stride, B, H, W):
    Cin, Cout = 4, 5
    kh, kw = k
    ph, pw = (kh - 1) // 2, (kw - 1) // 2
    OH, OW = WR.out_size(H, W, kh, kw, stride)
    gen = torch.Generator().manual_seed(7 * H + kw + stride)
    x, dy, _ = WR.wgrad_lattice(gen, B * H * W, B * OH * OW, Cin, Cout, 8, Cin + 8, 8 + 8, kh * kw)
    ref, mag = WR.wgrad_fp64_mag(x, dy, B, H, W, Cin, Cout, kh, kw, stride, ph, pw)
    w = torch.zeros(Cout, Cin, kh, kw, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(x[:, :Cin].double().view(B, H, W, Cin).permute(0, 3, 1, 2), w, stride=stride, padding=(ph, pw))
    assert y.shape == (B, Cout, OH, OW)
    y.backward(dy[:, :Cout].double().view(B, OH, OW, Cout).permute(0, 3, 1, 2))
    assert torch.equal(ref, w.grad.reshape(Cout, Cin, kh * kw))
    assert torch.equal(ref, WR.wgrad_fp64(x, dy, B, H, W, Cin, Cout, kh, kw, stride, ph, pw))      # the reference of the randn tests agrees
    # mag is the same sum over magnitudes: it bounds the gradient and equals it on operands without signs
    assert bool((mag >= ref.abs()).all())
    ref_abs, _ = WR.wgrad_fp64_mag(x.abs(), dy.abs(), B, H, W, Cin, Cout, kh, kw, stride, ph, pw)
    assert torch.equal(mag, ref_abs)


ALL_CASES = WC.DEFAULT_CASES + [c for _, cases in WC.KNOB_SETS for c in cases]


@pytest.mark.parametrize("c", ALL_CASES, ids=[c.id for c in ALL_CASES])
def test_case_is_provably_exact(c):
    """operands() itself asserts the proof and the no-blind-pixel condition; here also the lattice's ranges, the thinning target and the
    columns around the tensors."""
    B, H, W, Cin, Cout = c.shape
    x, dy, dw0, ref, mag = WC.operands(c)
    coutp = (Cout + 7) // 8 * 8
    assert float(mag.max()) < WR.MAG_TARGET and float(dw0.abs().max()) <= WR.DW0_MAX
    assert float(mag.max()) + float(dw0.abs().max()) < CR.ABS_LIMIT
    assert float(x.float().abs().max()) <= 2 and float(dy.float().abs().max()) <= 1
    assert torch.equal(x.float(), x.float().round()) and torch.equal(dy.float(), dy.float().round()) and torch.equal(dw0, dw0.round())
    assert bool((dy[:, :Cout] != 0).any(1).all()) and bool((x[:, :Cin] != 0).any(1).all())
    assert bool((dy[:, Cout:coutp] == 0).all()) and x.shape[1] == Cin + c.ldx and dy.shape[1] == coutp + c.ldy
    if WC.pixels(c) * 0.8 < 0.9 * WR.MAG_TARGET:                     # thinned only where the bound needs it
        assert float((dy[:, :Cout] != 0).float().mean()) > 0.6
    assert float(ref.abs().max()) > 0


def test_proof_rejects_a_dense_lattice():
    c = WC._c("dense", (40, 60, 44, 32, 40), 0)
    B, H, W, Cin, Cout = c.shape
    gen = torch.Generator().manual_seed(1)
    x, dy, dw0 = WR.wgrad_lattice(gen, B * H * W, B * H * W, Cin, Cout, Cout, Cin, Cout, 9, keep=1.0)
    ref, mag = WR.wgrad_fp64_mag(x, dy, B, H, W, Cin, Cout, 3, 3, 1, 1, 1)
    with pytest.raises(AssertionError, match="test bug"):
        WR.prove_exact_wgrad(mag, dw0)
    WR.prove_exact_wgrad(mag * 0 + (CR.ABS_LIMIT - 65), dw0)        # the rule itself: just inside passes, on the limit fails
    with pytest.raises(AssertionError, match="test bug"):
        WR.prove_exact_wgrad(mag * 0 + (CR.ABS_LIMIT - 64), dw0 * 0 + 64)


def test_blind_pixels_are_repaired_and_detected():
    gen = torch.Generator().manual_seed(2)
    x, dy, _ = WR.wgrad_lattice(gen, 500, 500, 32, 40, 40, 32, 40, 9, keep=0.01)       # nearly every dY row thinned to zero, then repaired
    WR.assert_no_blind_pixels(x, dy, 32, 40)
    assert float((dy != 0).sum(1).float().mean()) < 2
    dy[17] = 0
    with pytest.raises(AssertionError, match="pixel row of dY"):
        WR.assert_no_blind_pixels(x, dy, 32, 40)


# ------------------------------------------------------------------------------------------------ census
def _default_words():
    if any(k.startswith("RYOLO_") and k != "RYOLO_LIB" for k in os.environ):           # the calling shell sets a knob: a clean child instead
        import json
        import subprocess
        import sys
        code = "from tests import wgrad_cases as WC\nimport json\nprint(json.dumps([WC.variant_word(c) for c in WC.DEFAULT_CASES]))\n"
        out = subprocess.check_output([sys.executable, "-c", code], cwd=WC.ROOT, env=WC.knob_env({}), timeout=120)
        return json.loads(out.decode().strip().splitlines()[-1])
    return [WC.variant_word(c) for c in WC.DEFAULT_CASES]


def _named(words):
    return sorted(WC.WORDS.get(w, hex(w)) for w in words)


def test_census_of_instantiations():
    got = list(zip(WC.DEFAULT_CASES, _default_words()))
    for n, (_, cases) in enumerate(WC.KNOB_SETS):
        got += list(zip(cases, WC.child_words(n)))
    wrong = [(c.id, WC.WORDS.get(w, hex(w)), WC.WORDS[c.word]) for c, w in got if w != c.word]
    assert not wrong, f"(case, routed to, written for): {wrong}"
    reached = {w for _, w in got}
    assert WC.NOT_REACHED <= set(WC.WORDS)
    assert reached == set(WC.WORDS) - WC.NOT_REACHED, (f"without a case: {_named(set(WC.WORDS) - WC.NOT_REACHED - reached)}; "
                                                       f"not in the list of instantiations: {_named(reached - set(WC.WORDS))}")


def test_variant_word_agrees_with_the_kernel_code():
    """The reporter makes no second decision: its low byte is what `ryolo_conv_wgrad_kernel` answers, its waves what `_grid` answers."""
    from ryolov4_amd import hip
    from ryolov4_amd.engine import structs as S
    hip.lib()
    for c in WC.DEFAULT_CASES:
        p = WC.params(c)
        word, kern, wgs, waves = S.I(-1), S.I(-1), S.I(-1), S.I(-1)
        hip.call("ryolo_conv_wgrad_variant", p, word)
        hip.call("ryolo_conv_wgrad_kernel", p, kern)
        hip.call("ryolo_conv_wgrad_grid", p, wgs, waves)
        assert word.value & 0xff == kern.value
        assert waves.value == (8 if kern.value == 3 or (kern.value == 1 and (word.value >> 8) & 15) else 4)
    p = WC.params(WC.DEFAULT_CASES[0])
    p.Cin = 40                                                       # a block the launch rejects: the status is the plan's
    word = S.I(-1)
    assert hip.lib().ryolo_conv_wgrad_variant(p, word) == 1 and hip.lib().ryolo_conv_wgrad_variant(None, word) == 1
