"""Harness and case tables of the bit-exact weight-gradient tests (tests/test_gpu_wgrad_lattice.py on the GPU, tests/test_wgrad_lattice_cpu.py
for the reference, the proofs and the census of instantiations).

One case = one `ryolo_conv_wgrad` launch on integer lattices (tests/wgrad_ref.py) where every fp32 sum is provably exact, so the gradient must equal
dW0 + the float64 reference bit for bit: one pixel dropped for one (co, ci, tap) element changes an integer.  The split-K workspace is poisoned with
NaN (in the engine it holds the previous layer's slabs: a slab row a kernel forgets to write is read as stale data), the gradient tensors and the
workspace sit between guards, the instantiation the launch takes is asserted through `ryolo_conv_wgrad_variant`, and a second launch from the same
dW0 must reproduce the bits.

The tables name, per case, the variant word it must land on; WORDS is the written-out list of every instantiation `wgrad_route`, `w3_geometry` and
`w8_geometry` (csrc/conv.hip, conv3x3.hip, conv3x3_wgrad8.hip) can choose, and the census asserts that the cases reach exactly that list."""
import collections
import json
import os
import subprocess
import sys

import torch

from tests import wgrad_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ------------------------------------------------------------------------------------------------ variant words (include/ryolo.h)
WGV_REG, WGV_REG_P1, WGV_DMA32, WGV_DMA64 = range(4)


def generic(bm, variant):
    return 0 | ((bm // 64) << 8) | (variant << 12)


def ring(v8, pd, step64, co64, mirror):
    return 1 | (v8 << 8) | (pd << 12) | (step64 << 16) | (co64 << 17) | (mirror << 18)


TAPS_DMA, W1X1_8W = 2, 3

WORDS = {
    generic(64, WGV_REG): "conv_wgrad_kernel<64, false>",
    generic(64, WGV_REG_P1): "conv_wgrad_kernel<64, true>",
    generic(128, WGV_REG): "conv_wgrad_kernel<128, false>",
    generic(128, WGV_REG_P1): "conv_wgrad_kernel<128, true>",
    generic(128, WGV_DMA32): "wgrad1x1_dma_kernel<32>",
    generic(128, WGV_DMA64): "wgrad1x1_dma_kernel<64>",
    TAPS_DMA: "wgrad_taps_dma_kernel",
    W1X1_8W: "wgrad1x1_8w_kernel",
    ring(0, 0, 0, 0, 0): "conv3x3_wgrad_kernel<false>",
    ring(0, 0, 0, 1, 0): "conv3x3_wgrad_kernel<true>",
    ring(0, 0, 1, 0, 0): "conv3x3_wgrad64_kernel<false, false>",
    ring(0, 0, 1, 0, 1): "conv3x3_wgrad64_kernel<false, true>",
    ring(0, 0, 1, 1, 0): "conv3x3_wgrad64_kernel<true, false>",
    ring(0, 0, 1, 1, 1): "conv3x3_wgrad64_kernel<true, true>",
    ring(2, 1, 1, 1, 1): "conv3x3_wgrad8_kernel<2>, one prefetch step",
    ring(2, 2, 1, 1, 1): "conv3x3_wgrad8_kernel<2>, two prefetch steps",
    ring(4, 1, 1, 0, 1): "conv3x3_wgrad8_kernel<4>, one prefetch step",
    ring(4, 2, 1, 0, 1): "conv3x3_wgrad8_kernel<4>, two prefetch steps",
}
# conv3x3_wgrad64_kernel<false, false>: the 128-channel tiles drop the mirror only under the A/B knob RYOLO_W3_MIRROR=0 (their ring never exceeds
# 512 rows, so the mirrored head always fits the 80 KiB: w3_geometry) — no knob set of the tables below sets it, and the census says so.
NOT_REACHED = {ring(0, 0, 1, 0, 0)}

# ------------------------------------------------------------------------------------------------ cases
Case = collections.namedtuple("Case", "id shape k stride zeros cout1 ldx ldy word")


def _c(id, shape, word, k=(3, 3), stride=1, zeros=True, cout1=None, ldx=0, ldy=0):
    return Case(id, shape, k, stride, zeros, cout1, ldx, ldy, word)


R8_4, R8_2 = ring(4, 2, 1, 0, 1), ring(2, 2, 1, 1, 1)
DEFAULT_CASES = [
    # M = 216 output pixels of an odd 17 x 23 map: the last output row and column read padding
    _c("taps-3x3s2-64-128", (2, 17, 23, 64, 128), TAPS_DMA, stride=2),
    _c("taps-3x3s2-32-96", (2, 17, 23, 32, 96), TAPS_DMA, stride=2),
    _c("taps-1x3-64-128", (2, 17, 23, 64, 128), TAPS_DMA, k=(1, 3)),                      # reduce chunk 64 (taps <= 4)
    _c("taps-1x1s2-64-128", (2, 17, 23, 64, 128), TAPS_DMA, k=(1, 1), stride=2),
    _c("taps-3x3s1-64-128", (2, 17, 23, 64, 128), TAPS_DMA),                              # too small for the ring
    _c("reg64-3x3s2-32-64", (2, 17, 23, 32, 64), generic(64, WGV_REG), stride=2),         # three column tiles per block
    _c("reg64-3x3s2-64-40", (2, 17, 23, 64, 40), generic(64, WGV_REG), stride=2),         # four column tiles per block, ragged Cout
    _c("dma64-1x1-128-256", (2, 17, 23, 128, 256), generic(128, WGV_DMA64), k=(1, 1)),
    _c("reg64p1-1x1-128-64", (2, 17, 23, 128, 64), generic(64, WGV_REG_P1), k=(1, 1)),
    _c("dma64-1x1-256-136", (2, 17, 23, 256, 136), generic(128, WGV_DMA64), k=(1, 1)),    # reduce chunk 256, ragged second tile
    _c("reg128-3x3s2-64-128-nozeros", (2, 17, 23, 64, 128), generic(128, WGV_REG), stride=2, zeros=None),
    _c("reg128p1-1x1-128-256-nozeros", (2, 17, 23, 128, 256), generic(128, WGV_REG_P1), k=(1, 1), zeros=None),
    _c("ring8-128-256", (3, 62, 62, 128, 256), R8_4),                                     # M = 11 532: multi-split, laps
    _c("ring8-192-200", (3, 62, 62, 192, 200), R8_4),                                     # ragged second output tile
    _c("ring8-64-40", (24, 47, 33, 64, 40), R8_2),                                        # M = 37 224: pixel halves, two slabs per range, ragged quarter
    _c("ring4-s32-32-128", (4, 160, 160, 32, 128), ring(0, 0, 0, 0, 0)),                  # M = 102 400: 32-pixel steps, 132 slabs
    _c("ring4-co64-32-40", (40, 60, 44, 32, 40), ring(0, 0, 1, 1, 1)),                    # M = 105 600
    _c("w8-1x1-1024-396", (12, 25, 25, 1024, 396), W1X1_8W, k=(1, 1)),                    # M = 7 500: 8 tiles, ragged, 8 slabs
    # dW2 / Cout1: two sibling convolutions out of one launch, split where no 32-channel block ends
    _c("taps-3x3s2-64-128-cout1", (2, 17, 23, 64, 128), TAPS_DMA, stride=2, cout1=50),
    _c("ring8-128-256-cout1", (3, 62, 62, 128, 256), R8_4, cout1=100),
    _c("w8-1x1-1024-396-cout1", (12, 25, 25, 1024, 396), W1X1_8W, k=(1, 1), cout1=203),
    # concat slices: channel strides wider than the tensors, lattice values in the neighbouring columns
    _c("taps-3x3s2-32-96-ld", (2, 17, 23, 32, 96), TAPS_DMA, stride=2, ldx=96, ldy=64),
    _c("reg64-3x3s2-64-40-ld", (2, 17, 23, 64, 40), generic(64, WGV_REG), stride=2, ldx=32, ldy=16),
    _c("dma64-1x1-128-256-ld", (2, 17, 23, 128, 256), generic(128, WGV_DMA64), k=(1, 1), ldx=32, ldy=16),
    _c("ring8-64-40-ld", (24, 47, 33, 64, 40), R8_2, ldx=32, ldy=16),
    _c("w8-1x1-1024-396-ld", (12, 25, 25, 1024, 396), W1X1_8W, k=(1, 1), ldx=32, ldy=16),
]

_P1 = dict(k=(1, 1))
KNOB_SETS = [
    ({"RYOLO_W3_FORCE": "1", "RYOLO_WGRAD_8W_FORCE": "1", "RYOLO_WGRAD_8W_MINC": "128"}, [
        _c("s1-ring8-64-128", (2, 17, 23, 64, 128), R8_4),                                # M = 782 from here on
        _c("s1-ring8-64-40", (2, 17, 23, 64, 40), R8_2),
        _c("s1-ring4-s64-32-128", (2, 17, 23, 32, 128), ring(0, 0, 1, 0, 1)),
        _c("s1-ring4-s64-32-40", (2, 17, 23, 32, 40), ring(0, 0, 1, 1, 1)),
        _c("s1-ring8-64-128-splits", (6, 17, 23, 64, 128), R8_4),                         # M = 2 346: several K ranges
        _c("s1-ring4-s32-fallback", (1, 5, 420, 32, 40), ring(0, 0, 0, 1, 0)),            # M = 2 100: 1024-row ring, 32-pixel steps
        _c("s1-ring4-s64-nomirror", (1, 9, 200, 32, 40), ring(0, 0, 1, 1, 0)),            # M = 1 800: 1024-row ring, no room for the mirror
        _c("s1-w8-256-256", (2, 17, 23, 256, 256), W1X1_8W, **_P1),
        _c("s1-w8-320-200", (2, 17, 23, 320, 200), W1X1_8W, **_P1),
        _c("s1-w8-idle-128-256", (2, 17, 23, 128, 256), W1X1_8W, **_P1),
        _c("s1-w8-idle-256-128", (2, 17, 23, 256, 128), W1X1_8W, **_P1),
        _c("s1-w8-idle-192-72", (2, 17, 23, 192, 72), W1X1_8W, **_P1),
    ]),
    ({"RYOLO_W3_FORCE": "1", "RYOLO_W3_V8": "0", "RYOLO_WGRAD_8W": "0", "RYOLO_WGRAD_TAPS_DMA": "0", "RYOLO_WGRAD_P1": "3"}, [
        _c("s2-ring4-s64-64-128", (2, 17, 23, 64, 128), ring(0, 0, 1, 0, 1)),
        _c("s2-ring4-s64-64-40", (2, 17, 23, 64, 40), ring(0, 0, 1, 1, 1)),
        _c("s2-ring4-s64-64-128-splits", (6, 17, 23, 64, 128), ring(0, 0, 1, 0, 1)),
        _c("s2-dma32-256-256", (2, 17, 23, 256, 256), generic(128, WGV_DMA32), **_P1),
        _c("s2-dma32-320-200", (2, 17, 23, 320, 200), generic(128, WGV_DMA32), **_P1),
        _c("s2-reg128-3x3s2-64-128", (2, 17, 23, 64, 128), generic(128, WGV_REG), stride=2),       # register-staged, zero page present
    ]),
    ({"RYOLO_W3_FORCE": "1", "RYOLO_W3_V8_PD": "1", "RYOLO_W3_STEP64": "0"}, [
        _c("s3-ring8-pd1-64-128", (2, 17, 23, 64, 128), ring(4, 1, 1, 0, 1)),
        _c("s3-ring8-pd1-64-40", (2, 17, 23, 64, 40), ring(2, 1, 1, 1, 1)),
        _c("s3-ring4-s32-32-128", (2, 17, 23, 32, 128), ring(0, 0, 0, 0, 0)),
        _c("s3-ring4-s32-32-40", (2, 17, 23, 32, 40), ring(0, 0, 0, 1, 0)),
    ]),
]


def pixels(c):
    B, H, W = c.shape[:3]
    OH, OW = WR.out_size(H, W, c.k[0], c.k[1], c.stride)
    return B * OH * OW


# ------------------------------------------------------------------------------------------------ parameter block
def params(c, dY=0x10000, X=0x20000, dW=0x30000, partial=0x40000, zeros=0x50000, dW2=0x60000):
    """WgradParams of a case.  The default pointers are placeholders for the host-only plan entry points (16-byte aligned like the engine's)."""
    from ryolov4_amd.engine import structs as S
    B, H, W, Cin, Cout = c.shape
    kh, kw = c.k
    ph, pw = (kh - 1) // 2, (kw - 1) // 2
    OH, OW = WR.out_size(H, W, kh, kw, c.stride)
    coutp = (Cout + 7) // 8 * 8
    p = S.WgradParams()
    p.dY, p.ldY, p.Cout, p.CoutPad = dY, coutp + c.ldy, Cout, coutp
    p.X, p.NB, p.IH, p.IW, p.Cin, p.ldX = X, B, H, W, Cin, Cin + c.ldx
    p.OH, p.OW, p.sh, p.sw, p.ntaps = OH, OW, c.stride, c.stride, kh * kw
    for r in range(kh):
        for s in range(kw):
            p.dh[r * kw + s], p.dw[r * kw + s] = r - ph, s - pw
    p.dW, p.partial = dW, partial
    p.zeros = zeros if c.zeros else None
    if c.cout1 is not None:
        p.dW2, p.Cout1 = dW2, c.cout1
    return p


def variant_word(c):
    """What `ryolo_conv_wgrad_variant` answers for the case under this process's knobs (host only: no GPU is touched)."""
    from ryolov4_amd import hip
    from ryolov4_amd.engine import structs as S
    hip.lib()
    word = S.I(-1)
    hip.call("ryolo_conv_wgrad_variant", params(c), word)
    return word.value


def knob_env(env):
    e = {k: v for k, v in os.environ.items() if not (k.startswith("RYOLO_") and k != "RYOLO_LIB")}
    e.update(env)
    return e


def child_words(n):
    """The variant words of knob set n from a fresh process (a knob is read once per process)."""
    code = f"from tests import wgrad_cases as WC\nimport json\nprint(json.dumps([WC.variant_word(c) for c in WC.KNOB_SETS[{n}][1]]))\n"
    out = subprocess.check_output([sys.executable, "-c", code], cwd=ROOT, env=knob_env(KNOB_SETS[n][0]), timeout=120)
    return json.loads(out.decode().strip().splitlines()[-1])


# ------------------------------------------------------------------------------------------------ operands, reference, proof
def operands(c, device="cpu", seed=None):
    """(x, dy, dw0, ref, mag) of a case on `device`; the lattice is drawn on the CPU from a seed fixed by the case's id.  Proves exactness and the
    no-blind-pixel condition before returning (both are conditions of the test)."""
    B, H, W, Cin, Cout = c.shape
    kh, kw = c.k
    ph, pw = (kh - 1) // 2, (kw - 1) // 2
    OH, OW = WR.out_size(H, W, kh, kw, c.stride)
    coutp = (Cout + 7) // 8 * 8
    gen = torch.Generator().manual_seed(sum(map(ord, c.id)) if seed is None else seed)
    x, dy, dw0 = WR.wgrad_lattice(gen, B * H * W, B * OH * OW, Cin, Cout, coutp, Cin + c.ldx, coutp + c.ldy, kh * kw)
    x, dy, dw0 = x.to(device), dy.to(device), dw0.to(device)
    WR.assert_no_blind_pixels(x, dy, Cin, Cout)
    assert bool((dy[:, Cout:coutp] == 0).all())
    assert c.ldy == 0 or bool((dy[:, coutp:] != 0).all())
    assert c.ldx == 0 or bool((x[:, Cin:] != 0).all())
    ref, mag = WR.wgrad_fp64_mag(x, dy, B, H, W, Cin, Cout, kh, kw, c.stride, ph, pw)
    WR.prove_exact_wgrad(mag, dw0)
    return x, dy, dw0, ref, mag


def mismatch_report(got, want, co0=0, pixel_grid=None):
    """Where a [rows, Cin, taps] gradient differs from the expected one: enough to point at a boundary without a second run.
    With pixel_grid = (B, H, W) the tensors are [pixels, channels] outputs of a stride-1 layer instead (compared as given: pass bit
    patterns to tell +0.0 from -0.0): first (pixel, channel), counts per image and per 32-pixel column block of the image rows."""
    if pixel_grid is not None:
        B, H, W = pixel_grid
        bad = got != want
        if got.is_floating_point():
            bad = bad | torch.isnan(got)
        p, ch = (int(v) for v in bad.nonzero()[0])
        per_px = bad.view(B, H, W, -1).sum(3)
        blocks = [int(per_px[:, :, 32 * b:32 * b + 32].sum()) for b in range((W + 31) // 32)]
        return (f"{int(bad.sum())} of {bad.numel()} elements wrong; first (pixel, channel) = ({p}, {ch}) = image {p // (H * W)}, row {p // W % H}, column "
                f"{p % W}: expected {want[p, ch].item()}, got {got[p, ch].item()}; wrong per image {per_px.sum((1, 2)).tolist()}; per 32-pixel column "
                f"block {blocks}; per channel {bad.sum(0).tolist()}")
    bad = (got != want) | torch.isnan(got)
    n = int(bad.sum())
    idx = bad.nonzero()
    co, ci, t = (int(v) for v in idx[0])
    taps = bad.sum((0, 1)).tolist()
    nblk = (bad.shape[1] + 31) // 32
    blocks = [int(bad[:, 32 * b:32 * b + 32].sum()) for b in range(nblk)]
    rows = torch.arange(bad.shape[0], device=bad.device) + co0
    quarters = {int(q): int(bad[rows // 32 == q].sum()) for q in torch.unique(rows // 32)}
    return (f"{n} of {bad.numel()} elements wrong; first (co, ci, tap) = ({co + co0}, {ci}, {t}): expected {float(want[co, ci, t])}, got {float(got[co, ci, t])}; "
            f"wrong per tap {taps}; per 32-channel input block {blocks}; per 32-channel output quarter {quarters}")


DEVICE = "cuda:0"
GUARD = 4096.5                  # fill of the guard rows: no lattice value equals it, and adding any non-zero integer changes it
WS_GUARD_BYTES = 1 << 16


def _guarded(rows_before, rows, rows_after, row_len, device):
    """One fp32 buffer [guard | rows | guard] filled with GUARD; returns (buffer, offset of the payload, payload length) in floats."""
    g = max(1024, 2 * row_len)
    n0, n = g + rows_before * row_len, rows * row_len
    buf = torch.full((n0 + n + rows_after * row_len + g,), GUARD, dtype=torch.float32, device=device)
    return buf, n0, n


def run_case(B, H, W, Cin, Cout, k, stride, *, ldx_extra=0, ldy_extra=0, zeros=True, cout1=None, expect_word, name="case"):
    """One launch of `ryolo_conv_wgrad` on the GPU, in the order of the module docstring."""
    from ryolov4_amd import hip
    from ryolov4_amd.engine import structs as S
    hip.lib()
    S.check_layouts()
    dev = DEVICE
    c = Case(name, (B, H, W, Cin, Cout), tuple(k), stride, zeros, cout1, ldx_extra, ldy_extra, expect_word)
    # 1. lattice, reference, proof (from the reference alone)
    x, dy, dw0, ref, mag = operands(c, dev)
    want = (dw0.double() + ref).float()
    assert torch.equal(want.double(), dw0.double() + ref)             # integers below 2^24: the fp32 image of the expected gradient is exact
    ntaps, row = k[0] * k[1], Cin * k[0] * k[1]
    n1 = Cout if cout1 is None else cout1
    # 2. workspace: planned bytes between two guard bands, all of it NaN
    p = params(c, dy.data_ptr(), x.data_ptr())
    sk, ws = S.I(), S.Z()
    hip.call("ryolo_conv_wgrad_plan", p, sk, ws)
    assert ws.value % 4 == 0 and ws.value == sk.value * Cout * row * 4
    nws, ng = ws.value // 4, WS_GUARD_BYTES // 4
    work = torch.full((ng + nws + ng,), float("nan"), dtype=torch.float32, device=dev)
    # 3. guard rows around dW (rows >= Cout1 of a shared launch are guard too: they belong to dW2) and around dW2
    wbuf, w0, wn = _guarded(0, n1, Cout - n1, row, dev)
    wbuf[w0:w0 + wn] = dw0[:n1].reshape(-1)
    zpage = torch.zeros(256, dtype=torch.uint8, device=dev)
    if cout1 is not None:
        w2buf, v0, vn = _guarded(0, Cout - n1, n1, row, dev)
        w2buf[v0:v0 + vn] = dw0[n1:].reshape(-1)
    p = params(c, dy.data_ptr(), x.data_ptr(), wbuf.data_ptr() + 4 * w0, work.data_ptr() + 4 * ng, zpage.data_ptr(),
               w2buf.data_ptr() + 4 * v0 if cout1 is not None else 0)
    # 4. the instantiation
    word = S.I(-1)
    hip.call("ryolo_conv_wgrad_variant", p, word)
    assert word.value == expect_word, (f"{name}: routed to {WORDS.get(word.value, hex(word.value))} ({word.value:#x}), the case is written for "
                                       f"{WORDS[expect_word]} ({expect_word:#x})")
    results = []
    for launch in range(2):
        if launch:                                                    # 8. again from the same dW0 (the workspace now holds the first launch's slabs)
            wbuf[w0:w0 + wn] = dw0[:n1].reshape(-1)
            if cout1 is not None:
                w2buf[v0:v0 + vn] = dw0[n1:].reshape(-1)
        # 5. launch
        hip.call("ryolo_conv_wgrad", p, hip.stream())
        torch.cuda.synchronize()
        if launch:
            assert torch.equal(wbuf, results[0]), f"{name}: the second launch from the same dW0 differs from the first"
            assert cout1 is None or torch.equal(w2buf, results[1]), f"{name}: dW2 of the second launch differs from the first"
            break
        results = [wbuf.clone(), w2buf.clone() if cout1 is not None else None]
        # 6. bit-exact gradient(s)
        got = wbuf[w0:w0 + wn].view(n1, Cin, ntaps)
        if not torch.equal(got, want[:n1]):
            raise AssertionError(f"{name} [{WORDS[expect_word]}, splitk {sk.value}] dW: " + mismatch_report(got, want[:n1]))
        if cout1 is not None:
            got2 = w2buf[v0:v0 + vn].view(Cout - n1, Cin, ntaps)
            if not torch.equal(got2, want[n1:]):
                raise AssertionError(f"{name} [{WORDS[expect_word]}, splitk {sk.value}] dW2: " + mismatch_report(got2, want[n1:], co0=n1))
        # 7. guards
        assert bool((wbuf[:w0] == GUARD).all()) and bool((wbuf[w0 + wn:] == GUARD).all()), f"{name}: wrote outside dW"
        if cout1 is not None:
            assert bool((w2buf[:v0] == GUARD).all()) and bool((w2buf[v0 + vn:] == GUARD).all()), f"{name}: wrote outside dW2"
        assert bool(torch.isnan(work[:ng]).all()) and bool(torch.isnan(work[ng + nws:]).all()), f"{name}: wrote outside the planned workspace"


def run(c):
    B, H, W, Cin, Cout = c.shape
    run_case(B, H, W, Cin, Cout, c.k, c.stride, ldx_extra=c.ldx, ldy_extra=c.ldy, zeros=c.zeros, cout1=c.cout1, expect_word=c.word, name=c.id)


def run_set(n):
    """(child process) every case of knob set n, in order; the first failure ends the process with its message."""
    import time
    for c in KNOB_SETS[n][1]:
        t0 = time.perf_counter()
        run(c)
        print(f"{c.id}: ok, {time.perf_counter() - t0:.2f} s", flush=True)
