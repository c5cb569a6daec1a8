"""Every split-K weight-gradient kernel, bit for bit: `ryolo_conv_wgrad` on integer lattices (X in [-2, 2], dY in {-1, 0, 1}, dW0 in [-64, 64]) where
the float64 reference itself proves every fp32 sum exact (tests/wgrad_ref.py: sum of magnitudes + |dW0| < 2^16 lattice units), so
`torch.equal(dW, dW0 + ref)` must hold whatever the K split, the slabs and the reduce order — a pixel dropped at a K-range end, an image seam read
through a tap, a lost ring lap or a ragged output-channel quarter changes an integer.  Harness and case tables: tests/wgrad_cases.py (NaN-poisoned
split-K workspace with guard bands, guard rows around dW and dW2, the instantiation asserted through `ryolo_conv_wgrad_variant`, a second launch
that must reproduce the bits; dW2 / Cout1; channel strides wider than the tensors).  The census of tests/test_wgrad_lattice_cpu.py ties the
tables to the list of instantiations.  The randn tests of test_gpu_wgrad3x3.py / _taps.py / _wgrad1x1.py stay: fp32 rounding at workload sizes is
their question, exactness at the boundaries is this file's.

The first layer's direct kernel (`ryolo_stem3x3_wgrad`, plain form) is held to the same standard on an fp32 lattice image.  Its fused form
(y != null) and `ryolo_stem3x3_bwd` evaluate an activation: with Mish / SiLU they are not exact on a lattice, with the linear activation
(which every arm of act.h supports) they are, and tests/test_gpu_stem_lattice.py pins them bit for bit there."""
import os
import subprocess
import sys

import pytest
import torch

from tests import wgrad_cases as WC
from tests import wgrad_ref as WR

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300          # seconds per knob set (a set is a dozen launches of at most 2 346 pixels; the time is the child's start-up)


def _child(code, env):
    return subprocess.run([sys.executable, "-c", code], cwd=WC.ROOT, env=WC.knob_env(env), capture_output=True, text=True, timeout=CHILD_TIMEOUT)


@pytest.mark.parametrize("c", WC.DEFAULT_CASES, ids=[c.id for c in WC.DEFAULT_CASES])
def test_default_knobs(c):
    if any(k.startswith("RYOLO_") and k != "RYOLO_LIB" for k in os.environ):
        # the calling shell sets a knob (read once per process): the case runs under the defaults in a clean child instead
        n = WC.DEFAULT_CASES.index(c)
        r = _child(f"from tests import wgrad_cases as WC\nWC.run(WC.DEFAULT_CASES[{n}])\n", {})
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    else:
        WC.run(c)


def test_knob_sets():
    """The instantiations that only a knob reaches at small sizes (tests/wgrad_cases.py: KNOB_SETS).  A knob is read once per process, so each set
    runs in a child of its own, one after the other; the first child that exits non-zero — or dies by a signal — ends the test, and nothing
    more is started on the GPU after it."""
    for n, (env, cases) in enumerate(WC.KNOB_SETS):
        r = _child(f"from tests import wgrad_cases as WC\nWC.run_set({n})\n", env)
        print(f"knob set {n + 1} {env}:\n{r.stdout}")
        assert r.returncode == 0, f"knob set {n + 1} {env} exited with {r.returncode}:\n" + r.stdout[-2000:] + r.stderr[-4000:]
        assert r.stdout.count(": ok") == len(cases)


@pytest.mark.parametrize("B,H,W", [(2, 32, 48), (3, 17, 16), (1, 8, 16)])
def test_stem_wgrad_lattice(B, H, W):
    """`ryolo_stem3x3_wgrad` with y == null on an fp32 lattice image: scratch[:, :27] (k = (r * 3 + s) * 3 + c) equals the float64 gradient exactly,
    the padding columns are zero, whatever the scratch and the workspace held; dY has ldY = 48 with lattice values in the columns >= 32."""
    from ryolov4_amd import hip
    from ryolov4_amd.engine import structs as S
    hip.lib()
    S.check_layouts()
    M, ld = B * H * W, 48
    gen = torch.Generator().manual_seed(100 * B + W)
    x, dy, _ = WR.wgrad_lattice(gen, M, M, 3, 32, 32, 3, ld, 9)
    x, dy = x.cuda(), dy.cuda()
    WR.assert_no_blind_pixels(x, dy, 3, 32)
    assert bool((dy[:, 32:] != 0).all())
    ref, mag = WR.wgrad_fp64_mag(x, dy, B, H, W, 3, 32, 3, 3, 1, 1, 1)             # [32, 3, 9]
    WR.prove_exact_wgrad(mag, torch.zeros(1))
    want = ref.permute(0, 2, 1).reshape(32, 27).float()
    img = x.float().view(B, H, W, 3).permute(0, 3, 1, 2).contiguous()
    rows, wsb = S.I(), S.Z()
    hip.call("ryolo_stem3x3_plan", B, H, W, 32, rows, wsb)
    ng = 4096
    ws = torch.full((ng + wsb.value // 4 + ng,), float("nan"), device="cuda")
    scratch = torch.full((3, 32, 32), 3.0, device="cuda")                          # [guard | scratch | guard]
    q = S.StemWgradParams()
    q.img, q.NB, q.H, q.W = img.data_ptr(), B, H, W
    q.dY, q.ldY, q.Cout, q.scratch, q.workspace = dy.data_ptr(), ld, 32, scratch[1].data_ptr(), ws.data_ptr() + 4 * ng
    hip.call("ryolo_stem3x3_wgrad", q, hip.stream())
    torch.cuda.synchronize()
    got = scratch[1]
    if not torch.equal(got[:, :27], want):
        raise AssertionError("stem dW: " + WC.mismatch_report(got[:, :27].reshape(32, 9, 3).permute(0, 2, 1), want.view(32, 9, 3).permute(0, 2, 1)))
    assert float(got[:, 27:].abs().max()) == 0.0
    assert bool((scratch[0] == 3.0).all()) and bool((scratch[2] == 3.0).all()), "wrote outside the scratch"
    assert bool(torch.isnan(ws[:ng]).all()) and bool(torch.isnan(ws[-ng:]).all()), "wrote outside the planned workspace"
