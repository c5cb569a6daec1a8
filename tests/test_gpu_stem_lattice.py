"""The first layer's kernels (csrc/stem.hip), bit for bit: `ryolo_stem3x3_fwd` (register-gather and LDS-patch kernels, every epilogue),
`ryolo_stem3x3_wgrad` with y != null and `ryolo_stem3x3_bwd` on integer lattices where the float64 reference (tests/stem_ref.py) itself proves
every sum exact.  The linear activation pins the data path — every pixel, tap, tile, wave range, slab and fold: with power-of-two BatchNorm
coefficients and a power-of-two pixel count the whole fused backward, the rearrangement dW = sc*G + A*(W.XX) + B*X1 and the double-precision
finalize included, equals the gradient computed from the definition.  The activation arms are elementwise and are held to a bound derived
from the reference alone.  Harness, case tables and what each shape is listed for: tests/stem_cases.py; the proofs and the grid facts are
asserted without a GPU by tests/test_stem_ref_cpu.py.

Measured worst error / bound of the derived bounds (asserted at 2): forward Mish / SiLU 0.50 of one ulp + the evaluation bound,
99.55 % or more bit-identical; fused weight gradient < 0.001; frozen fused backward dW 0.14-0.24, dgamma <= 6e-4, dbeta <= 4e-4."""
import subprocess
import sys

import pytest

from tests import ew_ref as R
from tests import stem_cases as SC
from tests import wgrad_cases as WC

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300          # seconds for the child (15 small forward cases; the time is the child's start-up)


@pytest.mark.parametrize("shape,kind", SC.FORWARD_CASES, ids=[f"{SC.sid(s)}-{k}" for s, k in SC.FORWARD_CASES])
def test_forward(shape, kind):
    """Epilogues 0, 1 (with and without out), 2 and 5 (linear, power-of-two scale, integer shift): bit-identical; statistics exact on the exact
    and fractional-image lattices, within n * 2^-24 * sum |term| on the rounding lattice."""
    SC.check_forward(shape, kind)


def test_forward_workload_width():
    """1 x 331 x 800: 8 275 tiles, three per wave on the 4 096 waves of the forward grid with a ragged last range — the only case where the
    prefetch ring turns over in steady state.  Statistics with out, and the rounded affine epilogue; the reference is computed on the device."""
    SC.check_forward(SC.LARGE, "exact", epilogues=(1, 5))


@pytest.mark.parametrize("act", [R.MISH, R.LEAKY, R.SILU])
@pytest.mark.parametrize("shape", SC.ACT_SHAPES, ids=SC.sid)
def test_forward_activation(shape, act):
    SC.check_forward_activation(shape, act)


@pytest.mark.parametrize("Cout", [8, 16, 24])
@pytest.mark.parametrize("shape", SC.COUT_SHAPES, ids=SC.sid)
def test_forward_narrow(shape, Cout):
    """Cout 8 / 16 / 24, raw and statistics: channels >= Cout of out untouched (rows >= Cout of the weights hold ones)."""
    for kind in ("exact", "round"):
        SC.check_forward(shape, kind, Cout=Cout, epilogues=(0, 1))


def test_argument_errors():
    SC.check_argument_errors()


def test_forward_gather_kernel_on_aligned_widths():
    """The register-gather kernel's `aligned` branch is reachable only under RYOLO_STEM_NO_LDS=1 (read once per process): the W % 32 == 0 shapes
    again in one child, with a time limit; the test ends at the child's first non-zero exit."""
    code = "from tests import stem_cases as SC\nSC.run_no_lds()\n"
    r = subprocess.run([sys.executable, "-c", code], cwd=WC.ROOT, env=WC.knob_env({"RYOLO_STEM_NO_LDS": "1"}), capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT)
    print(r.stdout)
    assert r.returncode == 0, f"child exited with {r.returncode}:\n" + r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.count(": ok") == len(SC.LDS_SHAPES) * len(SC.KINDS)


@pytest.mark.parametrize("act", [R.LINEAR, R.MISH, R.SILU])
@pytest.mark.parametrize("shape", SC.WGRAD_SHAPES, ids=SC.sid)
def test_fused_wgrad(shape, act):
    """`ryolo_stem3x3_wgrad` with y != null.  Linear: dy = sc*g + A*y + B exact in fp32, on and off the bf16 grid; scratch[:, :27] equals the
    reference exactly and scratch[:, 27:] is zero.  Mish / SiLU: the derived bound, asserted at 2x."""
    SC.check_wgrad(shape, act)


@pytest.mark.parametrize("shape,kind,frozen", SC.BACKWARD_CASES, ids=[f"{SC.sid(s)}-{k}-frozen{f}" for s, k, f in SC.BACKWARD_CASES])
def test_fused_backward(shape, kind, frozen):
    """`ryolo_stem3x3_bwd`, linear activation: dW, dgamma, dbeta equal the reference added onto the start values, bit for bit — by definition
    on the exact lattice, by the header's formula on the rounding lattice (which pins the bf16 rounding of the recomputed y inside S1)."""
    SC.check_backward(shape, kind, frozen)


@pytest.mark.parametrize("act", [R.MISH, R.SILU])
@pytest.mark.parametrize("shape", SC.BACKWARD_ACT_SHAPES, ids=SC.sid)
def test_fused_backward_activation(shape, act):
    """Frozen BatchNorm, so dW = sc*G: per element within twice the bound derived from the reference alone (tests/stem_cases.py)."""
    SC.check_backward_activation(shape, act)

