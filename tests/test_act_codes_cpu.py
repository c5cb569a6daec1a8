"""CPU: the activation and epilogue codes that Python writes into the parameter blocks (engine/structs.py: ACT, EPI_*) are the enumerators the
kernels compare them with (csrc/act.h: ACT_*, csrc/conv_internal.h: EPI_*).  Nothing else ties the two statements together: a code that
drifts selects another activation or another epilogue without any error."""
import os
import re

from ryolov4_amd.engine import structs

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "r-yolov4_amd", "csrc")
ACT_NAME = {"ACT_LINEAR": "linear", "ACT_MISH": "mish", "ACT_LEAKY": "leaky", "ACT_SILU": "swish"}     # enumerator -> the model's name for it


def _enum(header, prefix):
    """{enumerator: value} of the one `enum { PREFIX_X = n, ... };` of the header (comments between the enumerators allowed)."""
    text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, header)).read())
    bodies = [b for b in re.findall(r"\benum\s*\{([^}]*)\}", text) if prefix in b]
    assert len(bodies) == 1, f"{header}: {len(bodies)} enums with {prefix}* enumerators"
    items = [it.strip() for it in bodies[0].split(",") if it.strip()]
    pairs = [re.fullmatch(rf"({prefix}\w+)\s*=\s*(\d+)", it) for it in items]
    assert all(pairs), f"{header}: enumerator without an explicit value in {items}"
    return {m.group(1): int(m.group(2)) for m in pairs}


def test_act_codes():
    c = _enum("act.h", "ACT_")
    assert set(c) == set(ACT_NAME), f"act.h has {sorted(c)}, this test knows {sorted(ACT_NAME)}"
    assert {ACT_NAME[k]: v for k, v in c.items()} == structs.ACT


def test_epi_codes():
    c = _enum("conv_internal.h", "EPI_")
    py = {k: v for k, v in vars(structs).items() if k.startswith("EPI_")}
    assert c == py
    assert sorted(c.values()) == list(range(len(c)))
