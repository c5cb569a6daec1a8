"""CPU: the recorded routing table (tests/golden/routing_table.json, written once by tests/golden/make_golden_routing.py from the library of the
commit BEFORE `gemm_route` / `wgrad_route` existed) replayed against the library under test: every (parameter block, knob setting) must still
get the same status, kernel word and statistics rows from `ryolo_conv_gemm_plan`, and the same statuses, kernel, split-K, workspace bytes,
workgroups and waves from `ryolo_conv_wgrad_plan` / `_kernel` / `_grid`.  Python sizes device buffers from these answers, so a drift here is
not a wrong label but a kernel writing past what was allocated.  No GPU is touched (the plan entry points read the parameter block only);
default knobs are replayed in-process, every knob setting in a child process of its own (a knob is read once per process)."""
import os

import pytest

from tests.golden import make_golden_routing as MG

TABLE = MG.load_table()


def _same(rows, want, got, what):
    assert len(want) == len(got) == len(rows)
    bad = [(r, w, g) for r, w, g in zip(rows, want, got) if w != g]
    assert not bad, f"{len(bad)} of {len(rows)} {what} rows differ from the recorded table; first (row, recorded, now): {bad[:5]}"


def test_table_is_whole():
    assert len(TABLE["fwd"]) == len(TABLE["fwd_out"]) >= 2000 and len(TABLE["wg"]) == len(TABLE["wg_out"]) >= 600
    assert [v["env"] for v in TABLE["variants"]] == MG.VARIANTS
    for v in TABLE["variants"]:
        assert len(v["fwd_idx"]) == len(v["fwd"]) >= 250 and len(v["wg_idx"]) == len(v["wg"]) >= 150


def test_default_knobs():
    if any(k.startswith("RYOLO_") and k != "RYOLO_LIB" for k in os.environ):
        # the calling shell sets a knob: the defaults are replayed in a clean child instead
        got = MG.child_answers({}, MG.TABLE, -1)
    else:
        got = MG.answers(TABLE)
    _same(TABLE["fwd"], TABLE["fwd_out"], got["fwd"], "forward")
    _same(TABLE["wg"], TABLE["wg_out"], got["wg"], "weight-gradient")


@pytest.mark.parametrize("n", range(len(MG.VARIANTS)), ids=[",".join(f"{k}={v}" for k, v in e.items()) for e in MG.VARIANTS])
def test_knob_variant(n):
    v = TABLE["variants"][n]
    got = MG.child_answers(v["env"], MG.TABLE, n)
    _same([TABLE["fwd"][i] for i in v["fwd_idx"]], v["fwd"], got["fwd"], f"forward ({v['env']})")
    _same([TABLE["wg"][i] for i in v["wg_idx"]], v["wg"], got["wg"], f"weight-gradient ({v['env']})")
