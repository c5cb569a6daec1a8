"""CPU: the recorded execution plans (tests/golden/tapes.json, written once by tests/golden/make_golden_tapes.py from the commit BEFORE the
parameter-block builders and BatchNorm emitters of engine/params.py / engine/graph.py were shared) replayed against the planner under test.
Every launch of every plan must still carry the same name and the same arguments — parameter blocks field by field, pointers as (storage,
offset) with the storage's size: one digest per tape over all of them, and a short tag per entry that names the first one that differs — and
the plan the same stream schedule, gradient-write table, roofline labels, arena size, heads and allocations.  A drift here is not a wrong label but a buffer sized for a different kernel.  No GPU is touched; default knobs are replayed
in-process, every knob setting in a child process of its own (several knobs are read at import).

On a mismatch: `python tests/golden/make_golden_tapes.py --dump <plan> [--env KNOB=VALUE]` here and with --root <checkout of recorded_from>, and diff."""
import os

import pytest

from tests.golden import make_golden_tapes as MT

TABLE = MT.load_table()


def _same(env, plan, want, got):
    """The 16-digit digest of every tape and of the per-plan items is the check; names and 3-digit tags name the first differing entry."""
    where = f"plan {plan} [{MT.env_key(env) or 'default knobs'}]"
    for t in MT.TAPES + ("items",):
        w, g = want[t], got[t]
        for i, (wn, wt, gn, gt) in enumerate(zip(w["names"], w["tags"], g["names"], g["tags"])):
            assert (wn, wt) == (gn, gt), f"{where}: {t}[{i}] differs from the recorded plan: recorded {wn} {wt}, now {gn} {gt}"
        assert len(w["names"]) == len(g["names"]), f"{where}: {t} has {len(g['names'])} entries, recorded {len(w['names'])}"
        assert w["digest"] == g["digest"], f"{where}: {t} differs from the recorded plan in an entry its 3-digit tag does not show ({w['digest']} / {g['digest']})"


def test_table_is_whole():
    assert list(TABLE["plans"]) == [""] + [MT.env_key(e) for e in MT.VARIANTS]
    assert list(TABLE["plans"][""]) == MT.DEFAULT_PLANS and len(MT.DEFAULT_PLANS) == 21
    for e in MT.VARIANTS:
        ps = TABLE["plans"][MT.env_key(e)]
        assert list(ps) == MT.KNOB_PLANS
        assert any(ps[p] != TABLE["plans"][""][p] for p in ps), f"{e} moves no recorded plan"
    for ps in TABLE["plans"].values():
        for p, d in ps.items():
            assert len(d["fwd"]["names"]) > 90 and all(len(d[t]["digest"]) == 16 and len(d[t]["names"]) == len(d[t]["tags"]) for t in d)
            assert (len(d["bwd"]["names"]) > 200, len(d["wprep"]["names"]) > 50) == ((False, True) if "eval" in p else (True, False))


@pytest.mark.parametrize("plan", MT.DEFAULT_PLANS)
def test_default_knobs(plan):
    if any(k.startswith("RYOLO_") and k != "RYOLO_LIB" for k in os.environ):
        got = MT.child_digests({}, [plan])[plan]       # the calling shell sets a knob: the defaults are replayed in a clean child instead
    else:
        got = MT.digests(plan)
    _same({}, plan, TABLE["plans"][""][plan], got)


@pytest.mark.parametrize("n", range(len(MT.VARIANTS)), ids=[MT.env_key(e) for e in MT.VARIANTS])
def test_knob_variant(n):
    env = MT.VARIANTS[n]
    got = MT.child_digests(env, MT.KNOB_PLANS)
    for plan in MT.KNOB_PLANS:
        _same(env, plan, TABLE["plans"][MT.env_key(env)][plan], got[plan])
