"""CPU: the stream schedule (engine/schedule.py) — the one statement of which launch runs on which stream and what waits for what.

  * the builders at the smallest sizes: exact operation lists for hand-made tapes;
  * Graph.run, traced through fake streams and events (tests/golden/make_golden_schedules.py), issues for every recorded plan and setting the
    records, waits, launches and hooks that tests/golden/schedules.json recorded from the commit before the schedule was data;
  * sharing implies ordering: for every plan and setting that has an arena layout, every two buffers whose arena ranges intersect have all
    their launches ordered by the schedule's operations (vector clocks over forward-then-backward, computed HERE from the operations and
    not with schedule.intervals, which the layout came from) — and the check finds unordered pairs when the backward schedule is built with
    a lag one larger than the layout's, or the forward schedule without its joins.
No GPU is touched; default knobs are examined in-process, every other setting in a child process of its own (several knobs are read at import).

On a trace mismatch: `python tests/golden/make_golden_schedules.py --dump <plan> [--setting S]` here and with --root <checkout of recorded_from>, and diff."""
import functools
import json
import os
import subprocess
import sys

import pytest

from ryolov4_amd.engine import schedule as SC
from ryolov4_amd.engine.schedule import NO_HOOK, REC, WAIT
from tests.golden import make_golden_schedules as MS

TABLE = MS.load_table()
LOOSE_LAG, NO_JOINS = "yolov7-kfiou-training-64", "yolov7-kfiou-eval-64"      # the plans whose schedules are loosened on purpose


# ---------------------------------------------------------------------------------------------------------------- builders, by hand
def test_no_side_stream_no_schedule():
    assert SC.forward(6, {}, {3}) is None and SC.backward(6, set(), 2, 1) is None
    assert SC.intervals(None, 3) == [(0, 0), (1, 1), (2, 2)]


def test_lane_rule():
    assert [SC.wgrad_lane(n, 1) for n in range(4)] == [0, 0, 0, 0] and [SC.wgrad_lane(n, 3) for n in range(5)] == [0, 1, 2, 0, 1]
    assert SC.wgrad_lane(7, 0) == 0
    assert [SC.wgrad_stream(k) for k in range(3)] == [1, 3, 4]              # stream 2 is the forward tape's (head tails)


def test_forward_builder():
    """0 main | 1, 2 a lane-1 branch | join before 3 | 4 a lane-2 tail | 5 main.  Events: 0 / 1 end-of-tape joins of lanes 1 / 2, then by need."""
    s = SC.forward(6, {1: (True, 1), 2: (False, 1), 4: (True, 2)}, {3})
    assert s.stream == [0, 1, 1, 0, 2, 0] and s.events == 5
    assert s.before == [(), ((REC, 2, 0), (WAIT, 2, 1)), (), ((REC, 3, 1), (WAIT, 3, 0)), ((REC, 4, 0), (WAIT, 4, 2)), ()]
    assert s.after == [()] * 6
    assert s.end == ((REC, 0, 1), (WAIT, 0, 0), (REC, 1, 2), (WAIT, 1, 0))
    assert s.hook == [NO_HOOK] + [(((REC, 0, 1),), 0)] * 5
    assert SC.intervals(s, 6) == [(0, 0), (1, 2), (1, 2), (3, 3), (4, 5), (5, 5)]


def test_forward_join_lands_on_the_next_main_launch():
    """A join point that is itself a side entry: lane 1 is snapshot there, the main stream waits at its next own launch; a join before
    anything ran on lane 1 is nothing."""
    s = SC.forward(5, {1: (True, 1), 2: (True, 1)}, {0, 2})
    assert s.before == [(), ((REC, 2, 0), (WAIT, 2, 1)), ((REC, 3, 1), (REC, 4, 0), (WAIT, 4, 1)), ((WAIT, 3, 0),), ()]
    assert SC.intervals(s, 5) == [(0, 0), (1, 2), (2, 4), (3, 3), (4, 4)]


def test_backward_builder_one_lane_no_lag():
    """Side entries 1, 3, 4.  Events: 0 the join, 1 lane 0's funnel (unused), then one fork per side entry."""
    s = SC.backward(6, {1, 3, 4}, 1, 0)
    assert s.stream == [0, 1, 0, 1, 1, 0] and s.events == 5
    assert s.before == [(), ((REC, 2, 0), (WAIT, 2, 1)), (), ((REC, 3, 0), (WAIT, 3, 1)), ((REC, 4, 0), (WAIT, 4, 1)), ()]
    assert s.after == [()] * 6
    assert s.end == ((REC, 0, 1), (WAIT, 0, 0))
    assert s.hook == [NO_HOOK] + [(((REC, 0, 1),), 0)] * 5
    assert SC.intervals(s, 6) == [(0, 0), (1, 5), (2, 2), (3, 5), (4, 5), (5, 5)]


def test_backward_builder_two_lanes_lag_one():
    """Side entries 1, 3, 4 dealt to lanes 0, 1, 0 = streams 1, 3, 1.  Events: 0 the join, 1 / 2 the lanes' funnels, then per side entry its
    fork and its completion.  The hook at 3 comes after both lanes were used: lane 1 funnels into stream 1, which records the join."""
    s = SC.backward(6, {1, 3, 4}, 2, 1)
    assert s.stream == [0, 1, 0, 3, 1, 0] and s.events == 9
    assert s.before == [(), ((REC, 3, 0), (WAIT, 3, 1)), (), ((WAIT, 4, 0), (REC, 5, 0), (WAIT, 5, 3)), ((WAIT, 6, 0), (REC, 7, 0), (WAIT, 7, 1)), ()]
    assert s.after == [(), ((REC, 4, 1),), (), ((REC, 6, 3),), ((REC, 8, 1),), ()]
    assert s.end == ((REC, 2, 3), (WAIT, 2, 0), (REC, 0, 1), (WAIT, 0, 0))
    both = (((REC, 2, 3), (WAIT, 2, 1), (REC, 0, 1)), 0)
    assert s.hook == [NO_HOOK, (((REC, 0, 1),), 0), (((REC, 0, 1),), 0), both, both, both]
    assert SC.intervals(s, 6) == [(0, 0), (1, 2), (2, 2), (3, 3), (4, 5), (5, 5)]


def test_a_schedule_that_never_joins_is_refused():
    s = SC.backward(3, {1}, 1, 0)
    s.end = ()
    with pytest.raises(RuntimeError, match="never joined"):
        SC.intervals(s, 3)


# ---------------------------------------------------------------------------------------------------------------- sharing implies ordering
def launch_clocks(tapes):
    """tapes: [(length, Schedule | None)] replayed one after the other.  Per launch of the joint timeline (stream, its number on that
    stream from 1, {other stream: how many of its launches have finished before this one starts}).  Every tape must end fully joined."""
    knows, count, out = {0: {}}, {}, []
    for n, s in tapes:
        at = {}

        def apply(ops):
            for kind, e, st in ops:
                mine = knows.setdefault(st, {})
                if kind == REC:
                    at[e] = dict(mine)
                    at[e][st] = count.get(st, 0)
                else:
                    for b, c in at[e].items():
                        mine[b] = max(mine.get(b, 0), c)
        for i in range(n):
            if s is not None:
                apply(s.before[i])
            st = s.stream[i] if s is not None else 0
            count[st] = count.get(st, 0) + 1
            out.append((st, count[st], dict(knows.setdefault(st, {}))))
            if s is not None:
                apply(s.after[i])
        if s is not None:
            apply(s.end)
        assert all(knows[0].get(st, 0) == c for st, c in count.items() if st), "the tape does not end fully joined"
    return out


def _ordered(x, y):
    (sx, nx, kx), (sy, ny, ky) = x, y
    return sx == sy or ky.get(sx, 0) >= nx or kx.get(sy, 0) >= ny


def sharing(uses, off, sizes, clocks):
    """(pairs of buffers whose arena ranges intersect, those of them with two launches that no chain of operations orders)."""
    items = sorted((off[k], off[k] + sizes[k], k) for k in off if sizes[k] and k in uses)
    pairs, bad = 0, []
    for n, (o, e, a) in enumerate(items):
        for o2, _e2, b in items[n + 1:]:
            if o2 >= e:
                break
            pairs += 1
            if not all(_ordered(clocks[p], clocks[q]) for p in uses[a] for q in uses[b]):
                bad.append((a, b))
    return pairs, bad


def examine(plan, serial=False):
    """Under this process's knobs: {"trace": digests of the traced replay, "pairs": memory-sharing buffer pairs | None without a layout,
    "unordered": those that the schedule does not order, "loosened": the same count under the schedule loosened on purpose | None}."""
    from ryolov4_amd.engine import arena
    seen, plan_ = {}, arena.plan

    def spy(dry, *a):                           # the dry graph of Runtime.graph: the only one that knows which launch mentions which buffer
        seen["uses"] = arena.uses(dry)
        return plan_(dry, *a)
    arena.plan = spy
    try:
        g, rt, _m = MS.MT.build_plan(plan)
    finally:
        arena.plan = plan_
    g.serial = serial
    out = {"pairs": None, "unordered": [], "loosened": None}
    if g.layout is not None:
        F, B, lay = len(g.fwd), len(g.bwd), g.layout
        fs, bs = (None, None) if serial else (g.schedule(g.fwd), g.schedule(g.bwd))
        out["pairs"], out["unordered"] = sharing(seen["uses"], lay.off, lay.sizes, launch_clocks([(F, fs), (B, bs)]))
        if plan == LOOSE_LAG and not serial:
            loose = SC.backward(B, g.side_idx, rt.wgrad_lanes, g.lag + 1)
            out["loosened"] = len(sharing(seen["uses"], lay.off, lay.sizes, launch_clocks([(F, fs), (B, loose)]))[1])
        if plan == NO_JOINS and not serial:
            loose = SC.forward(F, g.fwd_side, set())
            out["loosened"] = len(sharing(seen["uses"], lay.off, lay.sizes, launch_clocks([(F, loose), (B, bs)]))[1])
    out["trace"] = MS.trace_digests(g, rt)      # last: it consumes the tapes
    return out


@functools.lru_cache(maxsize=None)
def _examined(setting, plans):
    """{plan: examine()}: each plan is built once per setting, for the trace and the ordering check alike."""
    if not setting and not any(k.startswith("RYOLO_") and k != "RYOLO_LIB" for k in os.environ):
        return {p: examine(p) for p in plans}
    code = f"import json\nfrom tests import test_schedule_cpu as T\nprint(json.dumps({{p: T.examine(p, {setting == MS.SERIAL}) for p in {list(plans)!r}}}))\n"
    out = subprocess.check_output([sys.executable, "-c", code], env=MS.child_env(setting), cwd=MS.ROOT).decode()
    return json.loads(out.strip().splitlines()[-1])


CASES = [("", p) for p in MS.DEFAULT_PLANS] + [(s, p) for s in MS.SETTINGS for p in MS.KNOB_PLANS]


def _case(setting, plan):
    return _examined(setting, (plan,) if not setting else tuple(MS.KNOB_PLANS))[plan]


def test_table_is_whole():
    assert list(TABLE["plans"]) == [""] + MS.SETTINGS and len(MS.SETTINGS) == 8
    assert list(TABLE["plans"][""]) == MS.DEFAULT_PLANS and len(MS.DEFAULT_PLANS) == 21
    for s in MS.SETTINGS:
        assert list(TABLE["plans"][s]) == MS.KNOB_PLANS
        assert any(TABLE["plans"][s][p] != TABLE["plans"][""][p] for p in MS.KNOB_PLANS), f"{s} moves no recorded replay"
    for ps in TABLE["plans"].values():
        for p, d in ps.items():
            assert len(d["fwd"]["tags"]) > 90 and (len(d["bwd"]["tags"]) > 200) == ("eval" not in p)
            assert all(len(d[t]["digest"]) == 16 for t in MS.TAPES)


@pytest.mark.parametrize("setting,plan", CASES, ids=[f"{p}[{s or 'default knobs'}]" for s, p in CASES])
def test_replay_issues_the_recorded_operations(setting, plan):
    """The 16-digit digest of each tape's trace is the check; the 3-digit tags name the first launch around which it differs."""
    want, got = TABLE["plans"][setting][plan], _case(setting, plan)["trace"]
    for t in MS.TAPES:
        w, g = want[t], got[t]
        for i, (wt, gt) in enumerate(zip(w["tags"], g["tags"])):
            assert wt == gt, f"{plan} [{setting or 'default knobs'}]: the replay of {t} differs from the recorded one at launch {i} (or, past the last launch, at the end of the tape)"
        assert len(w["tags"]) == len(g["tags"]) and w["digest"] == g["digest"], f"{plan} [{setting}]: the replay of {t} differs from the recorded one ({w['digest']} / {g['digest']})"


@pytest.mark.parametrize("setting,plan", CASES, ids=[f"{p}[{s or 'default knobs'}]" for s, p in CASES])
def test_buffers_that_share_memory_have_ordered_launches(setting, plan):
    c = _case(setting, plan)
    if setting == "RYOLO_BUFFER_REUSE=0":
        assert c["pairs"] is None               # no layout: one tensor per buffer, nothing shares
        return
    assert c["pairs"] > 0, "no two buffers share memory: the check is vacuous"
    assert c["unordered"] == [], f"{plan} [{setting or 'default knobs'}]: {len(c['unordered'])} of {c['pairs']} memory-sharing buffer pairs have unordered launches, first {c['unordered'][:3]}"


@pytest.mark.parametrize("plan,what", [(LOOSE_LAG, "a lag one larger than the layout's"), (NO_JOINS, "no forward joins")])
def test_the_ordering_check_has_teeth(plan, what):
    c = _case("", plan)
    assert c["unordered"] == [] and c["loosened"] >= 1, f"{plan} replayed with {what}: no unordered pair found"
