"""Fixture `schedules.json`: what Graph.run (engine/graph.py) DOES with streams and events when it replays a plan — every record, wait,
launch and gradient-bucket hook, in order — for the plans of make_golden_tapes.py at default knobs and for yolov7 / yolov5 kfiou under every
setting that moves a launch to another stream or a wait to another place (SETTINGS; one child process per setting).
tests/test_schedule_cpu.py replays the table against the code under test.

How a replay is traced, without a GPU: the plan is built on torch.device("cpu"); then torch.cuda.Event, torch.cuda.current_stream, the graph
module's hip.stream, rt.side_stream and g.dev (an object whose .type is "cuda") are replaced by recording fakes, every tape entry is
replaced in place by a callable that logs (tape index, stream handle) and returns 0, and g.run(g.fwd) and g.run(g.bwd, None, after) are
called; `after` fires at the grad_ready_points of gflat cut in thirds and logs which event rt.side_event holds.  Only these seams are
touched, so the same script traces any commit whose Graph has them.  Streams are named "main" or by the lane rt.side_stream was called
with, events are numbered by first mention within the tape's replay.

What the file stores: per (plan, tape) one sha256 (16 hex digits) of the whole trace — the check — and per launch the first 3 hex digits of
the digest of its own lines (the operations since the previous launch, and the launch), which only serve to NAME the first launch around
which something differs; the operations after the last launch form one more such group.  Traces that several plans share are stored once.

The table is a RECORD of the replay at the commit named in "recorded_from"; it is never regenerated from the code under test (this script
refuses to overwrite it without --force).

    RYOLO_LIB=<libryolo_hip.so> python tests/golden/make_golden_schedules.py --root <checkout of the parent commit> --recorded-from <commit>
    python tests/golden/make_golden_schedules.py --dump yolov7-kfiou-training-64 [--setting RYOLO_WGRAD_LANES=2] [--root <checkout>]   # full text, for diffing
"""
import argparse
import contextlib
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.dont_write_bytecode = True
if __package__:             # plan ids, build_plan and the digest helpers are shared with the tape fixture
    from . import make_golden_tapes as MT
else:
    import make_golden_tapes as MT

TABLE = os.path.join(ROOT, "tests", "golden", "schedules.json")
DEFAULT_PLANS, KNOB_PLANS = MT.DEFAULT_PLANS, MT.KNOB_PLANS
SERIAL = "serial"           # not a knob: Graph.serial set on the finished plan, as bench.py's per-kernel timing passes do
SETTINGS = ["RYOLO_WGRAD_LANES=2", "RYOLO_WGRAD_LANES=3", "RYOLO_WGRAD_LAG=1", "RYOLO_WGRAD_STREAM=0", "RYOLO_FWD_FORK=0", "RYOLO_BUFFER_REUSE=0",
            "RYOLO_HEAD_FUSED=0", SERIAL]
TAPES = ("fwd", "bwd")


class _Stream:
    def __init__(self, name, log):
        self.name, self.log = name, log
        self.cuda_stream = name                     # the handle a launch on this stream is given

    def wait_event(self, ev):
        self.log.append(f"wait {ev.tag()} {self.name}")


@contextlib.contextmanager
def fakes(g, rt, log, numbers):
    """The seams of a replay replaced by fakes that append to `log`; `numbers`: id(event) -> number by first mention."""
    import torch
    from ryolov4_amd.engine import graph as G

    class Event:
        def tag(self):
            return f"e{numbers.setdefault(id(self), len(numbers))}"

        def record(self, stream=None):
            log.append(f"rec {self.tag()} {stream.name if stream is not None else 'main'}")
    main, sides = _Stream("main", log), {}
    saved = (torch.cuda.Event, torch.cuda.current_stream, G.hip.stream, rt.side_stream, g.dev)
    torch.cuda.Event, torch.cuda.current_stream, G.hip.stream = Event, (lambda device=None: main), (lambda: "main")
    rt.side_stream = lambda lane: sides.setdefault(lane, _Stream(f"lane{lane}", log))
    g.dev = types.SimpleNamespace(type="cuda")
    try:
        yield
    finally:
        torch.cuda.Event, torch.cuda.current_stream, G.hip.stream, rt.side_stream, g.dev = saved


def trace(g, rt):
    """{"fwd" / "bwd": [lines of one launch: the operations before it and `launch <index> <stream>`, ..., the lines after the last launch]}.
    The tapes of g are consumed: their entries are replaced by loggers."""
    n = rt.gflat.numel()
    points = g.grad_ready_points([(k * n // 3, (k + 1) * n // 3) for k in range(3)])
    out, log, numbers, groups = {}, [], {}, []

    def launch(handle, i):
        log.append(f"launch {i} {handle}")
        groups.append("\n".join(log))
        del log[:]
        return 0

    def hook(i):
        ev = rt.side_event
        log.append(f"hook {i} {ev.tag() if ev is not None else None}")
    with fakes(g, rt, log, numbers):                # one set of fakes for both replays: a plan may use an event in both tapes
        for t in TAPES:
            tape = getattr(g, t)
            for i, (_fn, _args, name) in enumerate(tape):
                tape[i] = ((lambda handle, i=i: launch(handle, i)), (), name)
            if t == "fwd":
                g.run(tape)
            else:
                g.run(tape, None, {i: (lambda i=i: hook(i)) for i in points if i >= 0})
            out[t] = groups + ["\n".join(log)]
            numbers.clear()
            del groups[:], log[:]
    return out


def trace_digests(g, rt):
    tr = trace(g, rt)
    return {t: {"tags": [MT._h(x, MT.TAG) for x in tr[t]], "digest": MT._h("\n".join(tr[t]))} for t in TAPES}


def digests(plan, serial=False):
    """{"fwd" / "bwd": {"tags", "digest"}} of a plan's replay under this process's knobs."""
    g, rt, _m = MT.build_plan(plan)
    g.serial = serial
    return trace_digests(g, rt)


def dump_text(plan, serial=False):
    g, rt, _m = MT.build_plan(plan)
    g.serial = serial
    tr = trace(g, rt)
    return "\n".join(f"== {t}\n" + "\n".join(tr[t]) for t in TAPES)


def setting_env(setting):
    return {} if setting in ("", SERIAL) else dict([setting.split("=", 1)])


def child_env(setting):
    """The environment of a fresh process with exactly the knobs of `setting` set."""
    e = dict(os.environ)
    for k in [k for k in e if k.startswith("RYOLO_") and k != "RYOLO_LIB"]:
        del e[k]
    e.update(setting_env(setting))
    return e


def child(setting, args, root=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + args + (["--serial"] if setting == SERIAL else []) + (["--root", root] if root else [])
    return subprocess.check_output(cmd, env=child_env(setting), cwd=ROOT).decode()


def child_digests(setting, plans, root=None):
    return json.loads(child(setting, ["--answer", ",".join(plans)], root).strip().splitlines()[-1])


def load_table(path=TABLE):
    """{"recorded_from", "plans": {setting: {plan: digests}}} written out as digests() returns them."""
    with open(path) as f:
        raw = json.load(f)
    pool = [{"tags": [tg[k:k + MT.TAG] for k in range(0, len(tg), MT.TAG)], "digest": dg} for tg, dg in raw["traces"]]
    return {"recorded_from": raw["recorded_from"],
            "plans": {s: {p: {t: pool[i] for t, i in zip(TAPES, idx)} for p, idx in ps.items()} for s, ps in raw["plans"].items()}}


def _write(path, recorded_from, plans):
    pool, at = [], {}

    def ref(d):
        key = ("".join(d["tags"]), d["digest"])
        if key not in at:
            at[key] = len(pool)
            pool.append(list(key))
        return at[key]
    out = {s: {p: [ref(d[t]) for t in TAPES] for p, d in ps.items()} for s, ps in plans.items()}
    with open(path, "w") as f:
        f.write('{\n "recorded_from": ' + json.dumps(recorded_from) + ',\n "plans": {\n')
        f.write(",\n".join(f"  {json.dumps(s)}: {json.dumps(ps, separators=(',', ':'))}" for s, ps in out.items()))
        f.write('\n },\n "traces": [\n' + ",\n".join("  " + json.dumps(x, separators=(",", ":")) for x in pool) + "\n ]\n}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recorded-from", help="commit of the checkout under --root")
    ap.add_argument("--root", help="checkout whose replay is recorded / dumped (default: the one this script lies in)")
    ap.add_argument("--force", action="store_true", help="overwrite an existing table")
    ap.add_argument("--answer", help="(child) print {plan: digests} of the comma-separated plans as one JSON line")
    ap.add_argument("--serial", action="store_true", help="(child, --dump) set Graph.serial on the plan before it is replayed")
    ap.add_argument("--dump", metavar="PLAN", help="print the full trace of a plan")
    ap.add_argument("--setting", default="", help=f"with --dump: one of {SETTINGS} (a fresh process is started)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root) if a.root else ROOT)
    if a.answer is not None:
        print(json.dumps({p: digests(p, a.serial) for p in a.answer.split(",")}))
        return
    if a.dump:
        if a.setting:
            sys.stdout.write(child(a.setting, ["--dump", a.dump], a.root))
        else:
            print(dump_text(a.dump, a.serial))
        return
    if os.path.exists(TABLE) and not a.force:
        sys.exit(f"{TABLE} exists: it records the parent commit's replay and is not regenerated from the code under test (--force to overwrite)")
    if not a.recorded_from:
        sys.exit("--recorded-from <commit> is required")
    plans = {"": child_digests("", DEFAULT_PLANS, a.root)}
    for s in SETTINGS:
        plans[s] = child_digests(s, KNOB_PLANS, a.root)
    assert child_digests("", DEFAULT_PLANS[:3], a.root) == {p: plans[""][p] for p in DEFAULT_PLANS[:3]}, "a fresh process replays differently"
    _write(TABLE, a.recorded_from, plans)
    assert load_table(TABLE)["plans"] == json.loads(json.dumps(plans)), "the written table does not read back"
    n = sum(len(d[t]["tags"]) for ps in plans.values() for d in ps.values() for t in TAPES)
    print(f"wrote {TABLE}: {sum(len(ps) for ps in plans.values())} plans, {n} trace groups, {os.path.getsize(TABLE)} bytes")


if __name__ == "__main__":
    main()
