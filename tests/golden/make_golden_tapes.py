"""Fixture `tapes.json`: the execution plans of engine/graph.py, launch by launch — for every version x mode x {eval, training, frozen
training} at B = 2, 64 x 64 (yolov7 kfiou also at 128 x 128), and for yolov7 / yolov5 kfiou under every planning knob (one child process per
setting: several knobs are read at import).  tests/test_tapes_cpu.py replays the table against the code under test.

Canonical form of a plan (`canon`): per tape entry its name and every argument, parameter blocks written out field by field (nested arrays
included).  Every integer argument or field that lies inside the storage of a tensor the plan or the runtime owns (g.keep, g.arena, g.img, the
model's parameters and buffers, the runtime's flat buffers, `zeros` and packed weights) is written as `@rank:bytes+offset`, rank = order of
first mention of that storage in the dump, bytes = its size.  A non-null pointer field, or any value >= 2^32, that lies in NO owned storage
fails the dump: nothing escapes canonicalisation.  Python-callable entries (copy_slice, zero_scratch) are recorded by name.  Per plan also:
side_idx, fwd_side, fwd_join, grad_writes, meta, layout.total, the heads and the keep list (what was allocated, in order).
What the file stores, so that it stays small enough to read in a diff (30 000 entries): per TAPE one sha256 (16 hex digits) of its whole canonical
text — the check: any difference in any entry changes it — and per entry its name (one character, an index into "names") and the first 3 hex
digits of its own sha256, which only serve to NAME the first differing entry; likewise one 16-digit digest of the per-plan items and 3 digits per
item.  Name sequences and tapes that several plans share are stored once ("name_lists", "tapes").

The table is a RECORD of the planner at the commit named in "recorded_from"; it is never regenerated from the code under test (this script
refuses to overwrite it without --force).  It reads only what that commit's Graph exposes.  Plans build without a GPU.

    RYOLO_LIB=<libryolo_hip.so> python tests/golden/make_golden_tapes.py --root <checkout of the parent commit> --recorded-from <commit>
    python tests/golden/make_golden_tapes.py --dump yolov7-kfiou-training-64 [--env RYOLO_HEAD_FUSED=0] [--root <checkout>]    # full text, for diffing
"""
import argparse
import bisect
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.dont_write_bytecode = True
TABLE = os.path.join(ROOT, "tests", "golden", "tapes.json")

KINDS = {"eval": (False, False), "training": (True, False), "frozen": (True, True)}
MODES = {"csl": 2, "kfiou": 16}
DEFAULT_PLANS = [f"{ver}-{mode}-{kind}-64" for ver in ("yolov4", "yolov5", "yolov7") for mode in MODES for kind in KINDS] + \
                [f"yolov7-kfiou-{kind}-128" for kind in KINDS]
KNOB_PLANS = [f"{ver}-kfiou-{kind}-64" for ver in ("yolov7", "yolov5") for kind in ("training", "eval")]
VARIANTS = [{"RYOLO_HEAD_FUSED": "0"}, {"RYOLO_HEAD_FOLD_A": "0"}, {"RYOLO_HEAD_SPARSE": "0"}, {"RYOLO_STEM_RECOMPUTE": "0"},
            {"RYOLO_STEM_RECOMPUTE": "0", "RYOLO_FUSE_STEM_BN": "0"}, {"RYOLO_S2D_DGRAD": "0"}, {"RYOLO_FUSE_POOL_GRAD": "0"},
            {"RYOLO_MERGE_SIBLINGS": "0"}, {"RYOLO_FOLD_REPCONV": "0"}, {"RYOLO_BUFFER_REUSE": "0"}, {"RYOLO_WGRAD_STREAM": "0"},
            {"RYOLO_WGRAD_LANES": "2"}, {"RYOLO_FWD_FORK": "0"}]
TAPES = ("wprep", "fwd", "bwd")
TAG = 3                     # hex digits of an entry's own digest kept to locate a difference (the 16-digit tape digest is the check)


def env_key(env):
    return ",".join(f"{k}={v}" for k, v in env.items())


class Escaped(Exception):
    """A pointer-like value that no owned storage holds."""


class _Owned:
    """The storages a plan may point into, and their ranks by first mention."""

    def __init__(self, g, rt, model):
        import torch
        iv = {}

        def add(t):
            if isinstance(t, torch.Tensor) and t.device.type != "meta":
                st = t.untyped_storage()
                if st.nbytes():
                    iv[st.data_ptr()] = st.nbytes()
        for k in g.keep:
            if isinstance(k, torch.Tensor):
                add(k)
            elif hasattr(k, "t") and hasattr(k, "g"):           # a Buf: activation and (lazily) its gradient twin
                add(k.t)
                add(k.g)
        for t in [g.arena, g.img, rt.flat, rt.gflat, rt.zeros, rt.nbt] + list(model.parameters()) + list(model.buffers()):
            add(t)
        for pk in rt._packed.values():
            add(pk["wf"])
            add(pk["wd"])
        for _conv, img in rt._s2d.values():
            add(img)
        self.base = sorted(iv)
        self.size = [iv[b] for b in self.base]
        for (b, n), b2 in zip(zip(self.base, self.size), self.base[1:]):
            assert b + n <= b2, "owned storages overlap"
        self.rank = {}

    def ref(self, v, must):
        i = bisect.bisect_right(self.base, v) - 1
        if i >= 0 and v < self.base[i] + self.size[i]:
            r = self.rank.setdefault(self.base[i], len(self.rank))
            return f"@{r}:{self.size[i]}+{v - self.base[i]}"
        if must or v >= 2 ** 32:
            raise Escaped(f"{v:#x} lies in no tensor the plan or the runtime owns")
        return str(v)

    def tensor(self, t):
        if t is None:
            return "None"
        if t.numel() == 0:
            return f"empty{tuple(t.shape)}"
        return f"{self.ref(t.data_ptr(), True)}{str(t.dtype)[6:]}{tuple(t.shape)}"


def _value(own, v, ctype=None):
    if v is None:
        return "None"
    if isinstance(v, C.Structure):
        parts = []
        for name, ct in v._fields_:
            try:
                parts.append(f"{name}={_value(own, getattr(v, name), ct)}")
            except Escaped as e:
                raise Escaped(f"{type(v).__name__}.{name}: {e}") from None
        return f"{type(v).__name__}{{{','.join(parts)}}}"
    if isinstance(v, C.Array):
        return "[" + ",".join(_value(own, x) for x in v) + "]"
    if isinstance(v, bool):
        return str(int(v))
    if isinstance(v, int):
        return own.ref(v, ctype is C.c_void_p)
    if isinstance(v, float):
        return repr(v)
    if hasattr(v, "_obj"):                                      # ctypes.byref(struct)
        return _value(own, v._obj)
    raise TypeError(f"cannot canonicalise {type(v).__name__}")


def canon(g, rt, model):
    """{"wprep" / "fwd" / "bwd": [(entry name, canonical text)], "items": {item: canonical text}} of a built plan."""
    import torch
    own = _Owned(g, rt, model)
    out = {}
    tapes = {t: getattr(g, t) for t in TAPES}
    for tname, tape in tapes.items():
        ents = []
        for i, (fn, args, name) in enumerate(tape):
            try:
                ents.append((name, f"{name}({', '.join(_value(own, a) for a in args)})"))
            except Escaped as e:
                raise Escaped(f"{tname}[{i}] {name}: {e}") from None
        out[tname] = ents
    tid = {id(t): n for n, t in tapes.items()}
    items = {
        "side_idx": repr(sorted(g.side_idx)),
        "fwd_side": repr(sorted(g.fwd_side.items())),
        "fwd_join": repr(sorted(g.fwd_join)),
        "grad_writes": repr([(i, list(offs)) for i, offs in g.grad_writes]),
        "meta": "\n".join(f"{t}[{i}] {v!r}" for (t, i), v in sorted(((tid[k[0]], k[1]), v) for k, v in g.meta.items())),
        "layout_total": repr(g.layout.total if g.layout is not None else None),
        "heads": "\n".join(f"out={own.tensor(h['out'])} dout={own.tensor(h['dout'])} preobj={own.tensor(h.get('preobj'))} "
                           f"xobj={own.tensor(h.get('xobj'))} och={h.get('och')} dout_slot={h.get('dout_slot')}" for h in g.heads),
    }
    keep = []
    for k in g.keep:
        if isinstance(k, torch.Tensor):
            keep.append(own.tensor(k))
        elif hasattr(k, "t") and hasattr(k, "g"):
            keep.append(f"Buf{k.k}({k.N},{k.H},{k.W},{k.C}) t={own.tensor(k.t)} g={own.tensor(k.g)}")
        else:
            keep.append(type(k).__name__)
    items["keep"] = "\n".join(keep)
    out["items"] = items
    return out


def build_plan(plan):
    """(g, rt, model) of a plan id `<version>-<mode>-<eval|training|frozen>-<size>` under this process's knobs."""
    import torch
    from ryolov4_amd.engine.runtime import Runtime
    from ryolov4_amd.model.yolo import Yolo
    from ryolov4_amd.synth import CFG
    ver, mode, kind, size = plan.split("-")
    training, frozen = KINDS[kind]
    torch.manual_seed(0)
    m = Yolo(MODES[mode], CFG, mode, ver)
    m.train(training and not frozen)
    m.frozen_bn = frozen
    rt = Runtime(m, torch.device("cpu"))
    g = rt.graph(2, int(size), int(size), training, frozen=frozen)
    return g, rt, m


def _h(text, n=16):
    return hashlib.sha256(text.encode()).hexdigest()[:n]


def _seq(named_texts):
    """{"names", "tags" (TAG digits per text: they locate a difference), "digest" (16 digits of all the texts: the check)}."""
    return {"names": [n for n, _x in named_texts], "tags": [_h(x, TAG) for _n, x in named_texts], "digest": _h("\n".join(x for _n, x in named_texts))}


def digests(plan):
    c = canon(*build_plan(plan))
    return dict({t: _seq(c[t]) for t in TAPES}, items=_seq(list(c["items"].items())))


def dump_text(plan):
    c = canon(*build_plan(plan))
    lines = []
    for t in TAPES:
        lines += [f"{t}[{i}] {x}" for i, (_n, x) in enumerate(c[t])]
    for k, v in c["items"].items():
        lines += [f"== {k}"] + v.split("\n")
    return "\n".join(lines)


def _child(env, args, root=None):
    e = dict(os.environ)
    for k in [k for k in e if k.startswith("RYOLO_") and k != "RYOLO_LIB"]:
        del e[k]
    e.update(env)
    cmd = [sys.executable, os.path.abspath(__file__)] + args + (["--root", root] if root else [])
    return subprocess.check_output(cmd, env=e).decode()


def child_digests(env, plans, root=None):
    """{plan: digests} from a fresh process with exactly the knobs of `env` set."""
    return json.loads(_child(env, ["--answer", ",".join(plans)], root).strip().splitlines()[-1])


_ALPHABET = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789"


def load_table(path=TABLE):
    """{"recorded_from", "plans": {knob setting: {plan: digests}}} with names, tags and digests written out as digests() returns them."""
    with open(path) as f:
        raw = json.load(f)
    lists = [[raw["names"][_ALPHABET.index(ch)] for ch in nl] for nl in raw["name_lists"]]
    pool = [{"names": lists[nl], "tags": [tg[k:k + TAG] for k in range(0, len(tg), TAG)], "digest": dg} for nl, tg, dg in raw["tapes"]]
    plans = {}
    for ek, ps in raw["plans"].items():
        plans[ek] = {}
        for p, (tape_idx, tg, dg) in ps.items():
            plans[ek][p] = dict({t: pool[i] for t, i in zip(TAPES, tape_idx)},
                                items={"names": raw["items"], "tags": [tg[k:k + TAG] for k in range(0, len(tg), TAG)], "digest": dg})
    return {"recorded_from": raw["recorded_from"], "plans": plans}


def _write(path, recorded_from, plans):
    names, lists, pool, pool_idx = [], [], [], {}

    def tape(d):
        key = json.dumps(d)
        if key not in pool_idx:
            names.extend(n for n in dict.fromkeys(d["names"]) if n not in names)
            nl = "".join(_ALPHABET[names.index(n)] for n in d["names"])
            if nl not in lists:
                lists.append(nl)
            pool_idx[key] = len(pool)
            pool.append([lists.index(nl), "".join(d["tags"]), d["digest"]])
        return pool_idx[key]
    items = next(iter(plans[""].values()))["items"]["names"]
    out = {}
    for ek, ps in plans.items():
        assert all(d["items"]["names"] == items for d in ps.values())
        out[ek] = {p: [[tape(d[t]) for t in TAPES], "".join(d["items"]["tags"]), d["items"]["digest"]] for p, d in ps.items()}
    assert len(names) <= len(_ALPHABET)

    def rows(xs, ind):
        return ",\n".join(ind + json.dumps(x, separators=(",", ":")) for x in xs)
    with open(path, "w") as f:
        f.write('{\n "recorded_from": ' + json.dumps(recorded_from) + ',\n "names": ' + json.dumps(names) + ',\n "items": ' + json.dumps(items) +
                ',\n "plans": {\n')
        for n, (ek, ps) in enumerate(out.items()):
            f.write(f"  {json.dumps(ek)}: {{\n" + ",\n".join(f"   {json.dumps(p)}: " + json.dumps(d, separators=(",", ":")) for p, d in ps.items()) +
                    "\n  }" + (",\n" if n + 1 < len(out) else "\n"))
        f.write(' },\n "name_lists": [\n' + rows(lists, "  ") + '\n ],\n "tapes": [\n' + rows(pool, "  ") + "\n ]\n}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recorded-from", help="commit of the checkout under --root")
    ap.add_argument("--root", help="checkout whose planner is recorded / dumped (default: the one this script lies in)")
    ap.add_argument("--force", action="store_true", help="overwrite an existing table")
    ap.add_argument("--answer", help="(child) print {plan: digests} of the comma-separated plans as one JSON line")
    ap.add_argument("--dump", metavar="PLAN", help="print the full canonical text of a plan")
    ap.add_argument("--env", action="append", default=[], metavar="KNOB=VALUE", help="with --dump: knob setting (a fresh process is started)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root) if a.root else ROOT)
    if a.answer is not None:
        print(json.dumps({p: digests(p) for p in a.answer.split(",")}))
        return
    if a.dump:
        if a.env:
            sys.stdout.write(_child(dict(e.split("=", 1) for e in a.env), ["--dump", a.dump], a.root))
        else:
            print(dump_text(a.dump))
        return
    if os.path.exists(TABLE) and not a.force:
        sys.exit(f"{TABLE} exists: it records the parent commit's plans and is not regenerated from the code under test (--force to overwrite)")
    if not a.recorded_from:
        sys.exit("--recorded-from <commit> is required")
    plans = {"": child_digests({}, DEFAULT_PLANS, a.root)}
    for env in VARIANTS:
        plans[env_key(env)] = child_digests(env, KNOB_PLANS, a.root)
        base = {p: plans[""][p] for p in KNOB_PLANS}
        assert plans[env_key(env)] != base, f"knob setting {env} changes no recorded plan"
    assert child_digests({}, DEFAULT_PLANS[:3], a.root) == {p: plans[""][p] for p in DEFAULT_PLANS[:3]}, "a fresh process plans differently"
    _write(TABLE, a.recorded_from, plans)
    assert load_table(TABLE)["plans"] == json.loads(json.dumps(plans)), "the written table does not read back"
    n = sum(len(d[t]["names"]) for ps in plans.values() for d in ps.values() for t in TAPES)
    print(f"wrote {TABLE}: {sum(len(ps) for ps in plans.values())} plans, {n} tape entries, {os.path.getsize(TABLE)} bytes")


if __name__ == "__main__":
    main()
