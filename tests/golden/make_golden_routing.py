"""Fixture `routing_table.json`: what the convolution plan entry points of libryolo_hip.so answer for a few thousand parameter blocks —
`ryolo_conv_gemm_plan` (status, kernel word, statistics rows) and `ryolo_conv_wgrad_plan` / `_kernel` / `_grid` (statuses, kernel, split-K,
workspace bytes, workgroups, waves) — under the default knobs and under every knob setting the GPU suite forces (one child process per
setting: the library reads a knob once).  tests/test_routing_table_cpu.py replays the table against the library under test.
The file is compact (load_table() writes the rows out): a row is its index in candidates(), answers stand back to back, and a knob setting
stores only the answers it moves.

The table is a RECORD of the library at the commit named in its "recorded_from" field, taken before the dispatch was rewritten; it is never
regenerated from the code under test (this script refuses to overwrite it without --force).  The plan entry points only read the parameter
block (fake non-null pointers; no GPU is touched, and without a device the persistent 3x3 kernel sizes itself for 256 CUs, the MI355X's own
count), so a table recorded on a CPU-only box holds on the GPU box.

    RYOLO_LIB=<libryolo_hip.so built from the parent commit> python tests/golden/make_golden_routing.py --recorded-from <commit>
"""
import argparse
import json
import os
import random
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
TABLE = os.path.join(ROOT, "tests", "golden", "routing_table.json")

# forward / data-gradient row: [form, B, H, Cin, Cout, k, s, epi, pipe, aux]
PLAIN, DGRAD_S2, DGRAD_S2D, POOL_GRAD, HEAD, NO_ZEROS, RAGGED_CIN = range(7)
# weight-gradient row: [B, H, Cin, Cout, k, s, flags]
WG_NO_ZEROS, WG_X_MISALIGNED, WG_COUT_PAD, WG_RAGGED_CIN = 1, 2, 4, 8

BATCHES = (1, 8, 64)
SIDES = (13, 25, 50, 100, 200, 400, 800)
CINS = (32, 64, 128, 256, 512, 1024, 2048)
COUTS = (18, 24, 32, 40, 64, 72, 128, 256, 396, 512, 1024)
EPIS = (0, 1, 2, 4)
PIPES = (0, 0x001, 0x101, 0x201, 0x301, 0x601, 0x301 | 0x800, 0x201 | 0x2000)

# every knob setting tests/test_gpu_forced_kernels.py and the multi-GPU partition force
VARIANTS = [{"RYOLO_GEMM_256": "2"}, {"RYOLO_GEMM_DEEP": "6"}, {"RYOLO_GEMM_DEEP": "4"}, {"RYOLO_GEMM_N64": "2"}, {"RYOLO_GEMM_T1": "0"},
            {"RYOLO_P3_WS64": "2"}, {"RYOLO_P3_WS64": "0"}, {"RYOLO_GEMM_WS": "2"}, {"RYOLO_GEMM_WS": "0"}, {"RYOLO_S2C32": "0"},
            {"RYOLO_W3_FORCE": "1"}, {"RYOLO_W3_V8": "0"}, {"RYOLO_WGRAD_8W": "0"}, {"RYOLO_WGRAD_8W_MINC": "128"}, {"RYOLO_WGRAD_P1": "3"},
            {"RYOLO_WGRAD_TAPS_DMA": "0"}, {"RYOLO_W3_MINSTEPS": "4"}, {"RYOLO_W3_V8_BLOCKS": "88", "RYOLO_WGRAD_8W_BLOCKS": "88"}]
# settings that only choose among instantiations of one kernel family (no plan entry point reports the difference): recorded all the same
SILENT = ({"RYOLO_GEMM_DEEP": "6"}, {"RYOLO_GEMM_DEEP": "4"}, {"RYOLO_WGRAD_P1": "3"})


def _taps_fwd(k, pad):
    return [(r - pad, c - pad, r * k + c) for r in range(k) for c in range(k)]


def _fill(tc, taps, oh_add=0, ow_add=0):
    tc.ntaps, tc.oh_add, tc.ow_add = len(taps), oh_add, ow_add
    for i, (dh, dw, wi) in enumerate(taps):
        tc.dh[i], tc.dw[i], tc.widx[i] = dh, dw, wi


def gemm_block(row):
    """The ConvGemmParams of a forward row, built the way engine/graph.py builds it (tests/test_routing_cpu.py::_plan for the plain form)."""
    from ryolov4_amd.engine import structs as S
    form, B, H, Cin, Cout, k, s, epi, pipe, aux = row
    p = S.ConvGemmParams()
    pad = (k - 1) // 2
    OH = (H + 2 * pad - k) // s + 1
    p.A, p.NB, p.IH, p.IW, p.Cin, p.ldA = 0x1000, B, H, H, Cin, Cin
    p.W, p.Nout, p.wtaps = 0x2000, Cout, k * k
    p.OH, p.OW, p.sh, p.sw = OH, OH, s, s
    p.oh_mul, p.ow_mul, p.OHf, p.OWf = 1, 1, OH, OH
    p.nclasses = 1
    _fill(p.cls[0], _taps_fwd(k, pad))
    p.epi, p.out, p.ldC, p.zeros, p.pipe = epi, 0x3000, Cout, 0x4000, pipe
    p.scale, p.shift = 0x5000, 0x6000
    if form == DGRAD_S2:            # data gradient of a 3x3 stride-2 layer Cout -> Cin over an H x H input: four output-parity classes on the dY grid
        h = H // 2
        p.IH = p.IW = p.OH = p.OW = h
        p.sh = p.sw = 1
        p.Cin = p.ldA = Cout
        p.Nout, p.ldC, p.wtaps = Cin, Cin, 9
        p.oh_mul, p.ow_mul, p.OHf, p.OWf = 2, 2, 2 * h, 2 * h
        p.nclasses = 4
        for i, (ph, pw) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            taps = [((ph + 1 - r) // 2, (pw + 1 - c) // 2, r * 3 + c) for r in range(3) for c in range(3) if (ph + 1 - r) % 2 == 0 and (pw + 1 - c) % 2 == 0]
            _fill(p.cls[i], taps, ph, pw)
    elif form == DGRAD_S2D:         # the same gradient as ONE space-to-depth GEMM: aux = the layer's input channels, Cin = its output channels
        h = H // 2
        p.IH = p.IW = p.OH = p.OW = h
        p.sh = p.sw = 1
        p.Cin = p.ldA = Cin
        p.Nout, p.ldC, p.wtaps = 4 * aux, aux, 4
        p.oh_mul, p.ow_mul, p.OHf, p.OWf = 2, 2, 2 * h, 2 * h
        p.s2d_cin = aux
        _fill(p.cls[0], [(da, db, 2 * da + db) for da in range(2) for db in range(2)])
    elif form == POOL_GRAD:         # pointwise data gradient whose store adds a MaxPool2d(2, 2) gradient
        p.pool_idx, p.pool_dz, p.pool_ldi, p.pool_ld = 0x7000, 0x8000, Cout, Cout
    elif form == HEAD:              # detection head written in its final layout: aux = attributes per anchor
        p.head_attrs, p.head_och, p.bias = aux, 4, 0x9000
    elif form == NO_ZEROS:
        p.zeros = None
    elif form == RAGGED_CIN:
        p.Cin = p.ldA = Cin + 8
    return p


def wgrad_block(row):
    from ryolov4_amd.engine import structs as S
    B, H, Cin, Cout, k, s, flags = row
    p = S.WgradParams()
    pad = (k - 1) // 2
    OH = (H + 2 * pad - k) // s + 1
    cpad = (Cout + 31) // 32 * 32
    if flags & WG_COUT_PAD and cpad == Cout:
        cpad += 32
    if not flags & WG_COUT_PAD and Cout % 8 == 0:
        cpad = Cout
    p.dY, p.ldY, p.Cout, p.CoutPad = 0x1000, cpad, Cout, cpad
    p.X, p.NB, p.IH, p.IW, p.Cin, p.ldX = 0x2000 + (8 if flags & WG_X_MISALIGNED else 0), B, H, H, Cin + (8 if flags & WG_RAGGED_CIN else 0), Cin + 32
    p.OH, p.OW, p.sh, p.sw = OH, OH, s, s
    taps = _taps_fwd(k, pad)
    p.ntaps = len(taps)
    for i, (dh, dw, _) in enumerate(taps):
        p.dh[i], p.dw[i] = dh, dw
    p.dW, p.partial = 0x3000, 0x4000
    p.zeros = None if flags & WG_NO_ZEROS else 0x5000
    return p


def gemm_answer(row):
    """[status, kernel word, statistics rows] of ryolo_conv_gemm_plan."""
    from ryolov4_amd import hip
    from ryolov4_amd.engine import structs as S
    rows, kern = S.I(-1), S.I(-1)
    rc = hip.lib().ryolo_conv_gemm_plan(gemm_block(row), rows, kern)
    return [rc, kern.value, rows.value]


def wgrad_answer(row):
    """[plan status, splitk, workspace bytes, kernel status, kernel, grid status, workgroups, waves] of the three weight-gradient plan entry points."""
    from ryolov4_amd import hip
    from ryolov4_amd.engine import structs as S
    L = hip.lib()
    p = wgrad_block(row)
    sk, ws, kern, wgs, waves = S.I(-1), S.Z(0), S.I(-1), S.I(-1), S.I(-1)
    rc_plan = L.ryolo_conv_wgrad_plan(p, sk, ws)
    rc_kern = L.ryolo_conv_wgrad_kernel(p, kern)
    rc_grid = L.ryolo_conv_wgrad_grid(p, wgs, waves)
    return [rc_plan, sk.value, ws.value, rc_kern, kern.value, rc_grid, wgs.value, waves.value]


def answers(table, fwd_idx=None, wg_idx=None):
    fwd = table["fwd"] if fwd_idx is None else [table["fwd"][i] for i in fwd_idx]
    wg = table["wg"] if wg_idx is None else [table["wg"][i] for i in wg_idx]
    return {"fwd": [gemm_answer(r) for r in fwd], "wg": [wgrad_answer(r) for r in wg]}


def load_table(path=TABLE):
    """The table with its rows written out.  The file names a row by its index in candidates() (a fifth of the bytes of the row itself; the
    digest of the candidate lists is recorded, so an edit of the enumeration cannot silently re-label the rows) and stores, per knob setting, only
    the answers the setting moves: every other row of its subset (the shared probe rows) must answer as under the default knobs."""
    with open(path) as f:
        raw = json.load(f)
    cand = candidates()
    assert raw["candidates_sha1"] == _digest(cand), "the candidate enumeration changed since the table was recorded"
    t = {"recorded_from": raw["recorded_from"], "variants": []}
    for key in ("fwd", "wg"):
        t[key] = [cand[key][i] for i in raw[key + "_rows"]]
        flat, n = raw[key + "_out"], len(raw[key + "_answer"])          # answers back to back, len(<key>_answer) numbers per row
        t[key + "_out"] = [flat[i:i + n] for i in range(0, len(flat), n)]
    for v in raw["variants"]:
        e = {"env": v["env"]}
        for key in ("fwd", "wg"):
            moved = {m[0]: m[1:] for m in v[key + "_moved"]}
            e[key + "_idx"] = sorted(set(raw[key + "_probe"]) | set(moved))
            e[key] = [moved.get(i, t[key + "_out"][i]) for i in e[key + "_idx"]]
        t["variants"].append(e)
    return t


def child_answers(env, table_path, variant):
    """The answers of knob variant `variant` from a fresh process (a knob is read once per process)."""
    e = dict(os.environ)
    for k in [k for k in e if k.startswith("RYOLO_") and k != "RYOLO_LIB"]:
        del e[k]
    e.update(env)
    out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--answer", str(variant), "--table", table_path], env=e)
    return json.loads(out.decode().strip().splitlines()[-1])


def _forward_candidates():
    rows = []
    for B in BATCHES:
        for H in SIDES:
            for Cin in CINS:
                for Cout in COUTS:
                    for k in (1, 3):
                        for s in (1, 2):
                            for epi in EPIS:
                                for pipe in PIPES:
                                    rows.append([PLAIN, B, H, Cin, Cout, k, s, epi, pipe, 0])
    special = []
    for B in BATCHES:
        for H in (26, 50, 100, 200, 400, 800):
            for pipe in PIPES:
                for epi in (0, 4):
                    for Cin in (32, 64, 128, 256):
                        for Cout in (64, 128, 256, 512):
                            special.append([DGRAD_S2, B, H, Cin, Cout, 3, 2, epi, pipe, 0])
                    for cin in (32, 16):
                        for dyc in (32, 64, 128):
                            special.append([DGRAD_S2D, B, H, dyc, 4 * cin, 3, 2, epi, pipe, cin])
                for epi in EPIS:
                    for Cin in (64, 128, 256, 512):
                        for Cout in (64, 128, 256):
                            special.append([POOL_GRAD, B, H, Cin, Cout, 1, 1, epi, pipe, 0])
                for Cin in (128, 256, 512, 1024):
                    for attrs, Cout in ((22, 396), (22, 66), (185 + 16, 603), (5, 396), (22, 400), (7, 126)):
                        for epi in (3, 0):
                            special.append([HEAD, B, H, Cin, Cout, 1, 1, epi, pipe, attrs])
                    special.append([HEAD, B, H, Cin, 396, 3, 1, 3, pipe, 22])          # a head that is not a 1x1 GEMM
            for Cin, Cout, k, s in ((64, 64, 3, 1), (128, 128, 3, 1), (32, 64, 3, 2), (256, 256, 1, 1), (512, 512, 1, 1), (1024, 256, 1, 1)):
                for epi in EPIS:
                    for pipe in PIPES:
                        special.append([NO_ZEROS, B, H, Cin, Cout, k, s, epi, pipe, 0])
                        special.append([RAGGED_CIN, B, H, Cin, Cout, k, s, epi, pipe, 0])
    # the hand-picked routes of tests/test_routing_cpu.py always belong to the table
    anchors = []
    for epi in EPIS:
        for B, H, Cin, Cout in ((8, 25, 256, 256), (8, 25, 1024, 512), (8, 50, 128, 128), (8, 100, 128, 128), (1, 25, 256, 256), (64, 25, 256, 256),
                                (64, 50, 128, 128), (64, 400, 64, 64), (8, 200, 64, 64), (8, 100, 64, 64)):
            anchors.append([PLAIN, B, H, Cin, Cout, 3, 1, epi, 0x201, 0])
        for B, H, Cin, Cout in ((64, 100, 512, 512), (64, 25, 2048, 512), (64, 100, 512, 128), (64, 200, 256, 256), (8, 25, 1024, 1024)):
            anchors.append([PLAIN, B, H, Cin, Cout, 1, 1, epi, 0x201, 0])
    anchors += [[PLAIN, 64, 800, 32, 64, 3, 2, 1, 0x201, 0], [PLAIN, 64, 400, 64, 128, 3, 2, 1, 0x201, 0], [PLAIN, 8, 50, 256, 256, 3, 2, 1, 0x201, 0],
                [PLAIN, 64, 25, 256, 256, 3, 1, 1, 0x201 | 0x2000, 0], [PLAIN, 8, 25, 256, 256, 3, 1, 1, 0x201 | 0x400, 0], [PLAIN, 8, 25, 256, 256, 3, 1, 1, 0x001, 0]]
    return rows, special, anchors


def candidates():
    cross, special, anchors = _forward_candidates()
    return {"fwd": cross + special + anchors, "wg": _wgrad_candidates()}


def _digest(cand):
    import hashlib
    return hashlib.sha1(json.dumps([cand["fwd"], cand["wg"]]).encode()).hexdigest()


def _wgrad_candidates():
    rows = []
    for B in BATCHES:
        for H in SIDES:
            for Cin in CINS:
                for Cout in COUTS:
                    for k in (1, 3):
                        for s in (1, 2):
                            rows.append([B, H, Cin, Cout, k, s, 0])
                            for f in (WG_NO_ZEROS, WG_X_MISALIGNED, WG_COUT_PAD, WG_RAGGED_CIN):
                                rows.append([B, H, Cin, Cout, k, s, f])
    return rows


def _thin(rng, rows, ans, per_answer, extra, key):
    """Deterministic thinning, stratified by the recorded answer: up to `per_answer` rows of every distinct key(answer), then `extra` rows drawn
    uniformly from the rest."""
    groups = {}
    for i, a in enumerate(ans):
        groups.setdefault(key(a), []).append(i)
    keep = set()
    for k in sorted(groups):
        g = groups[k]
        keep.update(rng.sample(g, min(per_answer, len(g))))
    rest = [i for i in range(len(rows)) if i not in keep]
    keep.update(rng.sample(rest, min(extra, len(rest))))
    return sorted(keep)


def _check_coverage(table, ans, variants):
    fwd_ok = [a for a in ans["fwd"] if a[0] == 0]
    fams = {a[1] & 0xff for a in fwd_ok}
    assert fams == set(range(7)), f"forward families reached: {sorted(fams)}"
    tiles = {(((a[1] >> 12) & 15) * 64, ((a[1] >> 16) & 15) * 32, bool(a[1] & 0x100)) for a in fwd_ok if a[1] & 0xff == 0}
    for t in ((256, 32), (256, 64), (128, 64), (128, 128)):
        for t1 in (False, True):
            assert t + (t1,) in tiles, f"generic tile {t} t1={t1} not in the table ({sorted(tiles)})"
    heads = [r for r, a in zip(table["fwd"], ans["fwd"]) if r[0] == HEAD and a[0] == 0]
    assert heads and all(a[1] == (0x100 | (2 << 12) | (4 << 16)) for r, a in zip(table["fwd"], ans["fwd"]) if r[0] == HEAD and a[0] == 0), "fused head word"
    assert {(a[1] & 0xff, ((a[1] >> 16) & 15) * 32) for a in fwd_ok} >= {(1, 64), (1, 128), (4, 256)}, "patch / gemm256 tiles"
    assert {a[0] for a in ans["fwd"]} == {0, 1, 4}, "forward statuses"
    wg_ok = [a for a in ans["wg"] if a[0] == 0 and a[5] == 0]
    assert {(a[4], a[7]) for a in wg_ok} >= {(0, 4), (1, 4), (1, 8), (2, 4), (3, 8)}, "weight-gradient kernels / waves"
    assert {a[0] for a in ans["wg"]} == {0, 1} and {a[5] for a in ans["wg"]} == {0, 1}, "weight-gradient statuses"
    assert any(a[0] == 1 and a[3] == 0 for a in ans["wg"]), "ryolo_conv_wgrad_kernel answers RY_OK for blocks the plan rejects"
    for v in variants:                      # every knob setting must move at least one recorded answer, or its rows pin nothing
        base_f = [ans["fwd"][i] for i in v["fwd_idx"]]
        base_w = [ans["wg"][i] for i in v["wg_idx"]]
        moved = base_f != v["fwd"] or base_w != v["wg"]
        assert moved or v["env"] in SILENT, f"knob variant {v['env']} changes no recorded answer"
    # a variant on GEMM_256=2 must reach the 256 x 128 gemm256 tile, W3_V8=0 the 4-wave ring kernel on Cin % 64 == 0 layers
    v256 = next(v for v in variants if v["env"] == {"RYOLO_GEMM_256": "2"})
    assert any(a[0] == 0 and a[1] & 0xff == 4 and (a[1] >> 16) & 15 == 4 for a in v256["fwd"]), "256 x 128 gemm256 tile under RYOLO_GEMM_256=2"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recorded-from", help="commit the library under RYOLO_LIB was built from")
    ap.add_argument("--force", action="store_true", help="overwrite an existing table")
    ap.add_argument("--answer", type=int, help="(child) print the answers of knob variant N of --table as one JSON line; -1: all rows, default knobs")
    ap.add_argument("--table", default=TABLE)
    a = ap.parse_args()
    if a.answer is not None:
        table = load_table(a.table)
        v = table["variants"][a.answer] if a.answer >= 0 else {}
        print(json.dumps(answers(table, v.get("fwd_idx"), v.get("wg_idx"))))
        return
    if os.path.exists(TABLE) and not a.force:
        sys.exit(f"{TABLE} exists: it records the parent commit's routing and is not regenerated from the code under test (--force to overwrite)")
    if not a.recorded_from:
        sys.exit("--recorded-from <commit> is required")
    if any(k.startswith("RYOLO_") and k != "RYOLO_LIB" for k in os.environ):
        sys.exit("unset the RYOLO_* knobs: the main table records the defaults")
    rng = random.Random(20260)
    cross, special, anchors = _forward_candidates()
    cand = candidates()
    n_cross, n_special = len(cross), len(special)
    fwd_rows = _thin(rng, cross, [gemm_answer(r) for r in cross], 40, 920, lambda x: (x[0], x[1])) + \
        [n_cross + i for i in _thin(rng, special, [gemm_answer(r) for r in special], 25, 250, lambda x: (x[0], x[1]))] + \
        [n_cross + n_special + i for i in range(len(anchors))]
    wg_rows = _thin(rng, cand["wg"], [wgrad_answer(r) for r in cand["wg"]], 60, 330, lambda x: (x[0], x[3], x[4], x[5], x[7]))
    raw = {"recorded_from": a.recorded_from, "candidates_sha1": _digest(cand),
           "fwd_answer": ["status", "kernel", "stats_rows"],
           "wg_answer": ["plan_status", "splitk", "workspace_bytes", "kernel_status", "kernel", "grid_status", "workgroups", "waves"],
           "fwd_rows": fwd_rows, "wg_rows": wg_rows}
    ans = answers({"fwd": [cand["fwd"][i] for i in fwd_rows], "wg": [cand["wg"][i] for i in wg_rows]})
    raw["fwd_out"], raw["wg_out"] = [x for a_ in ans["fwd"] for x in a_], [x for a_ in ans["wg"] for x in a_]
    # every knob setting is replayed on the same probe rows plus (up to 40 / 30 of) the rows whose answer it moves: a few hundred rows each
    raw["fwd_probe"] = sorted(rng.sample(range(len(fwd_rows)), 250))
    raw["wg_probe"] = sorted(rng.sample(range(len(wg_rows)), 150))
    raw["variants"] = []
    tmp = TABLE + ".tmp"

    def dump(path):
        with open(path, "w") as f:
            f.write("{\n")
            for n, k in enumerate(raw):
                f.write(f' "{k}": ' + json.dumps(raw[k], separators=(",", ":")) + (",\n" if n + 1 < len(raw) else "\n"))
            f.write("}\n")
    dump(tmp)
    try:
        assert child_answers({}, tmp, -1) == ans, "a fresh process answers differently from this one"
        for env in VARIANTS:
            got = child_answers(env, tmp, -1)
            v = {"env": env}
            for key, n_moved in (("fwd", 40), ("wg", 30)):
                moved = [i for i, (x, y) in enumerate(zip(ans[key], got[key])) if x != y]
                probe = set(raw[key + "_probe"])
                keep = [i for i in moved if i in probe]                 # a moved probe row must carry its answer
                rest = [i for i in moved if i not in probe]
                keep += rng.sample(rest, min(n_moved, len(rest)))
                v[key + "_moved"] = [[i] + got[key][i] for i in sorted(keep)]
            raw["variants"].append(v)
    finally:
        os.remove(tmp)
    dump(tmp)
    try:
        table = load_table(tmp)
    finally:
        os.remove(tmp)
    _check_coverage(table, ans, table["variants"])
    dump(TABLE)
    print(f"wrote {TABLE}: {len(fwd_rows)} forward rows, {len(wg_rows)} weight-gradient rows, {len(VARIANTS)} knob variants, {os.path.getsize(TABLE)} bytes")


if __name__ == "__main__":
    main()
