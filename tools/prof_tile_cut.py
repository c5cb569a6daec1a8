"""Per-launch time of the window-cut kernels of full-scene detection on the same windows: ryolo_tile_cut against ryolo_tile_cut_views
with the non-transposing views (id, hflip, vflip, rot180) and with the transposing ones (transpose, rot90, rot270, antitranspose).

  python tools/prof_tile_cut.py                     launches only: run it under `rocprofv3 --kernel-trace --stats --output-format csv`
  python tools/prof_tile_cut.py --table TRACE.csv   reads that run's *_kernel_trace.csv and prints the table + one JSON line

A 4000 x 4000 scene, S = 1024, overlap 200: 25 windows in groups of 8 (three full groups and one window).  Phases, REPS times each, in
this order: (a) ryolo_tile_cut, (b) cut_views all id, (c) cut_views cycling hflip / vflip / rot180, (d) cut_views cycling the four
transposing views.  All move the same bytes (3 B read, 12 B written per pixel); the yardstick for (b)-(d) is (a)'s own min-max over its
launches of full groups.  Environment: SCENE, S, OVERLAP, B, REPS (20)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SC, S, OV, B = int(os.environ.get("SCENE", 4000)), int(os.environ.get("S", 1024)), int(os.environ.get("OVERLAP", 200)), int(os.environ.get("B", 8))
REPS = int(os.environ.get("REPS", 20))
PHASES = (("tile_cut", None), ("views id", (0,)), ("views hflip/vflip/rot180", (1, 2, 3)), ("views transposing", (4, 5, 6, 7)))


def launches():
    import numpy as np
    import torch
    from ryolov4_amd import hip
    from ryolov4_amd.lib.tiled import tile_plan
    dev = torch.device("cuda:0")
    scene = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (SC, SC, 3)).astype(np.uint8)).to(dev)
    wins = tile_plan(SC, SC, S, OV)
    dst = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
    for name, codes in PHASES:
        rows = [[0, SC, SC, x0, y0] + ([] if codes is None else [codes[k % len(codes)]]) for k, (_, x0, y0) in enumerate(wins)]
        table = torch.tensor(rows, dtype=torch.int64, device=dev)
        fn = "ryolo_tile_cut" if codes is None else "ryolo_tile_cut_views"
        for _ in range(REPS):
            for w0 in range(0, len(wins), B):
                hip.call(fn, hip.ptr(scene), hip.ptr(table), w0, min(B, len(wins) - w0), S, hip.ptr(dst), hip.stream())
        torch.cuda.synchronize()
    print(json.dumps({"windows": len(wins), "groups": -(-len(wins) // B), "reps": REPS}))


def table(path):
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "tile_cut" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    old = [r for r in rows if "tile_cut_views" not in r["Kernel_Name"]]
    new = [r for r in rows if "tile_cut_views" in r["Kernel_Name"]]
    per = len(old)                                              # launches per phase
    assert per and len(new) == 3 * per, (len(old), len(new))
    from ryolov4_amd.lib.tiled import tile_plan
    n = len(tile_plan(SC, SC, S, OV))
    groups = -(-n // B)
    full = [g for g in range(groups) if min(B, n - g * B) == B]
    out = {"scene": SC, "S": S, "batch": B, "windows": n, "launches_per_phase": per, "unit": "us per launch of a full group"}
    print(f"{'phase':28s} {'launches':>8s} {'min':>8s} {'median':>8s} {'max':>8s} {'median / tile_cut median':>26s}")
    base = None
    for k, (name, _) in enumerate(PHASES):
        rs = old if k == 0 else new[(k - 1) * per:k * per]
        us = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for i, r in enumerate(rs) if i % groups in full)
        med = us[len(us) // 2]
        base = base or med
        out[name] = {"launches": len(us), "min": round(us[0], 2), "median": round(med, 2), "max": round(us[-1], 2), "ratio": round(med / base, 3)}
        print(f"{name:28s} {len(us):8d} {us[0]:8.2f} {med:8.2f} {us[-1]:8.2f} {med / base:26.3f}")
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--table":
        table(sys.argv[2])
    else:
        launches()
