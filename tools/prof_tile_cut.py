"""Per-launch time of the window-cut kernel of full-scene detection (ryolo_tile_cut_views) on the same windows with view id, with the other
non-transposing views (hflip, vflip, rot180) and with the transposing ones (transpose, rot90, rot270, antitranspose).

  python tools/prof_tile_cut.py                     launches only: run it under `rocprofv3 --kernel-trace --stats --output-format csv`
  python tools/prof_tile_cut.py --table TRACE.csv   reads that run's *_kernel_trace.csv and prints the table + one JSON line

A 4000 x 4000 scene, S = 1024, overlap 200: 25 windows in groups of 8 (three full groups and one window).  Three phases, REPS times
each, in this order: all id; cycling hflip / vflip / rot180; cycling the four transposing views.  All move the same bytes (3 B read,
12 B written per pixel).

The yardstick in the table is not measured here: it is the recorded "tile_cut" row of profiles/tiled_views_cut_per_launch.txt, the
retired view-less cut kernel on the same scene and sizes (20.24 / 20.52 / 29.32 us min / median / max over 60 launches of full groups).
It holds for the default sizes only.  Environment: SCENE, S, OVERLAP, B, REPS (20)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SC, S, OV, B = int(os.environ.get("SCENE", 4000)), int(os.environ.get("S", 1024)), int(os.environ.get("OVERLAP", 200)), int(os.environ.get("B", 8))
REPS = int(os.environ.get("REPS", 20))
PHASES = (("views id", (0,)), ("views hflip/vflip/rot180", (1, 2, 3)), ("views transposing", (4, 5, 6, 7)))
RECORDED = {"launches": 60, "min": 20.24, "median": 20.52, "max": 29.32}      # "tile_cut" in profiles/tiled_views_cut_per_launch.txt


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
        rows = [[0, SC, SC, x0, y0, codes[k % len(codes)]] for k, (_, x0, y0) in enumerate(wins)]
        table = torch.tensor(rows, dtype=torch.int64, device=dev)
        for _ in range(REPS):
            for w0 in range(0, len(wins), B):
                hip.call("ryolo_tile_cut_views", hip.ptr(scene), hip.ptr(table), w0, min(B, len(wins) - w0), S, hip.ptr(dst), hip.stream())
        torch.cuda.synchronize()
    print(json.dumps({"windows": len(wins), "groups": -(-len(wins) // B), "reps": REPS}))


def table(path):
    import csv
    rows = [r for r in csv.DictReader(open(path)) if "tile_cut_views" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = len(rows) // len(PHASES)                              # launches per phase
    assert per and len(rows) == len(PHASES) * per, len(rows)
    from ryolov4_amd.lib.tiled import tile_plan
    n = len(tile_plan(SC, SC, S, OV))
    groups = -(-n // B)
    full = [g for g in range(groups) if min(B, n - g * B) == B]
    out = {"scene": SC, "S": S, "batch": B, "windows": n, "launches_per_phase": per, "unit": "us per launch of a full group"}
    print(f"{'phase':28s} {'launches':>8s} {'min':>8s} {'median':>8s} {'max':>8s} {'median / recorded median':>26s}")
    base = RECORDED["median"]
    out["recorded tile_cut"] = dict(RECORDED, ratio=1.0)
    print(f"{'recorded tile_cut':28s} {RECORDED['launches']:8d} {RECORDED['min']:8.2f} {base:8.2f} {RECORDED['max']:8.2f} {1.0:26.3f}")
    for k, (name, _) in enumerate(PHASES):
        rs = rows[k * per:(k + 1) * per]
        us = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for i, r in enumerate(rs) if i % groups in full)
        med = us[len(us) // 2]
        out[name] = {"launches": len(us), "min": round(us[0], 2), "median": round(med, 2), "max": round(us[-1], 2), "ratio": round(med / base, 3)}
        print(f"{name:28s} {len(us):8d} {us[0]:8.2f} {med:8.2f} {us[-1]:8.2f} {med / base:26.3f}")
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--table":
        table(sys.argv[2])
    else:
        launches()
