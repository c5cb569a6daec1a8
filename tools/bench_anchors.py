"""Fitting anchors on the device: what it costs.  Writes one JSON document (default profiles/anchor_fit_bench.json) and prints it.

n = 1 000 000 SYNTHETIC label sizes (tests/anchor_ref.lognormal_sizes: w = exp(N(3, 0.8)), h = w * exp(|N(0.6, 0.5)|), PCG64 seed 7), K = 9,
G = 1000 generations of C = 8 children, reference anchors as the start:
  evolve   wall clock of ryolo_anchor_evolve (host clock around enqueue + synchronize, best and worst of REPS runs), ms per generation, and the
           per-generation pass over the labels in GB/s of label bytes (8 bytes per label per generation: the pass is compute bound — 4 divisions
           per label, anchor and child — so this is a rate, not a bandwidth claim);
  kmeans   the 30 Lloyd iterations from the quantile start, sort included;
  split    ms per generation at n / 4, n / 2 and n labels and the line through them: a fixed part per generation (two launches and the
           single-workgroup deciding kernel over 1024 partial records) and a part per label (the scoring pass);
  host     the vectorised float32 numpy restatement (tests/anchor_ref.evolve) on the SAME sizes, cut down to HOST_G generations (stated in the
           output), ms per generation;
  table    drawing the [G, C, K, 2] mutation table on the host, and its upload.
Also the fitness / bpr / lost labels of the reference anchors on these sizes and of the fitted ones.  The sizes are synthetic: the numbers say
nothing about DOTA, and which anchors train the better detector there is not measured.  Nothing here is compared with an earlier commit: no
existing launch changes.  Environment: REPS (3), HOST_G (2), N (1 000 000), G (1000), C (8)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ryolov4_amd.lib import anchors as An
from tests import anchor_ref as R

dev = torch.device("cuda:0")
REPS, HOST_G = int(os.environ.get("REPS", 3)), int(os.environ.get("HOST_G", 2))
N, G, C, K = int(os.environ.get("N", 1000000)), int(os.environ.get("G", 1000)), int(os.environ.get("C", 8)), 9
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "anchor_fit_bench.json")


def wall(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


wh_host = R.lognormal_sizes(N, seed=7)
wh = torch.from_numpy(wh_host).to(dev)
t0 = time.perf_counter()
v_host = An.mutation_table(3, G, C, K)
t_table = (time.perf_counter() - t0) * 1e3
t0 = time.perf_counter()
v = torch.from_numpy(v_host).to(dev)
torch.cuda.synchronize()
t_upload = (time.perf_counter() - t0) * 1e3
k0 = torch.from_numpy(R.REF_ANCHORS).to(dev)

res_holder = {}


def run_evolve():
    res_holder["evolve"] = An.evolve_device(wh, k0, v)


def run_kmeans():
    res_holder["kmeans"] = An.kmeans_device(wh, K, 30)


t_evo = wall(run_evolve)
t_km = wall(run_kmeans)
k1, st = res_holder["evolve"]
fitted = An._stats(st.cpu(), N)
ref = An.anchor_fitness(wh, k0)
km = An.anchor_fitness(wh, res_holder["kmeans"])
k1b, stb = An.evolve_device(wh, k0, v)
same = bool(torch.equal(k1, k1b) and torch.equal(st, stb))

t0 = time.perf_counter()
kh, (fh, rh, ph), acch = R.evolve(wh_host, R.REF_ANCHORS, v_host[:HOST_G])
t_host = (time.perf_counter() - t0) * 1e3
kd, std = An.evolve_device(wh, k0, v[:HOST_G])
host_equal = bool(kd.cpu().numpy().tobytes() == kh.tobytes())

# where a generation's time goes: the same run at n / 4 and n / 2 labels (grids of 1024 workgroups at all three sizes, so the deciding launch sums
# the same 1024 partials); the line through the three points splits a generation into a part per label (the scoring pass) and a fixed part
# (two launches and the deciding kernel)
split = {}
if N >= 4 * 262144:
    pts = []
    for m in (N // 4, N // 2, N):
        sub = wh[:m].contiguous()
        pts.append((m, min(wall(lambda: An.evolve_device(sub, k0, v))) / max(G, 1)))
    xs, ys = np.array([p[0] for p in pts], dtype=np.float64), np.array([p[1] for p in pts])
    slope, fixed = np.polyfit(xs, ys, 1)
    split = {"labels": [p[0] for p in pts], "ms_per_generation": [round(p[1], 4) for p in pts], "fixed_ms_per_generation": round(float(fixed), 4),
             "ns_per_label_per_generation": round(float(slope) * 1e6, 4)}

ms_gen = min(t_evo) / max(G, 1)
res = {
    "device": torch.cuda.get_device_name(0), "synthetic_sizes": True, "n": N, "K": K, "G": G, "C": C, "reps": REPS,
    "evolve_wall_ms": [round(t, 2) for t in sorted(t_evo)], "evolve_ms_per_generation": round(ms_gen, 4),
    "evolve_label_GBps": round(N * 8 / (ms_gen * 1e-3) / 1e9, 1), "evolve_runs_bitwise_equal": same,
    "generation_time_split": split,
    "kmeans30_wall_ms": [round(t, 2) for t in sorted(t_km)],
    "table_draw_host_ms": round(t_table, 1), "table_upload_ms": round(t_upload, 2),
    "host_numpy_generations": HOST_G, "host_numpy_wall_ms": round(t_host, 1),
    "host_numpy_ms_per_generation": round(t_host * C / (1 + C * HOST_G), 1),  # (the wall clock covers 1 + C * HOST_G scored sets, a generation C)
    "host_and_device_anchors_equal_after_those_generations": host_equal,
    "reference_anchors": {"fitness": ref["fitness"], "bpr": ref["bpr"], "aat": ref["aat"], "lost": N - ref["reached"]},
    "kmeans_start": {"fitness": km["fitness"], "bpr": km["bpr"], "aat": km["aat"], "lost": N - km["reached"]},
    "evolved_from_reference": {"fitness": fitted["fitness"], "bpr": fitted["bpr"], "aat": fitted["aat"], "lost": N - fitted["reached"],
                               "accepted": fitted["accepted"], "anchors": [[round(float(x), 3) for x in a] for a in An._by_area(k1.cpu().numpy())]},
    "note": "synthetic log-normal sizes; says nothing about DOTA; the effect of fitted anchors on detector quality is not measured",
}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
