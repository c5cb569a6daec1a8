"""Cost of the cluster fusion of the full-scene merge where it is largest: ScenePlan.merge on candidates written straight into the plan's
buffers, nc = 16 classes with KC selected candidates each, fuse None against "box" and "wbf".  Prints one JSON line per case:

  disjoint   no two boxes overlap: every candidate is kept (nkeep = n), every cluster has one member.  ryolo_tile_fuse launches a wave
             per kept box and each scans the owner row behind it: nkeep * n / 2 dwords per class, the most the kernel can read.
  pairs      every box comes twice (second copy shifted by a pixel, lower score): nkeep = n / 2, every cluster has two members.
  packed     64 copies of every box: nkeep = n / 64, clusters of 64 (the serial part of a wave, the sums in bit order, at its longest
             per ballot).

merge_ms is the whole merge (both top-k, gather, NMS, mark or owner + fuse, emit) by device events over N calls; added_ms = the mode's
merge_ms minus fuse None's on the same candidates.  Under `rocprofv3 --kernel-trace --stats` the kernels' own times separate.
Environment: KC (comma list, "5000,16384"), NC (16), N (20)."""
import json
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ryolov4_amd.lib import tiled

dev = torch.device("cuda:0")
KCS = [int(k) for k in os.environ.get("KC", "5000,16384").split(",")]
NC, N = int(os.environ.get("NC", 16)), int(os.environ.get("N", 20))
CASES = (("disjoint", 1), ("pairs", 2), ("packed", 64))


def fill(p, kc, copies):
    """kc candidates per class at slots c * kc + i: site i // copies on a 64 px grid (20 x 40 boxes: sites never touch), copy i % copies
    shifted by up to a pixel; scores descend with i, so position i of the class row is candidate i."""
    rng = np.random.RandomState(kc + copies)
    i = np.arange(kc)
    site, cp = i // copies, i % copies
    side = int(np.ceil(np.sqrt(site.max() + 1)))
    rows = np.zeros((p.ld, 7), dtype=np.float32)
    key = np.full((p.nc, p.ld), -np.inf, dtype=np.float32)
    for c in range(p.nc):
        r = rows[c * kc:(c + 1) * kc]
        r[:, 0] = (site % side) * 64 + 32 + cp / max(copies, 1)
        r[:, 1] = (site // side) * 64 + 32
        r[:, 2], r[:, 3] = 20, 40
        r[:, 4] = rng.uniform(-1.5, 1.5, site.max() + 1)[site]
        r[:, 5] = 0.99 - 0.9 * i / kc
        r[:, 6] = c
        key[c, c * kc:(c + 1) * kc] = r[:, 5]
    p.cand.copy_(torch.from_numpy(rows))
    p.key.copy_(torch.from_numpy(key))


def merge_ms(p, fuse):
    def once():
        p.fkey.fill_(-float("inf"))                                    # what the collect pass leaves
        return p.merge(0.4, True, fuse)
    for _ in range(3):
        out, num = once()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(N):
        once()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / N, int(num.item()), p.nkeep.cpu().numpy()


for kc in KCS:
    # 4000 x 4000, S = 1024, overlap 200, all eight views: 200 entries in 25 groups of 8; mk sized so that ld holds nc * kc candidates
    mk = -(-NC * kc // 200)
    cfg = SimpleNamespace(device=dev, batch=8, mk=mk, nc=NC, size=1024, overlap=200, rates=(1.0,), max_nms=kc, max_det=min(kc, 5000),
                          views=tiled.VIEWS)
    p = tiled.ScenePlan(cfg, 4000, 4000)
    assert p.Kc == kc and p.ld >= NC * kc
    for name, copies in CASES:
        fill(p, kc, copies)
        base, num, nkeep = merge_ms(p, None)
        assert (nkeep == -(-kc // copies)).all(), (name, nkeep)
        for mode in tiled.FUSE:
            t, num_f, _ = merge_ms(p, mode)
            assert num_f == num
            print(json.dumps({"case": name, "nc": NC, "n_per_class": kc, "nkeep_per_class": int(nkeep[0]), "cluster": copies, "fuse": mode,
                              "merge_ms_unfused": round(base, 3), "merge_ms": round(t, 3), "added_ms": round(t - base, 3)}), flush=True)
