"""Time of the fused loss alone — one `criterion(outs, targets, sync_items=False)` + `backward()` — at the benchmark shape (batch 64,
800x800, nc 16, synth_batch targets, random head maps) for the losses that share the kfiou head layout.  Device events around `--iters`
calls after `--warmup`, the whole round repeated `--runs` times with the losses alternating, so that the spread of one loss across the
runs can be read next to the differences between losses.  Prints one JSON line.

    python tools/bench_loss.py [--losses kfiou,kld,gwd,probiou] [--batch 64] [--size 800] [--iters 50] [--warmup 10] [--runs 2]
                               [--ignore-rows 0,2048]

--ignore-rows: every loss is also timed with that many ignore rows per batch (`criterion(..., ignore=table)`; 0 = the plain call): random
rotated boxes of 16 .. 128 pixels spread over the images, so the marking kernel walks bounding boxes of the size real labels have.  A
case with rows is reported as "<loss>+<n>rows".

RYOLO_LIB=<another build of libryolo_hip.so> times that build instead (A/B against another commit with the SAME struct layouts; a commit
from before a parameter block grew is timed from its own checkout with this tool's version there)."""
import argparse
import json
import os
import math
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ryolov4_amd import hip
from ryolov4_amd.lib.loss import make_loss
from ryolov4_amd.synth import CFG, HYP, synth_batch


class _Model:
    pass


def ignore_table(n, batch, size, dev, seed=7):
    """n ignore rows [n, 9] = (image, four vertices normalised): rotated boxes with sides of 16 .. 128 pixels, centres anywhere."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n, 6, generator=g)
    img = torch.floor(u[:, 0] * batch)
    cx, cy = u[:, 1] * size, u[:, 2] * size
    w, h = 16.0 * 8.0 ** u[:, 3], 16.0 * 8.0 ** u[:, 4]
    th = (u[:, 5] - 0.5) * math.pi
    c, s_ = torch.cos(th), torch.sin(th)
    out = [img]
    for sx, sy in ((-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)):
        out += [(cx + sx * w * c - sy * h * s_) / size, (cy + sx * w * s_ + sy * h * c) / size]
    return torch.stack(out, 1).float().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--losses", default="kfiou,kld,gwd,probiou")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--nc", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--ignore-rows", default="0")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss: needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    from oracle import ref_ops
    m = _Model()
    m.anchors, m.nc = ref_ops.make_anchors(CFG, "kfiou"), args.nc
    _, tg = synth_batch(args.batch, args.size, args.nc, False, seed=42)
    tg = tg.to(dev)
    g = torch.Generator(device=dev).manual_seed(9)
    outs = [torch.randn(args.batch, 18, args.size // s, args.size // s, args.nc + 6, generator=g, device=dev).requires_grad_() for s in (8, 16, 32)]
    rows = [int(v) for v in args.ignore_rows.split(",")]
    names, crits, tables = [], {}, {}
    for n in args.losses.split(","):
        for r in rows:
            key = n if r == 0 else "{}+{}rows".format(n, r)
            names.append(key)
            crits[key], tables[key] = make_loss(n, m, HYP), (ignore_table(r, args.batch, args.size, dev) if r else None)

    def call(crit, ig):
        loss, _ = crit(outs, tg, sync_items=False) if ig is None else crit(outs, tg, ignore=ig, sync_items=False)
        loss.backward()
        for o in outs:
            o.grad = None

    ms = {n: [] for n in names}
    for _ in range(args.runs):
        for n in names:
            for _ in range(args.warmup):
                call(crits[n], tables[n])
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                call(crits[n], tables[n])
            t1.record()
            torch.cuda.synchronize()
            ms[n].append(round(t0.elapsed_time(t1) / args.iters, 4))
            crits[n].flush()
    ignored = {n: [int(v) for v in crits[n].ignored_cells.tolist()] for n in names if tables[n] is not None}
    print(json.dumps({"what": "fused loss forward + backward, ms per call (device events)", "lib": os.path.basename(os.path.dirname(hip.LIB_PATH)) + "/" + os.path.basename(hip.LIB_PATH),
                      "batch": args.batch, "size": args.size, "nc": args.nc, "targets": int(tg.shape[0]), "iters": args.iters, "warmup": args.warmup,
                      "ms_per_call": ms, "ignored_cells_per_scale": ignored}))


if __name__ == "__main__":
    main()
