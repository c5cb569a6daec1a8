"""What copy-paste (datasets/copy_paste.py, csrc/copypaste.hip) costs the scene loader, in tools/bench_scene_loader.py's standing configuration:
batch 64 of 800x800, every augmentation on, eight synthetic 4000x4000 scenes of 500 labels, jitter on.

  loader mode   python tools/bench_copy_paste.py loader OUT.json
                ms per batch of SceneDataset with copy_paste=None, nothing else.  It uses no interface newer than the scene loader's, so a copy
                of this file inside a checkout of the PARENT commit measures the parent; run the two alternately, two each, on one box.
  full mode     python tools/bench_copy_paste.py full [OUT.json] [--none A.json B.json] [--parent C.json D.json] [--step-img-per-s X]
                the loader with the default CopyPaste() (two runs), the host time inside the paste stage and its draws, the three kernels
                alone on one batch's item table by HIP events (the pixel kernel also as bytes moved over time), and, with --step-img-per-s
                (bench.py's value on the same box in the same visit), the ratio to the training step.  Default OUT: profiles/copy_paste_bench.json"""
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ryolov4_amd.datasets import augment as A
from ryolov4_amd.datasets.scene_dataset import SceneDataset

HYP = {"hsv_h": 0.015, "hsv_s": 0.7, "hsv_v": 0.4, "rotate": 45, "translate": 0.1, "scale": 0.5, "flipud": 0.5, "fliplr": 0.5, "mosaic": 1.0, "mixup": 0.15}
B, S, ITERS, NSCENE, NLAB = 64, 800, 20, 8, 500
STREAM_TBPS = 6.3            # what this part sustains on streaming kernels


def scenes():
    """tools/bench_scene_loader.py's scenes and labels (same generator, same seed)."""
    side = 5 * S
    rs = np.random.RandomState(0)
    base = rs.randint(0, 256, size=(side + 64, side + 64, 3), dtype=np.uint8)
    imgs = [base[o:o + side, o:o + side] for o in rs.randint(0, 64, size=NSCENE)]
    polys, labels = [], []
    for _ in range(NSCENE):
        c = rs.rand(NLAB, 2) * side
        d = (rs.rand(NLAB, 4, 2) - 0.5) * 60
        polys.append((c[:, None, :] + d).reshape(NLAB, 8).astype(np.float32))
        labels.append(rs.randint(0, 16, size=NLAB).astype(np.float32))
    return imgs, polys, labels


def dataset(data, **kw):
    ds = SceneDataset(HYP, S, True, False, device=torch.device("cuda:0"), overlap=S // 4, jitter=True, keep_empty=True, **kw)
    ds.set_arrays(*data)
    return ds


def feed_rate(ds, seed=0):
    n = len(ds)
    random.seed(seed)
    np.random.seed(seed)
    for _ in range(3):
        ds.assemble_batch([random.randrange(n) for _ in range(B)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nt = 0
    for _ in range(ITERS):
        _, _, tg = ds.assemble_batch([random.randrange(n) for _ in range(B)])
        nt += tg.shape[0]
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / ITERS
    return {"ms_per_batch": round(dt * 1e3, 2), "img_per_s": round(B / dt, 1), "targets_per_batch": nt // ITERS}


def gpu_ms(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def host_ms(ds, seed=3):
    """Host milliseconds per batch inside the paste stage and inside its parts (every launch is asynchronous)."""
    cp = ds.copy_paste
    spent = {}

    def timed(obj, name, key):
        f = getattr(obj, name)

        def g(*a, **k):
            t = time.perf_counter()
            out = f(*a, **k)
            spent[key] = spent.get(key, 0.0) + time.perf_counter() - t
            return out
        setattr(obj, name, g)
    timed(ds, "_canvas_stage", "canvas_stage")
    timed(ds, "paste_bank", "bank")
    timed(cp, "draw", "draws")
    timed(cp, "items", "item_table")
    n = len(ds)
    random.seed(seed)
    np.random.seed(seed)
    pastes = 0
    for _ in range(ITERS):
        ds.assemble_batch([random.randrange(n) for _ in range(B)])
        pastes += len(ds.last_pastes)
    torch.cuda.synchronize()
    for obj, name in ((ds, "_canvas_stage"), (ds, "paste_bank"), (cp, "draw"), (cp, "items")):
        delattr(obj, name)
    out = {k: round(v / ITERS * 1e3, 3) for k, v in spent.items()}
    out["uploads_and_launches"] = round(out["canvas_stage"] - out["bank"] - out["draws"] - out["item_table"], 3)
    out["pastes_per_batch"] = pastes / ITERS
    return out


def written_pixels(dq, bbox, slots):
    """Canvas pixels inside at least one item of their slot (what the pixel kernel writes), counted on the host from the device's own
    destination quads and boxes with the kernel's edge expression."""
    masks = {}
    for q, (x0, y0, x1, y1), s in zip(dq.astype(np.float64), bbox, slots):
        if x1 <= x0 or y1 <= y0:
            continue
        px, py = np.meshgrid(np.arange(x0, x1, dtype=np.float64), np.arange(y0, y1, dtype=np.float64))
        v = q.reshape(4, 2)
        sh = sum(v[k, 0] * v[(k + 1) % 4, 1] - v[(k + 1) % 4, 0] * v[k, 1] for k in range(4))
        sg = 1.0 if sh > 0 else -1.0
        m = np.ones(px.shape, dtype=bool)
        for k in range(4):
            a, b = v[k], v[(k + 1) % 4]
            m &= sg * ((b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])) >= 0
        full = masks.setdefault(int(s), np.zeros((S, S), dtype=bool))
        full[y0:y1, x0:x1] |= m
    return int(sum(m.sum() for m in masks.values()))


def kernels_alone(ds):
    """The three kernels on the item table of one batch: HIP events over 20 launches each, tables uploaded once."""
    seen = {}
    real = A.paste_objects

    def spy(pool, final, targets10, items, occ_thr=0.5):
        seen.update(final=final.clone(), targets10=targets10.clone(), items=np.array(items), occ_thr=occ_thr)
        return real(pool, final, targets10, items, occ_thr)
    A.paste_objects = spy
    try:
        random.seed(2)
        np.random.seed(2)
        ds.assemble_batch([random.randrange(len(ds)) for _ in range(B)])
    finally:
        A.paste_objects = real
    pool_buf, final, tg, items = ds._pool.buf, seen["final"], seen["targets10"], seen["items"]
    table = A.PasteTable(items, B, final.device)
    out = {"items": table.n, "existing_rows": int(tg.shape[0]), "max_box": list(table.max_box)}
    out["prepare_ms"] = round(gpu_ms(lambda: A.paste_prepare(table, S)), 4)
    out["pixels_ms"] = round(gpu_ms(lambda: A.paste_pixels(pool_buf, table, final)), 4)
    out["labels_ms"] = round(gpu_ms(lambda: A.paste_labels(table, tg, seen["occ_thr"])), 4)
    bbox = table.bbox.cpu().numpy()
    npx = written_pixels(table.dq.cpu().numpy(), bbox, items["slot"])
    box_px = int(((bbox[:, 2] - bbox[:, 0]) * (bbox[:, 3] - bbox[:, 1])).sum())
    moved = npx * (3 + 16)                     # 3 bytes written, two 8-byte tap loads per written pixel
    out.update(written_pixels=npx, box_pixels=box_px, canvas_pixels=B * S * S, bytes_moved=moved,
               pixels_GBps=round(moved / out["pixels_ms"] / 1e6, 2), share_of_streaming_rate=round(moved / out["pixels_ms"] / 1e9 / STREAM_TBPS, 5))
    return out


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "full"
    data = scenes()
    if mode == "loader":
        res = {"copy_paste_none": feed_rate(dataset(data))}
        json.dump(res, open(sys.argv[2], "w"), indent=1)
        print(json.dumps(res))
        return
    args = sys.argv[2:]
    path = args[0] if args and not args[0].startswith("--") else os.path.join("profiles", "copy_paste_bench.json")

    def files(flag):
        if flag not in args:
            return []
        k = args.index(flag) + 1
        got = []
        while k < len(args) and not args[k].startswith("--"):
            got.append(json.load(open(args[k]))["copy_paste_none"])
            k += 1
        return got
    from ryolov4_amd.datasets.copy_paste import CopyPaste
    res = {"copy_paste_none_runs": files("--none"), "parent_commit_runs": files("--parent")}
    none, on = dataset(data), dataset(data, copy_paste=CopyPaste())
    res["copy_paste_none_in_process"] = [feed_rate(none)]
    res["copy_paste_default"] = [feed_rate(on)]
    res["copy_paste_none_in_process"].append(feed_rate(none, seed=1))
    res["copy_paste_default"].append(feed_rate(on, seed=1))
    res["host_ms_per_batch"] = host_ms(on)
    res["kernels_alone"] = kernels_alone(on)
    if "--step-img-per-s" in args:
        step = float(args[args.index("--step-img-per-s") + 1])
        res["training_step_img_per_s"] = step
        res["loader_with_copy_paste_over_step"] = [round(r["img_per_s"] / step, 2) for r in res["copy_paste_default"]]
        res["loader_without_over_step"] = [round(r["img_per_s"] / step, 2) for r in res["copy_paste_none_in_process"]]
    out = {"what": f"scene loader with and without copy-paste, batch {B} at {S}x{S}, augment=True (mosaic 1.0, mixup 0.15, hsv, warp, flips), jitter on; "
                   f"{NSCENE} synthetic {5 * S}x{5 * S} scenes with {NLAB} labels each (random quadrilaterals: the strictly convex ones are the bank); wall "
                   "clock over 20 batches incl. host planning and the count read-back; one box, one visit",
           "result": res}
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
