"""Feed rate of the scene loader (datasets/scene_dataset.py) against the split-window loader on THE SAME windows, at the benchmark's batch:
64 samples of 800x800, every augmentation on (tools/bench_pipeline.py's hyper-parameters), synthetic 4000x4000 scenes with ~500 labels.

  scene_jitter / scene_planned   SceneDataset over the scenes (windows cut on the device; origins redrawn per use / as planned)
  split (two runs)               BaseDataset over the planned windows cut on the host, labels pre-filtered (what an offline split gives);
                                 the two runs give the run-to-run spread
  host_ms_in_hooks               host time per batch inside each first-stage hook of assemble_batch, per loader: where a difference comes from
  stages                         the first stage alone on one batch's table: the copy path (interp 2, with and without hsv) of
                                 ryolo_resize_hsv_windows against ryolo_resize_hsv_batch on the same bytes (GPU time, GB/s read + write),
                                 and ryolo_scene_label_rows
usage: python tools/bench_scene_loader.py [batch] [size] [iters] [scenes] [out.json]  (default profiles/scene_loader_feed_rate.json)
       python tools/bench_scene_loader.py [batch] [size] [iters] [scenes] out.json ignore
           only the scene_jitter loader, with ignore=None and with ignore=Ignore(0.1, True) (a tenth of the labels difficult), two runs
           each, alternating: what the shadow table of the ignore rows costs per batch
       python tools/bench_scene_loader.py [batch] [size] [iters] [scenes] out.json rotate
           the scene_jitter loader with rotate=None and with Rotate(degrees=180, p=1), two runs each, alternating, the host time in the
           hooks, and one launch of the window stage over a batch of windows copied against the same windows read at an angle"""
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ryolov4_amd import hip
from ryolov4_amd.datasets import augment as A
from ryolov4_amd.datasets.base_dataset import BaseDataset
from ryolov4_amd.datasets.scene_dataset import SceneDataset

HYP = {"hsv_h": 0.015, "hsv_s": 0.7, "hsv_v": 0.4, "rotate": 45, "translate": 0.1, "scale": 0.5, "flipud": 0.5, "fliplr": 0.5, "mosaic": 1.0, "mixup": 0.15}


def feed_rate(ds, B, iters, seed=0):
    n = len(ds)
    random.seed(seed)
    np.random.seed(seed)
    for _ in range(3):
        ds.assemble_batch([random.randrange(n) for _ in range(B)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    nt = 0
    for _ in range(iters):
        _, _, tg = ds.assemble_batch([random.randrange(n) for _ in range(B)])
        nt += tg.shape[0]
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    return {"ms_per_batch": round(dt * 1e3, 2), "img_per_s": round(B / dt, 1), "targets_per_batch": nt // iters}


HOOKS = ("_use_shape", "_use_labels", "_pixel_stage", "_label_table")


def hook_ms(ds, B, iters, seed=3):
    """Host milliseconds per batch inside each first-stage hook of assemble_batch (the loaders differ in nothing else), and the calls per
    batch: the feed rate is host-bound, every launch is asynchronous."""
    spent, calls = dict.fromkeys(HOOKS, 0.0), dict.fromkeys(HOOKS, 0)
    for name in HOOKS:
        def timed(*a, _f=getattr(ds, name), _n=name):
            t = time.perf_counter()
            out = _f(*a)
            spent[_n] += time.perf_counter() - t
            calls[_n] += 1
            return out
        setattr(ds, name, timed)
    n = len(ds)
    random.seed(seed)
    np.random.seed(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        ds.assemble_batch([random.randrange(n) for _ in range(B)])
    torch.cuda.synchronize()
    total = (time.perf_counter() - t0) / iters
    for name in HOOKS:
        delattr(ds, name)
    out = {name: {"ms": round(spent[name] / iters * 1e3, 3), "calls": calls[name] // iters} for name in HOOKS}
    out["batch_ms"] = round(total * 1e3, 2)
    return out


def gpu_ms(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    S = int(sys.argv[2]) if len(sys.argv) > 2 else 800
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    nscene = int(sys.argv[4]) if len(sys.argv) > 4 else 8
    side, nlab = 5 * S, 500
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    base = rs.randint(0, 256, size=(side + 64, side + 64, 3), dtype=np.uint8)
    scenes = [base[o:o + side, o:o + side] for o in rs.randint(0, 64, size=nscene)]
    polys, labels = [], []
    for _ in range(nscene):
        c = rs.rand(nlab, 2) * side
        d = (rs.rand(nlab, 4, 2) - 0.5) * 60
        polys.append((c[:, None, :] + d).reshape(nlab, 8).astype(np.float32))
        labels.append(rs.randint(0, 16, size=nlab).astype(np.float32))
    if len(sys.argv) > 6 and sys.argv[6] == "ignore":
        from ryolov4_amd.datasets.scene_dataset import Ignore
        diff = [(rs.rand(nlab) < 0.1).astype(np.uint8) for _ in range(nscene)]
        res, rows = {}, 0
        dss = {}
        for name, ig in (("ignore_off", None), ("ignore_on", Ignore(0.1, True))):
            dss[name] = SceneDataset(HYP, S, True, False, device=dev, overlap=S // 4, jitter=True, keep_empty=True, ignore=ig)
            dss[name].set_arrays(scenes, polys, labels, difficult=diff)
        for run in (1, 2):
            for name, ds in dss.items():
                res[f"{name}_run{run}"] = feed_rate(ds, B, iters, seed=run)
                if ds.last_ignore is not None:
                    rows = int(ds.last_ignore.shape[0])
        out = {"what": f"scene loader feed rate with and without ignore rows, batch {B} at {S}x{S}, augment=True (mosaic 1.0, mixup 0.15, hsv, warp, flips), "
                       f"{nscene} synthetic {side}x{side} scenes with {nlab} labels each, a tenth of them difficult; wall clock incl. host planning and "
                       "the read-backs of the row counts", "result": res, "ignore_rows_of_the_last_batch": rows}
        json.dump(out, open(sys.argv[5], "w"), indent=1)
        print(json.dumps(out))
        return
    if len(sys.argv) > 6 and sys.argv[6] == "rotate":
        from ryolov4_amd.datasets.scene_dataset import Rotate
        res, dss = {}, {}
        for name, rot in (("rotate_off", None), ("rotate_on", Rotate(degrees=180.0, p=1.0))):
            dss[name] = SceneDataset(HYP, S, True, False, device=dev, overlap=S // 4, jitter=True, keep_empty=True, rotate=rot)
            dss[name].set_arrays(scenes, polys, labels)
        for run in (1, 2):
            for name, ds in dss.items():
                res[f"{name}_run{run}"] = feed_rate(ds, B, iters, seed=run)
        host = {name: hook_ms(ds, B, iters) for name, ds in dss.items()}
        # the window stage alone: B windows of the last rotated batch, copied and read at their drawn angles (tables uploaded once)
        ds = dss["rotate_on"]
        wins, angles = list(ds.last_windows)[:B], list(ds.last_angles)[:B]
        ds._pool.ensure(range(nscene))
        stages = {"items": len(wins)}
        for tag, lut in (("plain", -1), ("hsv", 0)):
            ltd = None if lut < 0 else A._to_device(np.ascontiguousarray(A.hsv_luts(np.asarray([1.01, 1.3, 0.8])), dtype=np.uint8), dev)
            for mode in ("copied", "rotated"):
                arr = (A._WindowItem * len(wins))()
                total = 0
                for k, ((_, s, x0, y0, c), a) in enumerate(zip(wins, angles)):
                    sh, sw = ds._pool.shapes[s]
                    arr[k] = A._WindowItem(ds._pool.offsets[s], total, sh, sw, c, c, A.INTERP_COPY if mode == "copied" else A.INTERP_ROT, lut, x0, y0, c, 0)
                    if mode == "rotated":
                        arr[k].minv[:] = A.rot_window_maps(x0, y0, c, c, a)[0].tolist()
                    total += ((c * c * 3 + 15) // 16) * 16
                tab = A._to_device(arr, dev)
                stage = torch.empty(total, dtype=torch.uint8, device=dev)
                ms = gpu_ms(lambda: hip.call("ryolo_resize_hsv_windows", hip.ptr(ds._pool.buf), hip.ptr(tab), len(wins), S * S, hip.ptr(ltd), hip.ptr(stage),
                                             hip.stream()))
                nbytes = sum(w[4] * w[4] * 3 for w in wins)
                stages[f"{mode}_{tag}"] = {"ms": round(ms, 3), "MB_written": round(nbytes / 1e6, 1), "GBps_read_plus_written": round(2 * nbytes / ms / 1e6, 1)}
        out = {"what": f"scene loader feed rate with rotate=None and Rotate(degrees=180, p=1), batch {B} at {S}x{S}, augment=True (mosaic 1.0, mixup 0.15, hsv, "
                       f"warp, flips), {nscene} synthetic {side}x{side} scenes with {nlab} labels each, two runs each, alternating; wall clock incl. host "
                       "planning and the count read-back; host_ms_in_hooks as in the default leg; stages: one launch of ryolo_resize_hsv_windows over "
                       f"{len(wins)} windows of the last batch, copied (interp 2) and rotated (interp 3, the drawn angles), device events, 10 launches; "
                       "GB/s counts the result bytes twice (a rotated read touches up to 4 source pixels per result pixel, mostly from cache)",
               "result": res, "host_ms_in_hooks": host, "stages": stages}
        json.dump(out, open(sys.argv[5], "w"), indent=1)
        print(json.dumps(out))
        return
    res = {}
    sds = {}
    for name, jitter in (("scene_jitter", True), ("scene_planned", False)):
        ds = SceneDataset(HYP, S, True, False, device=dev, overlap=S // 4, jitter=jitter, keep_empty=True)
        ds.set_arrays(scenes, polys, labels)
        res[name] = feed_rate(ds, B, iters)
        sds[name] = ds
    planned = sds["scene_planned"]
    # the split: the planned windows cut on the host, their labels filtered by the label kernel (read back once)
    cuts, ps, cs = [], [], []
    for s, _, x0, y0, c in planned.items:
        cuts.append(np.ascontiguousarray(scenes[s][y0:y0 + c, x0:x0 + c]))                    # (no planned window hangs over a 5 S scene)
        p, k = planned._window_labels(s, x0, y0, c)
        if not len(k):
            ps.append(p)
            cs.append(k)
            continue
        rows = np.zeros(len(k), dtype=A.LABEL_ROW_DTYPE)
        rows["poly"] = p
        table = A.upload_label_rows(rows, dev)
        A.scene_label_rows(table, len(k), np.zeros(len(k), np.int32), [(x0, y0, c)], planned.iof_thr)
        back = np.frombuffer(table.cpu().numpy().tobytes(), dtype=A.LABEL_ROW_DTYPE)
        keep = ~np.isnan(back["poly"]).any(1)
        ps.append(back["poly"][keep].copy())
        cs.append(k[keep])
    split = BaseDataset(HYP, S, True, False, False, device=dev)
    split.set_arrays(cuts, ps, cs)
    res["split_run1"] = feed_rate(split, B, iters)
    res["split_run2"] = feed_rate(split, B, iters, seed=1)
    res["scene_jitter_run2"] = feed_rate(sds["scene_jitter"], B, iters, seed=1)
    host = {"scene_jitter": hook_ms(sds["scene_jitter"], B, iters), "scene_planned": hook_ms(planned, B, iters), "split": hook_ms(split, B, iters)}

    # ---- the first stage alone, on the table of one planned batch
    random.seed(2)
    np.random.seed(2)
    idx = [random.randrange(len(planned)) for _ in range(B)]
    planned.assemble_batch(idx)
    wins = list(planned.last_windows)
    luts = np.stack([A.hsv_luts(np.asarray([1.01, 1.3, 0.8])) for _ in wins])
    win_items = [(s, (x0, y0, c), (c, c), A.INTERP_COPY, k) for k, (_, s, x0, y0, c) in enumerate(wins)]
    cut_items = [(item, (c, c), A.INTERP_COPY, k) for k, (item, _, _, _, c) in enumerate(wins)]
    planned._pool.ensure(range(nscene))
    split._pool.ensure(w[0] for w in wins)
    nbytes = sum(c * c * 3 for _, _, _, _, c in wins)
    stages = {"uses": len(wins), "MB_per_direction": round(nbytes / 1e6, 1)}
    # the kernels alone: tables uploaded once
    for tag, lt in (("hsv", luts), ("plain", None)):
        ltd = None if lt is None else A._to_device(np.ascontiguousarray(lt, dtype=np.uint8), dev)
        strip = (lambda it: it) if lt is not None else (lambda it: it[:-1] + (-1,))
        warr = (A._WindowItem * len(wins))()
        barr = (A._ResizeItem * len(wins))()
        total = 0
        for k, (w, b) in enumerate(zip(win_items, cut_items)):
            w, b = strip(w), strip(b)
            sh, sw = planned._pool.shapes[w[0]]
            c = w[1][2]
            warr[k] = A._WindowItem(planned._pool.offsets[w[0]], total, sh, sw, c, c, A.INTERP_COPY, w[4], w[1][0], w[1][1], c, 0)
            barr[k] = A._ResizeItem(split._pool.offsets[b[0]], total, c, c, c, c, A.INTERP_COPY, b[3])
            total += ((c * c * 3 + 15) // 16) * 16
        wt, bt = A._to_device(warr, dev), A._to_device(barr, dev)
        stage = torch.empty(total, dtype=torch.uint8, device=dev)
        t_w = gpu_ms(lambda: hip.call("ryolo_resize_hsv_windows", hip.ptr(planned._pool.buf), hip.ptr(wt), len(wins), S * S, hip.ptr(ltd), hip.ptr(stage), hip.stream()))
        ref = stage.clone()
        t_b = gpu_ms(lambda: hip.call("ryolo_resize_hsv_batch", hip.ptr(split._pool.buf), hip.ptr(bt), len(wins), S * S, hip.ptr(ltd), hip.ptr(stage), hip.stream()))
        stages["kernel_" + tag] = {"windows_ms": round(t_w, 3), "batch_ms": round(t_b, 3), "windows_GBps": round(2 * nbytes / t_w / 1e6, 1),
                                   "batch_GBps": round(2 * nbytes / t_b / 1e6, 1), "same_bytes": bool(torch.equal(ref, stage))}
    # label stage of that batch
    parts, wor = [], []
    for k, (_, s, x0, y0, c) in enumerate(wins):
        p, _ = planned._window_labels(s, x0, y0, c)
        r = np.zeros(len(p), dtype=A.LABEL_ROW_DTYPE)
        r["poly"] = p
        parts.append(r)
        wor.append(np.full(len(p), k, np.int32))
    rows, wor = np.concatenate(parts), np.concatenate(wor)
    table = A.upload_label_rows(rows, dev)
    stages["label_rows"] = {"rows": len(rows), "ms_incl_upload": round(gpu_ms(lambda: A.scene_label_rows(table, len(rows), wor, [w[2:] for w in wins], 0.7)), 3)}
    out = {"what": f"scene loader vs split-window loader, batch {B} at {S}x{S}, augment=True (mosaic 1.0, mixup 0.15, hsv, warp, flips); {nscene} synthetic "
                   f"{side}x{side} scenes with {nlab} labels each ({nscene * side * side * 3 / 1e6:.0f} MB in HBM), {len(planned)} planned windows; wall clock "
                   "incl. host planning and the count read-back",
           "result": res, "host_ms_in_hooks": host, "stages": stages}
    path = sys.argv[5] if len(sys.argv) > 5 else os.path.join("profiles", "scene_loader_feed_rate.json")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
