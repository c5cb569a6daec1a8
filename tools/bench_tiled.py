"""Full-scene (tiled) detection throughput: yolov7 kfiou nc=16 (synth.fill_state weights), a synthetic 4000 x 4000 scene, S=1024,
overlap=200, batch=8 (25 windows in 4 groups; with VIEWS every window once per view: entries = windows x views in groups of 8).  Prints
one JSON line:
  scene_ms / windows_per_s        TiledDetector.run_async + the count read, per scene
  entries / entry_ms              windows x views, and scene_ms per entry
  replay_ms                       the same number of bare captured-graph replays (forward + post_process in the graph)
  glue_ms / glue_share            scene_ms - replay_ms: cut, collect, merge, final order, launches (target <= 5 % of scene time)
  naive_ms                        the Python loop a user writes today: per-window device slicing + to-tensor, the captured forward without
                                  post, post_process per group, a host-side shift, per-class nms_rotated
  files_overlap_ms / files_serial_ms   detect_files over 8 scenes with / without the side-stream upload overlap (decode = an in-memory copy)
  merge_ms                        ScenePlan.merge alone on the scene's collected candidates, by device events (the detector's fuse / seam)
The naive loop has no views: naive_ms and speedup_vs_naive compare like with like only for VIEWS=id.
With SEAM set (the seam leg) the line also carries, per scene: merge_ms_seam_off (the same merge with seam=None on the same candidates),
seam_flags_ms and seam_cover_ms (ryolo_tile_seam_flags / ryolo_tile_seam_cover alone, device events), seam_share_of_merge, nms_ms
(ryolo_nms_rotated_batched of the same merge on the same inputs: the yardstick of the cover kernel, which evaluates cut x kept pairs
against the NMS's half-square over all selected candidates), and the counts candidates / cut / redundant / covered / kept.
Environment: SCENE (4000), S (1024), OVERLAP (200), B (8), CONF (0.1), N (iterations, 10), VIEWS (comma list of lib.tiled.VIEWS names, id),
FUSE (box | wbf: cluster fusion in the merge; unset = none), SEAM (unset = none; 1 = Seam(); or margin,cover,whole with cover "none" for
rule 1 alone, e.g. 2,0.7,1)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ryolov4_amd import hip
from ryolov4_amd.lib import general
from ryolov4_amd.lib.tiled import Seam, TiledDetector, tile_entries, tile_plan
from ryolov4_amd.model.yolo import Yolo
from ryolov4_amd.synth import CFG, fill_state

dev = torch.device("cuda:0")
SC, S, OV, B = int(os.environ.get("SCENE", 4000)), int(os.environ.get("S", 1024)), int(os.environ.get("OVERLAP", 200)), int(os.environ.get("B", 8))
CONF, IOU, N = float(os.environ.get("CONF", 0.1)), 0.4, int(os.environ.get("N", 10))
VIEWS = tuple(v.strip() for v in os.environ.get("VIEWS", "id").split(",") if v.strip())
FUSE = os.environ.get("FUSE", "").strip() or None
SEAM = os.environ.get("SEAM", "").strip() or None
if SEAM is not None:
    _s = SEAM.split(",")
    SEAM = Seam() if len(_s) == 1 else Seam(float(_s[0]), None if _s[1].lower() == "none" else float(_s[1]), bool(int(_s[2])))

net = Yolo(16, CFG, "kfiou", "yolov7")
net.load_state_dict(fill_state(net.state_dict()))
net.to(dev).eval()
det = TiledDetector(net, size=S, overlap=OV, batch=B, conf_thres=CONF, iou_thres=IOU, views=VIEWS, fuse=FUSE, seam=SEAM)
scene = np.random.RandomState(0).randint(0, 256, (SC, SC, 3)).astype(np.uint8)
scene_dev = torch.from_numpy(scene).to(dev)
wins = tile_plan(SC, SC, S, OV)
entries = len(tile_entries(SC, SC, S, OV, views=VIEWS))
groups = -(-len(wins) // B)                                     # of the naive loop (windows only)
egroups = -(-entries // B)                                      # replays per scene


def wall(fn, n=N):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def tiled():
    out, num = det.run_async(scene_dev)
    return int(num.item())


def replays():
    for _ in range(egroups):
        det.run.graph.replay()
    torch.cuda.synchronize()


bare = net.capture_inference(B, S)                              # forward + decode only: the naive loop runs post_process itself


def naive():
    pad = torch.nn.functional.pad
    dets = []
    for g in range(groups):
        ws = wins[g * B:(g + 1) * B]
        imgs = torch.zeros((B, 3, S, S), dtype=torch.float32, device=dev)
        for k, (_, x0, y0) in enumerate(ws):
            w = scene_dev[y0:y0 + S, x0:x0 + S]
            w = pad(w.permute(2, 0, 1), (0, S - w.shape[1], 0, S - w.shape[0]), value=114)
            imgs[k] = w.flip(0).float() / 255
        _, infer = bare(imgs)
        res = general.post_process(infer, CONF, IOU)
        for k, (_, x0, y0) in enumerate(ws):
            d = res[k].cpu()
            d[:, 0] += x0
            d[:, 1] += y0
            dets.append(d)
    d = torch.cat(dets).to(dev)
    keep = []
    for c in d[:, 6].unique():
        idx = torch.nonzero(d[:, 6] == c)[:, 0]
        b = d[idx, :5].clone()
        b[:, 4] = b[:, 4] / np.pi * 180
        keep.append(idx[general.nms_rotated(b, d[idx, 5], IOU)])
    return len(torch.cat(keep)) if keep else 0


files = [f"scene{i}" for i in range(8)]


def read(path):
    return scene.copy()                                        # stands in for the decode


def run_files(overlap):
    return sum(len(d) for _, d in det.detect_files(files, imread=read, overlap=overlap))


def events(fn, n=max(N, 20)):
    """ms per call of fn by device events (fn only launches)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n


def merge_leg():
    """The merge alone on the candidates the last scene left in its plan, and with SEAM its two kernels against the NMS of that merge."""
    p = det.plan(SC, SC)
    res = {"merge_ms": round(events(lambda: p.merge_seam(det.merge_iou, det.gt_only, det.fuse, det.seam)), 4)}
    if det.seam is None:
        return res
    sm, st, nc, Kc = det.seam, hip.stream(), p.nc, p.Kc
    res["merge_ms_seam_off"] = round(events(lambda: p.merge(det.merge_iou, det.gt_only, det.fuse)), 4)
    p.merge_seam(det.merge_iou, det.gt_only, det.fuse, sm)                    # the state the three calls below are timed on
    fkey = p.key2[nc]
    t_flags = events(lambda: hip.call("ryolo_tile_seam_flags", hip.ptr(p.cand), hip.ptr(p.key), hip.ptr(p.win), hip.ptr(p.geom), p.T, p.nviews, p.mk,
                                      p.ld, nc, p.size, sm.margin, 1 if sm.whole else 0, hip.ptr(p.flags), hip.ptr(p.key2), hip.ptr(p.seam_counts), st))
    p.merge_seam(det.merge_iou, det.gt_only, det.fuse, sm)                    # the flags calls reset the final key: mark it again
    t_cover = 0.0
    if sm.cover is not None:
        t_cover = events(lambda: hip.call("ryolo_tile_seam_cover", hip.ptr(p.rboxes), hip.ptr(p.order), hip.ptr(p.nsel), hip.ptr(p.keep), hip.ptr(p.nkeep),
                                          nc, Kc, Kc, hip.ptr(p.flags), p.ld, sm.cover, hip.ptr(fkey), hip.ptr(p.seam_counts), hip.ptr(p.seam_ws),
                                          p.seam_ws.numel(), st))
    t_nms = events(lambda: hip.call("ryolo_nms_rotated_batched", hip.ptr(p.rboxes), hip.ptr(p.nsel), nc, Kc, det.merge_iou, 1 if det.gt_only else 0, Kc,
                                    hip.ptr(p.nms_ws), p.nms_ws.numel(), hip.ptr(p.keep), Kc, hip.ptr(p.nkeep), st))
    _, num = p.merge_seam(det.merge_iou, det.gt_only, det.fuse, sm)
    flags, counts = p.flags.cpu().numpy(), p.seam_counts.cpu().tolist()
    res.update(seam={"margin": sm.margin, "cover": sm.cover, "whole": sm.whole}, seam_flags_ms=round(t_flags, 4), seam_cover_ms=round(t_cover, 4),
               seam_share_of_merge=round((t_flags + t_cover) / res["merge_ms"], 4), nms_ms=round(t_nms, 4),
               candidates=int((p.key > -float("inf")).sum().item()), selected=int(p.nsel.sum().item()), kept=int(p.nkeep.sum().item()),
               cut=int(((flags & 15) != 0).sum()), redundant=counts[0], covered=counts[1], detections_seam=int(num.item()))
    return res


t_scene = wall(tiled)
leg = merge_leg()
t_rep = wall(replays)
t_naive = wall(naive, max(2, N // 3))
t_fo = wall(lambda: run_files(True), 2) / len(files)
t_fs = wall(lambda: run_files(False), 2) / len(files)
n_tiled, n_naive = tiled(), naive()
print(json.dumps({"scene": SC, "S": S, "overlap": OV, "batch": B, "views": list(VIEWS), "fuse": FUSE, "windows": len(wins), "entries": entries, "groups": egroups,
                  "padded_slots": egroups * B - entries,
                  "conf_thres": CONF, "detections": n_tiled, "naive_detections": n_naive,
                  "scene_ms": round(t_scene, 3), "entry_ms": round(t_scene / entries, 3), "windows_per_s": round(len(wins) / t_scene * 1e3, 1), "replay_ms": round(t_rep, 3),
                  "glue_ms": round(t_scene - t_rep, 3), "glue_share": round((t_scene - t_rep) / t_scene, 4), "naive_ms": round(t_naive, 3),
                  "speedup_vs_naive": round(t_naive / t_scene, 2), "files_overlap_ms": round(t_fo, 3), "files_serial_ms": round(t_fs, 3), **leg}))
