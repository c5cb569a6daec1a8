"""DOTA-protocol matching: what it costs.  Writes one JSON document (default profiles/dota_eval_match.json) and prints it.

(a) match   ryolo_dota_match (float64 clip against the annotated quads, three thresholds' owner tables) against ryolo_scene_match (the float
            pair function of the NMS, the reference's rule) on the same box in the same visit: the generated scene of tests/scene_eval_ref.py
            at 5 000 detections x 2 000 labels x 16 classes, the labels of the new path as jittered quads with a quarter difficult.  Two
            runs each, alternating (new, old, new, old), every run timed by events around each of REPS calls after warm-up (the cursors
            reset outside the timed region).  Both times and their ratio are written down.  No condition: the float64 clip is expected to
            cost a multiple of the float pair function, and this measures which.
(b) ap      ryolo_ap_voc on the rows of (a), both metrics.
(c) scene   scene_ms of tools/bench_tiled.py's standing configuration (yolov7 kfiou nc = 16, synthetic weights, 4000 x 4000 scene, S = 1024,
            overlap 200, batch 8) with and without DotaEvaluator.add per scene (2 000 quads uploaded per scene), as a share of scene_ms next
            to glue_share.  No condition.  The weights are synthetic: the mAP of these runs means nothing and is not reported.
Environment: REPS (20), N (scene iterations, 10), PART (any of a, b, c; default abc)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ryolov4_amd import hip
from ryolov4_amd.lib import general
from ryolov4_amd.lib.dota_eval import GRID11, DotaEvaluator
from ryolov4_amd.lib.scene_eval import group_labels
from tests import dota_eval_ref as D
from tests import scene_eval_ref as R

dev = torch.device("cuda:0")
REPS, N, PART = int(os.environ.get("REPS", 20)), int(os.environ.get("N", 10)), os.environ.get("PART", "abc")
NDET, NLAB, NC = 5000, 2000, 16
IOUV = (0.5, 0.75, 0.9)
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dota_eval_match.json")


def timed(prepare, call, reps=REPS, warm=3):
    """Mean milliseconds of call() over `reps`, one event pair per call; prepare() runs before every call, outside the pair."""
    for _ in range(warm):
        prepare()
        call()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(reps):
        prepare()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in pairs) / reps


def part_ab():
    per_class = np.random.default_rng(7).multinomial(NLAB, np.full(NC, 1.0 / NC))
    dets, boxes, classes = R.make_scene(7, tuple(int(c) for c in per_class), NDET)
    quads, _ = D.box_quads(boxes, 8)
    hard = (np.random.default_rng(9).random(NLAB) < 0.25).astype(np.float32)
    src = torch.from_numpy(dets).to(dev)
    num = torch.tensor([NDET], dtype=torch.int32, device=dev)
    order, off = group_labels(classes, NC)
    cls_off = torch.from_numpy(off).to(dev)
    conf, pcls = torch.zeros(NDET, device=dev), torch.zeros(NDET, device=dev)
    need = hip._Z()
    # new
    q = torch.from_numpy(quads[order]).to(dev)
    lab_new = torch.cat([torch.from_numpy(np.stack([classes[order], hard[order]], 1)).to(dev), q, general.xyxyxyxy2xywha(q)], 1).contiguous()
    iouv_new = torch.tensor(IOUV, dtype=torch.float32, device=dev)
    status = torch.zeros((NDET, len(IOUV)), dtype=torch.uint8, device=dev)
    state_new = torch.zeros(2, dtype=torch.int64, device=dev)
    npos = torch.zeros(NC, dtype=torch.int64, device=dev)
    hip.call("ryolo_dota_match_workspace_bytes", NDET, NLAB, len(IOUV), need)
    ws_new = torch.empty(need.value, dtype=torch.uint8, device=dev)
    # old
    lab_old = torch.from_numpy(np.concatenate([classes[order, None], boxes[order]], 1)).to(dev)
    iouv_old = R.IOUV.float().to(dev)
    tp = torch.zeros((NDET, 10), dtype=torch.uint8, device=dev)
    state_old = torch.zeros(2, dtype=torch.int64, device=dev)
    hip.call("ryolo_scene_match_workspace_bytes", NDET, NLAB, need)
    ws_old = torch.empty(need.value, dtype=torch.uint8, device=dev)

    def prepare():
        state_new.zero_()
        state_old.zero_()
        npos.zero_()

    def new():
        hip.call("ryolo_dota_match", hip.ptr(src), hip.ptr(num), NDET, hip.ptr(lab_new), hip.ptr(cls_off), NLAB, NC, hip.ptr(iouv_new), len(IOUV),
                 hip.ptr(status), hip.ptr(conf), hip.ptr(pcls), NDET, state_new.data_ptr(), state_new.data_ptr() + 8, hip.ptr(npos), hip.ptr(ws_new),
                 ws_new.numel(), hip.stream())

    def old():
        hip.call("ryolo_scene_match", hip.ptr(src), hip.ptr(num), NDET, hip.ptr(lab_old), hip.ptr(cls_off), NLAB, NC, hip.ptr(iouv_old), 10, hip.ptr(tp),
                 hip.ptr(conf), hip.ptr(pcls), NDET, state_old.data_ptr(), state_old.data_ptr() + 8, hip.ptr(ws_old), ws_old.numel(), hip.stream())

    res = {}
    if "a" in PART:
        t_new, t_old = [], []
        for _ in range(2):
            t_new.append(timed(prepare, new))
            t_old.append(timed(prepare, old))
        res["match"] = {"detections": NDET, "labels": NLAB, "classes": NC, "thresholds": list(IOUV), "reps": REPS,
                        "true_positives_at_0.5": int((status[:, 0] == 1).sum()), "ignored_at_0.5": int((status[:, 0] == 2).sum()),
                        "scene_match_true_positives_at_0.5": int(tp[:, 0].sum()), "dota_match_ms": [round(t, 4) for t in t_new],
                        "scene_match_ms": [round(t, 4) for t in t_old], "spread_ms": round(max(abs(t_new[0] - t_new[1]), abs(t_old[0] - t_old[1])), 4),
                        "ratio_dota_over_scene": round(min(t_new) / min(t_old), 2)}
    if "b" in PART:
        prepare()
        new()
        grid = torch.from_numpy(GRID11).to(dev)
        ap = torch.zeros((NC, len(IOUV)), dtype=torch.float64, device=dev)
        n_pred = torch.zeros(NC, dtype=torch.int64, device=dev)
        hip.call("ryolo_ap_voc_workspace_bytes", NDET, len(IOUV), NC, need)
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        res["ap"] = {"rows": NDET}
        for metric, name in ((0, "voc07"), (1, "voc12")):
            t = timed(lambda: None, lambda: hip.call("ryolo_ap_voc", hip.ptr(status), hip.ptr(conf), hip.ptr(pcls), NDET, hip.ptr(npos), NC, len(IOUV), metric,
                                                     hip.ptr(grid), hip.ptr(ws), ws.numel(), hip.ptr(ap), hip.ptr(n_pred), hip.stream()))
            res["ap"][name + "_ms"] = round(t, 4)
    return res


def part_c():
    from ryolov4_amd.lib.tiled import TiledDetector, tile_plan
    from ryolov4_amd.model.yolo import Yolo
    from ryolov4_amd.synth import CFG, fill_state
    SC, S, OV, B, CONF = 4000, 1024, 200, 8, 0.1
    net = Yolo(NC, CFG, "kfiou", "yolov7")
    net.load_state_dict(fill_state(net.state_dict()))
    det = TiledDetector(net.to(dev).eval(), size=S, overlap=OV, batch=B, conf_thres=CONF, iou_thres=0.4)
    scene = torch.from_numpy(np.random.RandomState(0).randint(0, 256, (SC, SC, 3)).astype(np.uint8)).to(dev)
    rs = np.random.RandomState(1)
    boxes = np.stack([rs.uniform(0, SC, NLAB), rs.uniform(0, SC, NLAB), rs.uniform(8, 30, NLAB), rs.uniform(30, 90, NLAB),
                      rs.uniform(-1.5, 1.5, NLAB)], 1).astype(np.float32)
    quads, _ = D.box_quads(boxes, 2)
    classes = rs.randint(0, NC, NLAB).astype(np.float32)
    hard = (rs.rand(NLAB) < 0.25).astype(np.uint8)
    ev = DotaEvaluator(NC, iouv=IOUV, device=dev)
    groups = -(-len(tile_plan(SC, SC, S, OV)) // B)

    def wall(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ev.reset()
        t0 = time.perf_counter()
        for _ in range(N):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / N

    def plain():
        out, num = det.run_async(scene)
        return int(num.item())

    def scored():
        out, num = det.run_async(scene)
        ev.add(out, num, quads, classes, hard)
        return int(num.item())

    def replays():
        for _ in range(groups):
            det.run.graph.replay()
        torch.cuda.synchronize()

    t_plain, t_scored, t_plain2, t_scored2, t_rep = wall(plain), wall(scored), wall(plain), wall(scored), wall(replays)
    p, s = min(t_plain, t_plain2), min(t_scored, t_scored2)
    return {"scene": SC, "S": S, "overlap": OV, "batch": B, "conf_thres": CONF, "labels": NLAB, "detections": plain(), "iterations": N,
            "scene_ms": [round(t_plain, 3), round(t_plain2, 3)], "scene_ms_with_add": [round(t_scored, 3), round(t_scored2, 3)],
            "replay_ms": round(t_rep, 3), "glue_share": round((p - t_rep) / p, 4), "eval_ms": round(s - p, 3), "eval_share": round((s - p) / p, 4),
            "glue_plus_eval_share": round((s - t_rep) / s, 4)}


res = {"device": torch.cuda.get_device_name(0)}
if "a" in PART or "b" in PART:
    res.update(part_ab())
if "c" in PART:
    res["scene"] = part_c()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
