"""Full-scene mAP matching: what it costs.  Writes one JSON document (default profiles/scene_eval_match.json) and prints it.

(a) match   ryolo_scene_match against the per-image kernel ryolo_map_match with batch = 1 on the same inputs: the generated scene of
            tests/scene_eval_ref.py at 5 000 detections x 2 000 labels x 16 classes.  Two runs each, alternating (new, old, new, old), every
            run timed by events around each of REPS calls after warm-up (inputs restored and the cursor reset outside the timed region).
            Condition: the new path is faster than the old kernel by more than the spread between the two runs of either.  Both numbers and
            their ratio are written down; the true-positive matrices of the two are compared as well.
(b) scene   scene_ms of tools/bench_tiled.py's standing configuration (yolov7 kfiou nc = 16, synthetic weights, 4000 x 4000 scene, S = 1024,
            overlap 200, batch 8) with and without SceneEvaluator.add per scene (2 000 labels uploaded per scene), as a share of scene_ms
            next to glue_share.  No condition.  The weights are synthetic: the mAP of these runs means nothing and is not reported.
Environment: REPS (20), N (scene iterations, 10), PART (a | b | ab)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ryolov4_amd import hip
from ryolov4_amd.lib.scene_eval import SceneEvaluator, group_labels
from tests import scene_eval_ref as R

dev = torch.device("cuda:0")
REPS, N, PART = int(os.environ.get("REPS", 20)), int(os.environ.get("N", 10)), os.environ.get("PART", "ab")
NDET, NLAB, NC = 5000, 2000, 16
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scene_eval_match.json")


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


def part_a():
    per_class = np.random.default_rng(7).multinomial(NLAB, np.full(NC, 1.0 / NC))
    dets, boxes, classes = R.make_scene(7, tuple(int(c) for c in per_class), NDET)
    iouv = R.IOUV.float().to(dev)
    src = torch.from_numpy(dets).to(dev)
    work = src.clone()
    # new
    order, off = group_labels(classes, NC)
    lab = torch.from_numpy(np.concatenate([classes[order, None], boxes[order]], 1)).to(dev)
    cls_off = torch.from_numpy(off).to(dev)
    num = torch.tensor([NDET], dtype=torch.int32, device=dev)
    tp_new = torch.zeros((NDET, 10), dtype=torch.uint8, device=dev)
    conf, pcls = torch.zeros(NDET, device=dev), torch.zeros(NDET, device=dev)
    state = torch.zeros(2, dtype=torch.int64, device=dev)
    need = hip._Z()
    hip.call("ryolo_scene_match_workspace_bytes", NDET, NLAB, need)
    ws_new = torch.empty(need.value, dtype=torch.uint8, device=dev)
    # old
    tg = R.targets_of(boxes, classes).to(dev)
    poff = torch.tensor([0, NDET], dtype=torch.int64, device=dev)
    toff = torch.tensor([0, NLAB], dtype=torch.int64, device=dev)
    tp_old = torch.zeros((NDET, 10), dtype=torch.uint8, device=dev)
    hip.call("ryolo_map_match_workspace_bytes", NDET, NLAB, need)
    ws_old = torch.empty(need.value, dtype=torch.uint8, device=dev)

    def prepare():
        work.copy_(src)                                               # the old kernel turns theta into degrees in place
        state.zero_()

    def new():
        hip.call("ryolo_scene_match", hip.ptr(work), hip.ptr(num), NDET, hip.ptr(lab), hip.ptr(cls_off), NLAB, NC, hip.ptr(iouv), 10, hip.ptr(tp_new),
                 hip.ptr(conf), hip.ptr(pcls), NDET, state.data_ptr(), state.data_ptr() + 8, hip.ptr(ws_new), ws_new.numel(), hip.stream())

    def old():
        hip.call("ryolo_map_match", hip.ptr(work), hip.ptr(poff), hip.ptr(tg), hip.ptr(toff), 1, NDET, NLAB, hip.ptr(iouv), 10, NC + 1, hip.ptr(tp_old),
                 hip.ptr(ws_old), ws_old.numel(), hip.stream())

    t_new, t_old = [], []
    for _ in range(2):
        t_new.append(timed(prepare, new))
        t_old.append(timed(prepare, old))
    spread = max(abs(t_new[0] - t_new[1]), abs(t_old[0] - t_old[1]))
    return {"detections": NDET, "labels": NLAB, "classes": NC, "reps": REPS, "true_positives_at_0.5": int(tp_new[:, 0].sum()),
            "tp_equal": bool(torch.equal(tp_new, tp_old)), "scene_match_ms": [round(t, 4) for t in t_new], "map_match_ms": [round(t, 4) for t in t_old],
            "spread_ms": round(spread, 4), "ratio_old_over_new": round(min(t_old) / max(t_new), 2),
            "faster_by_more_than_the_spread": bool(min(t_old) - max(t_new) > spread)}


def part_b():
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
    classes = rs.randint(0, NC, NLAB).astype(np.float32)
    ev = SceneEvaluator(NC, device=dev)
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
        ev.add(out, num, boxes, classes)
        return int(num.item())

    def replays():
        for _ in range(groups):
            det.run.graph.replay()
        torch.cuda.synchronize()

    t_plain, t_scored, t_plain2, t_scored2, t_rep = wall(plain), wall(scored), wall(plain), wall(scored), wall(replays)
    p, s = min(t_plain, t_plain2), min(t_scored, t_scored2)
    return {"scene": SC, "S": S, "overlap": OV, "batch": B, "conf_thres": CONF, "labels": NLAB, "detections": plain(), "iterations": N,
            "scene_ms": [round(t_plain, 3), round(t_plain2, 3)], "scene_ms_with_add": [round(t_scored, 3), round(t_scored2, 3)],
            "replay_ms": round(t_rep, 3), "glue_share": round((p - t_rep) / p, 4), "eval_ms": round(s - p, 3), "eval_share": round((s - p) / p, 4)}


res = {"device": torch.cuda.get_device_name(0)}
if "a" in PART:
    res["match"] = part_a()
if "b" in PART:
    res["scene"] = part_b()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
if "a" in PART and not (res["match"]["faster_by_more_than_the_spread"] and res["match"]["tp_equal"]):
    sys.exit(1)
