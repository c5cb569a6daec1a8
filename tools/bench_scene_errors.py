"""Full-scene error breakdown: what it costs.  Writes one JSON document (default profiles/scene_errors.json) and prints it.

ryolo_scene_errors against ryolo_scene_match (ten thresholds) on the same buffers in the same process: the generated scene of
tests/scene_eval_ref.py at 3 501 detections x 1 765 labels x 16 classes.  The existing matcher is the yardstick — the new one scans the
labels of every class, 16 times as many rows per detection, keeps two maxima and computes two more IoUs per detection.  Two runs each,
alternating (errors, match, errors, match), every run timed by events around each of REPS calls after warm-up (the cursor and the
histograms reset outside the timed region).  No condition: both times, the spread between the runs and the ratio are written down, with
the code and status counts of the scene (conf_thres 0) and whether the TP code equals the matcher's true positives at 0.5.
Environment: REPS (50)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from ryolov4_amd import hip
from ryolov4_amd.lib.scene_errors import CODES, STATUSES
from ryolov4_amd.lib.scene_eval import group_labels
from tests import scene_eval_ref as R

dev = torch.device("cuda:0")
REPS = int(os.environ.get("REPS", 50))
NC = R.SCENE_CLASSES
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scene_errors.json")


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


dets, boxes, classes = R.case("scene")
NDET, NLAB = len(dets), len(classes)
out = torch.from_numpy(dets).to(dev)
order, off = group_labels(classes, NC)
lab = torch.from_numpy(np.concatenate([classes[order, None], boxes[order]], 1)).to(dev)
cls_off = torch.from_numpy(off).to(dev)
num = torch.tensor([NDET], dtype=torch.int32, device=dev)
iouv = R.IOUV.float().to(dev)
tp = torch.zeros((NDET, 10), dtype=torch.uint8, device=dev)
code = torch.zeros(NDET, dtype=torch.uint8, device=dev)
cols = [torch.zeros(NDET, device=dev) for _ in range(6)]              # conf, pcls, ocls, s_iou, o_iou, a_iou
conf, pcls = torch.zeros(NDET, device=dev), torch.zeros(NDET, device=dev)
hists = torch.zeros((NC + 1) * 8 + (NC + 1) * (NC + 1) + NC * 12, dtype=torch.int64, device=dev)
det_hist, cm, lab_hist = hists[:(NC + 1) * 8], hists[(NC + 1) * 8:(NC + 1) * 8 + (NC + 1) ** 2], hists[(NC + 1) * 8 + (NC + 1) ** 2:]
state = torch.zeros(2, dtype=torch.int64, device=dev)
need = hip._Z()
hip.call("ryolo_scene_errors_workspace_bytes", NDET, NLAB, need)
ws_err = torch.empty(need.value, dtype=torch.uint8, device=dev)
hip.call("ryolo_scene_match_workspace_bytes", NDET, NLAB, need)
ws_match = torch.empty(need.value, dtype=torch.uint8, device=dev)


def prepare():
    state.zero_()
    hists.zero_()


def errors():
    hip.call("ryolo_scene_errors", hip.ptr(out), hip.ptr(num), NDET, hip.ptr(lab), hip.ptr(cls_off), NLAB, NC, 0.5, 0.1, 0.0, 32.0 ** 2, 96.0 ** 2,
             hip.ptr(code), *(hip.ptr(c) for c in cols), det_hist.data_ptr(), cm.data_ptr(), lab_hist.data_ptr(), NDET, state.data_ptr(),
             state.data_ptr() + 8, hip.ptr(ws_err), ws_err.numel(), hip.stream())


def match():
    hip.call("ryolo_scene_match", hip.ptr(out), hip.ptr(num), NDET, hip.ptr(lab), hip.ptr(cls_off), NLAB, NC, hip.ptr(iouv), 10, hip.ptr(tp),
             hip.ptr(conf), hip.ptr(pcls), NDET, state.data_ptr(), state.data_ptr() + 8, hip.ptr(ws_match), ws_match.numel(), hip.stream())


t_err, t_match = [], []
for _ in range(2):
    t_err.append(timed(prepare, errors))
    t_match.append(timed(prepare, match))
prepare()
match()
prepare()
errors()                                                              # the histograms of one scene
torch.cuda.synchronize()
spread = max(abs(t_err[0] - t_err[1]), abs(t_match[0] - t_match[1]))
res = {"device": torch.cuda.get_device_name(0), "detections": NDET, "labels": NLAB, "classes": NC, "reps": REPS,
       "codes": dict(zip(CODES, det_hist.view(NC + 1, 8).sum(0).tolist())), "statuses": dict(zip(STATUSES, lab_hist.view(NC, 3, 4).sum((0, 1)).tolist())),
       "tp_code_equals_scene_match": bool(torch.equal(code == 1, tp[:, 0] == 1)), "scene_errors_ms": [round(t, 4) for t in t_err],
       "scene_match_ms": [round(t, 4) for t in t_match], "spread_ms": round(spread, 4),
       "ratio_errors_over_match": round(min(t_err) / min(t_match), 2)}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
if not res["tp_code_equals_scene_match"]:
    sys.exit(1)
