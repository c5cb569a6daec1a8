"""GPU tests of csrc/anchors.hip, lib/anchors.py and BaseDataset.label_table against tests/anchor_ref.py (numpy) and against the loss's own
target assignment (ryolo_loss_match_records of a real ryolo_loss call).

  reach      per-row counts and the integer summary equal the restatement; per scale the rows and (anchor, row) pair counts equal those of the
             loss's match records; no lost row appears in a record
  fitness    reached labels and anchor passes exact, fitness within 1e-12 relative (double sums in another order)
  evolution  final anchors bit-equal and the same number of accepted generations, after the restatement's gaps are shown to be 0 or > 1e-9
  k-means    first assignment exact, centroids after 1, 2, 30 iterations within 1e-6 relative
  dataset    label_table bit-equal to assemble_batch(augment=False)[:, :7]; generators untouched
  end to end label_sizes -> fit_anchors -> to_model_config -> Yolo; anchor_report; equal seeds give equal bits
"""
import random

import numpy as np
import pytest
import torch

from oracle import ref_ops
from ryolov4_amd.synth import CFG, HYP, synth_targets
from tests import anchor_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STRIDES = (8, 16, 32)
NS = (1, 255, 256, 257, 10007)
_WH = R.lognormal_sizes(max(NS), seed=7)               # shared, never modified
_KS = {3: R.REF_ANCHORS[[1, 4, 7]], 9: R.REF_ANCHORS, 18: np.concatenate([R.REF_ANCHORS, R.REF_ANCHORS[:, ::-1] * np.float32(0.7)])}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------- reach
class _Model:
    def __init__(self, mode, nc):
        self.anchors, self.nc, self.mode = ref_ops.make_anchors(CFG, mode), nc, mode


def _reach_targets(nt, S, csl):
    if nt == 0:
        return torch.zeros((0, 187 if csl else 7))
    tg = synth_targets(1, nt, 2, csl, seed=5 + nt + S, img_size=S, edge_cases=nt > 2)
    if nt >= 64:
        for j, (w, h) in enumerate([(2.5, 40.0), (2.0, 2.9), (100.0, 1900.0), (2000.0, 2100.0), (1.0, 300.0)]):
            tg[7 + 11 * j, 4], tg[7 + 11 * j, 5] = w / S, h / S                # thinner than 12 / 4 px or longer than 4 * 401 px: lost
    return tg


@pytest.mark.parametrize("mode", ["csl", "kfiou"])
@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("nt", [0, 1, 257])
def test_reach_equals_restatement_and_loss_records(nt, S, mode):
    from ryolov4_amd.lib import anchors as An
    from ryolov4_amd.lib import loss as L
    csl = mode == "csl"
    nc = 2
    model = _Model(mode, nc)
    tg = _reach_targets(nt, S, csl)
    gs = [S // s for s in STRIDES]
    m = 0 if csl else 1
    if not csl and nt:                                                             # the restatement's cosine is numpy's, the kernel's the device's
        an = np.asarray(model.anchors[0], dtype=np.float32)[:, 2]
        c = np.abs(np.cos(tg[:, 6:7].numpy() - an[None, :]))
        assert (np.abs(c - 0.866) > 1e-5).all(), "a target angle sits on the 30 degree threshold: change the seed"
    want_counts, want_sum = R.reach(tg.numpy(), model.anchors, gs, m)
    counts, summary = An.anchor_reach(tg.to(DEV), model.anchors, gs, m)
    counts, summary = counts.cpu().numpy(), summary.cpu().numpy()
    print(nt, S, mode, "summary", summary.tolist())
    assert np.array_equal(summary, want_sum)
    assert counts.shape == (nt, 3) and np.array_equal(counts, want_counts)
    if nt == 257:
        assert summary[3] >= 5 and summary[:3].min() > 0                            # some rows are lost, every scale reaches some
    rep = An.anchor_report(tg.to(DEV), model, S)
    assert rep["rows"] == nt and rep["reached"] == summary[:3].tolist() and rep["lost"] == summary[3] and rep["passes"] == summary[4]
    assert rep["lost_share"] == (summary[3] / nt if nt else 0.0)
    # the loss itself, on the same targets
    crit = (L.ComputeCSLLoss if csl else L.ComputeKFIoULoss)(model, HYP)
    g = torch.Generator().manual_seed(3)
    na, attrs = len(model.anchors[0]), nc + (185 if csl else 6)
    outs = [torch.randn(1, na, x, x, attrs, generator=g).to(DEV) for x in gs]
    crit(outs, tg.to(DEV))
    recs = crit.debug_matches()
    lost = set(np.nonzero(counts.sum(1) == 0)[0].tolist()) if nt else set()
    for i in range(3):
        pairs = {(int(r[1]), int(r[5])) for r in recs[i]}
        per_row = np.zeros(nt, dtype=np.int64)
        for _, t in pairs:
            per_row[t] += 1
        assert np.array_equal(per_row, counts[:, i] if nt else per_row), i             # anchors per row
        assert len({t for _, t in pairs}) == summary[i]                             # distinct rows = reached
        assert not ({t for _, t in pairs} & lost)
    assert sum(len({(int(r[1]), int(r[5])) for r in recs[i]}) for i in range(3)) == summary[4]


def test_reach_bad_arguments():
    from ryolov4_amd import hip
    from ryolov4_amd.lib import anchors as An
    model = _Model("kfiou", 2)
    tg = _reach_targets(4, 64, False).to(DEV)
    counts = torch.empty((4, 3), dtype=torch.int32, device=DEV)
    summary = torch.empty(5, dtype=torch.int64, device=DEV)
    for edit in ("mode", "na", "gs", "tcols"):
        p = An.reach_params(tg, model.anchors, [8, 4, 2], 1)
        if edit == "mode":
            p.mode = 6
        elif edit == "na":
            p.na = 19
        elif edit == "gs":
            p.gs[1] = 0
        else:
            p.tcols = 6
        with pytest.raises(RuntimeError, match="invalid argument"):
            hip.call("ryolo_anchor_reach", p, hip.ptr(counts), hip.ptr(summary), hip.stream())
    with pytest.raises(RuntimeError):
        An.anchor_reach(tg.cpu(), model.anchors, [8, 4, 2], 1)


# ---------------------------------------------------------------------------------------------- fitness
@pytest.mark.parametrize("K", sorted(_KS))
@pytest.mark.parametrize("n", NS)
def test_fitness_counts_exact_sum_to_rounding(n, K):
    from ryolov4_amd.lib import anchors as An
    wh, k = _WH[:n], _KS[K]
    f, reached, passes = R.fitness(wh, k)
    got = An.anchor_fitness(_dev(wh), _dev(k))
    print(n, K, got, f)
    assert got["reached"] == reached and got["passes"] == passes
    assert got["bpr"] == reached / n and got["aat"] == passes / n
    assert abs(got["fitness"] - f) <= 1e-12 * abs(f)


def test_fitness_hand_cases_and_bad_arguments():
    from ryolov4_amd import hip
    from ryolov4_amd.lib import anchors as An
    one = np.array([[40.0, 28.0]], dtype=np.float32)
    got = An.anchor_fitness(_dev(one), _dev(one))
    assert got["fitness"] == 1.0 and got["bpr"] == 1.0 and got["aat"] == 1.0
    got = An.anchor_fitness(_dev(one * np.float32(4.0001)), _dev(one))
    assert got["fitness"] == 0.0 and got["bpr"] == 0.0 and got["aat"] == 0.0
    wh, k = _dev(_WH[:16]), _dev(R.REF_ANCHORS)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    st = torch.empty(4, dtype=torch.int64, device=DEV)
    v = torch.ones((1, 17, 9, 2), dtype=torch.float32, device=DEV)
    bad = [("ryolo_anchor_fitness", (hip.ptr(wh), 16, hip.ptr(k), 33, 4.0, hip.ptr(ws), ws.numel(), hip.ptr(st), hip.stream())),
           ("ryolo_anchor_fitness", (hip.ptr(wh), 0, hip.ptr(k), 9, 4.0, hip.ptr(ws), ws.numel(), hip.ptr(st), hip.stream())),
           ("ryolo_anchor_fitness", (hip.ptr(wh), 16, hip.ptr(k), 9, 0.0, hip.ptr(ws), ws.numel(), hip.ptr(st), hip.stream())),
           ("ryolo_anchor_fitness", (hip.ptr(wh), 16, hip.ptr(k), 9, 4.0, hip.ptr(ws), 64, hip.ptr(st), hip.stream())),
           ("ryolo_anchor_evolve", (hip.ptr(wh), 16, hip.ptr(k), 9, hip.ptr(v), 1, 17, 4.0, hip.ptr(ws), ws.numel(), hip.ptr(st), hip.stream())),
           ("ryolo_anchor_evolve", (hip.ptr(wh), 16, hip.ptr(k), 9, hip.ptr(v), 1, 0, 4.0, hip.ptr(ws), ws.numel(), hip.ptr(st), hip.stream())),
           ("ryolo_anchor_kmeans", (hip.ptr(wh), 16, hip.ptr(k), 33, 1, 1, None, hip.ptr(ws), ws.numel(), hip.stream())),
           ("ryolo_anchor_kmeans", (hip.ptr(wh), 16, hip.ptr(k), 9, -1, 1, None, hip.ptr(ws), ws.numel(), hip.stream()))]
    for name, args in bad:
        with pytest.raises(RuntimeError, match="workspace too small" if args[-4:-2] == (hip.ptr(ws), 64) else "invalid argument"):
            hip.call(name, *args)


# ---------------------------------------------------------------------------------------------- evolution
_EVO = {}


def _evo_ref(n, C):
    """The restatement's run from the reference anchors with table seed 3, G = 40; computed once per case and never modified."""
    if (n, C) not in _EVO:
        v = R.mutation_table(3, 40, C, 9)
        trace = []
        k, stats, acc = R.evolve(_WH[:n], R.REF_ANCHORS, v, trace=trace)
        _EVO[(n, C)] = (v, k, stats, acc, R.gaps(trace))
    return _EVO[(n, C)]


@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("n", NS)
def test_evolution_bit_equal_to_restatement(n, C):
    from ryolov4_amd.lib import anchors as An
    v, k_ref, (f, reached, passes), acc, gaps = _evo_ref(n, C)
    nz = gaps[gaps != 0]
    print(n, C, "accepted", acc, "smallest nonzero gap", nz.min() if len(nz) else None)
    assert ((gaps == 0) | (gaps > 1e-9)).all(), "a decision of the restatement hangs on the order of a double sum: change the seed"
    k, st = An.evolve_device(_dev(_WH[:n]), _dev(R.REF_ANCHORS), _dev(v))
    got = An._stats(st.cpu(), n)
    assert k.cpu().numpy().tobytes() == k_ref.tobytes()
    assert got["accepted"] == acc and got["reached"] == reached and got["passes"] == passes
    assert abs(got["fitness"] - f) <= 1e-12 * abs(f)
    if n >= 255:
        assert acc > 0                                                              # the case exercises the accept path


# ---------------------------------------------------------------------------------------------- k-means
@pytest.mark.parametrize("n", [257, 10007])
def test_kmeans_against_restatement(n):
    from ryolov4_amd.lib import anchors as An
    wh = _WH[:n]
    dwh = _dev(wh)
    k0, none = An.kmeans_device(dwh, 9, 0, want_assign=True)                        # no iteration: the start, and no assignment
    assert none is None
    k0 = k0.cpu().numpy()
    assert k0.tobytes() == R.kmeans_init(wh, 9).tobytes()                           # the quantile start: labels, bit for bit
    for iters in (1, 2, 30):
        want, _ = R.kmeans(wh, 9, iters)
        got, assign = An.kmeans_device(dwh, 9, iters, want_assign=True)
        got = got.cpu().numpy()
        err = np.abs(got.astype(np.float64) - want) / np.abs(want)
        print(n, iters, "max relative centroid error", err.max())
        if iters == 1:
            assert np.array_equal(assign.cpu().numpy(), R.kmeans_assign(wh, k0))
        assert err.max() <= 1e-6
    # a start of the caller's; an empty cluster keeps its centroid
    far = np.concatenate([k0[:8], np.array([[1e6, 1e6]], dtype=np.float32)])
    got = An.kmeans_device(dwh, 9, 2, start=_dev(far)).cpu().numpy()
    want, _ = R.kmeans(wh, 9, 2, start=far)
    assert got[8].tobytes() == far[8].tobytes() and (np.abs(got.astype(np.float64) - want) <= 1e-6 * np.abs(want)).all()


# ---------------------------------------------------------------------------------------------- dataset path
AUG = dict(mosaic=1.0, mixup=0.5, hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, rotate=10.0, scale=0.3, translate=0.1, fliplr=0.5, flipud=0.3)


def _rot_rects(rs, n, W, H, lo, hi):
    cx, cy = rs.uniform(0, W, n), rs.uniform(0, H, n)
    w, h, a = rs.uniform(lo, hi, n), rs.uniform(lo, hi, n), rs.uniform(0, np.pi, n)
    ux, uy = np.cos(a) * w / 2, np.sin(a) * w / 2
    vx, vy = -np.sin(a) * h / 2, np.cos(a) * h / 2
    return np.stack([cx - ux - vx, cy - uy - vy, cx + ux - vx, cy + uy - vy, cx + ux + vx, cy + uy + vy, cx - ux + vx, cy - uy + vy], 1).astype(np.float32)


def _arrays(shapes, per, seed, lo=3, hi=60):
    rs = np.random.RandomState(seed)
    imgs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in shapes]
    polys = [_rot_rects(rs, per, w, h, lo, hi) for h, w in shapes]
    labels = [rs.randint(0, 3, size=per).astype(np.float32) for _ in shapes]
    return imgs, polys, labels


IMG_SHAPES = ((96, 160), (128, 128), (160, 97), (111, 150), (101, 99), (155, 131))


def _expect(twin, idx):
    tg = twin.assemble_batch(idx)[2][:, :7].clone()
    tg[:, 0] = torch.tensor(idx, dtype=torch.float32, device=tg.device)[tg[:, 0].long()]
    return tg


@pytest.mark.parametrize("csl", [True, False])
def test_label_table_equals_plain_batch(csl):
    from ryolov4_amd.datasets.base_dataset import BaseDataset
    arrays = _arrays(IMG_SHAPES, 14, 21)
    rng = (random.Random(1), np.random.RandomState(2))
    ds = BaseDataset(AUG, 128, True, csl, False, device=DEV, rng=rng)
    ds.set_arrays(*arrays)
    twin = BaseDataset(AUG, 128, False, csl, False, device=DEV)
    twin.set_arrays(*arrays)
    before = (rng[0].getstate(), rng[1].get_state()[1].tobytes(), rng[1].get_state()[2:])
    got = ds.label_table()
    after = (rng[0].getstate(), rng[1].get_state()[1].tobytes(), rng[1].get_state()[2:])
    assert before == after
    want = _expect(twin, list(range(6)))
    assert got.dtype == torch.float32 and got.shape == want.shape and got.shape[0] > 40
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    idx = [4, 1, 5]
    assert ds.label_table(idx, chunk=2).cpu().numpy().tobytes() == _expect(twin, idx).cpu().numpy().tobytes()
    assert ds.label_table([]).shape == (0, 7)
    for bad in (0, -3):
        with pytest.raises(ValueError):
            ds.label_table(idx, chunk=bad)
    assert twin.label_table().cpu().numpy().tobytes() == want.cpu().numpy().tobytes()


def test_label_table_of_scene_windows():
    from ryolov4_amd.datasets.scene_dataset import SceneDataset
    arrays = _arrays(((300, 300), (300, 300)), 60, 22)
    rng = (random.Random(1), np.random.RandomState(2))
    ds = SceneDataset(AUG, 128, True, False, device=DEV, rng=rng, overlap=16, window_seed=4)
    ds.set_arrays(*arrays)
    twin = SceneDataset(AUG, 128, False, False, device=DEV, overlap=16)
    twin.set_arrays(*arrays)
    assert ds.jitter and not twin.jitter and len(ds) == len(twin) > 8
    ds.last_windows, ds._row_wins = ["kept"], ["kept"]
    before = (rng[0].getstate(), rng[1].get_state()[1].tobytes(), ds._wrng.getstate())
    got = ds.label_table(chunk=5)
    assert before == (rng[0].getstate(), rng[1].get_state()[1].tobytes(), ds._wrng.getstate())
    assert ds.jitter and ds.last_windows == ["kept"] and ds._row_wins == ["kept"]
    want = _expect(twin, list(range(len(twin))))
    assert got.shape == want.shape and got.shape[0] > 60 and got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------- end to end
def test_fit_from_a_dataset_end_to_end():
    from ryolov4_amd.datasets.base_dataset import BaseDataset
    from ryolov4_amd.lib import anchors as An
    from ryolov4_amd.model.yolo import Yolo
    S = 128
    ds = BaseDataset(AUG, S, False, False, False, device=DEV)
    ds.set_arrays(*_arrays(IMG_SHAPES, 30, 23, lo=2, hi=70))
    table = ds.label_table()
    wh, dropped = An.label_sizes(ds, return_dropped=True)
    assert dropped == 0 and wh.shape == (table.shape[0], 2) and wh.shape[0] > 100
    assert torch.equal(wh, table[:, 4:6] * float(S))
    bad = table.clone()
    bad[3, 4], bad[5, 5], bad[9, 4] = float("nan"), 0.0, float("inf")
    wh_bad, dropped = An.label_sizes(bad, S, return_dropped=True)
    assert dropped == 3 and wh_bad.shape[0] == wh.shape[0] - 3
    fit = An.fit_anchors(wh, generations=60, children=4, seed=1)
    print(fit)
    assert fit.anchors.shape == (9, 2) and (np.diff(fit.anchors[:, 0] * fit.anchors[:, 1]) >= 0).all()
    assert fit.fitness >= fit.start_fitness and fit.bpr >= fit.start_bpr
    chk = An.anchor_fitness(wh, torch.from_numpy(fit.anchors).to(DEV))
    assert chk["fitness"] == fit.fitness and chk["bpr"] == fit.bpr and chk["aat"] == fit.aat
    again = An.fit_anchors(wh, generations=60, children=4, seed=1)
    assert again.anchors.tobytes() == fit.anchors.tobytes() and again.fitness == fit.fitness and again.accepted == fit.accepted
    from_ref = An.fit_anchors(wh, generations=60, children=4, seed=1, start=R.REF_ANCHORS)
    ref_stats = An.anchor_fitness(wh, torch.from_numpy(R.REF_ANCHORS).to(DEV))
    assert from_ref.start_fitness == ref_stats["fitness"] and from_ref.fitness >= from_ref.start_fitness
    cfg = fit.to_model_config()
    assert [len(r) for r in cfg["anchors"]] == [6, 6, 6] and cfg["angles"] == CFG["angles"]
    assert fit.to_model_config(angles=[0, 45])["angles"] == [0, 45]
    fitted, reference = Yolo(3, cfg, "csl", "yolov7"), Yolo(3, CFG, "csl", "yolov7")
    rep_fit, rep_ref = An.anchor_report(table, fitted, S), An.anchor_report(table, reference, S)
    print("fitted", rep_fit, "reference", rep_ref)
    assert rep_fit["rows"] == rep_ref["rows"] == table.shape[0]
    assert rep_ref["lost"] > 0 and rep_fit["lost"] <= rep_ref["lost"]
