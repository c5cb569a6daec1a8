"""CPU tests of tests/anchor_ref.py, the numpy restatement csrc/anchors.hip is checked against on the device: its reach rule against the
oracle's build_targets, fitness / bpr / aat on hand cases, the evolution strategy's invariants and the mutation table."""
import numpy as np
import pytest
import torch

from oracle import ref_ops
from ryolov4_amd.lib import anchors as product
from ryolov4_amd.model.yolo import Yolo
from ryolov4_amd.synth import CFG, synth_targets
from tests import anchor_ref as R

STRIDES = (8, 16, 32)


def _anchors(mode):
    if mode == "csl":
        return Yolo._make_anchors(STRIDES, CFG["anchors"])
    return Yolo._make_rotated_anchors(STRIDES, CFG["anchors"], [a * np.pi / 180 for a in CFG["angles"]])


def _hand_batch(S):
    """Rows sized to be lost (thinner than a quarter of the thinnest anchor, longer than four times the longest) among rows that are not."""
    rows = [[0, 1, 0.50, 0.50, 30 / S, 60 / S, 0.1],
            [0, 2, 0.30, 0.70, 2.5 / S, 40 / S, -0.4],          # w < 12 / 4
            [1, 0, 0.52, 0.11, 2.0 / S, 2.9 / S, 1.0],          # both sides tiny
            [1, 3, 0.25, 0.25, 100 / S, 1900 / S, 0.7],         # h > 4 * 401
            [1, 3, 0.75, 0.40, 16 / S, 16 / S, -1.2],
            [0, 5, 0.10, 0.90, 2000 / S, 2100 / S, 0.0]]        # both sides huge
    return torch.tensor(rows, dtype=torch.float32)


def _oracle_pairs(targets, anchors, gs, mode):
    res = ref_ops.build_targets([(g, g) for g in gs], targets, anchors, mode)
    # every (anchor, row) that passes the rule yields its centre-offset match; the neighbour offsets repeat pairs, never add one
    return [set(zip(r["a"].tolist(), r["tidx"].tolist())) for r in res]


@pytest.mark.parametrize("mode", ["csl", "kfiou"])
@pytest.mark.parametrize("case", ["synth64", "synth128", "hand"])
def test_reach_rule_is_build_targets(mode, case):
    S = 128 if case == "synth128" else 64
    if case == "hand":
        tg = _hand_batch(S)
    else:
        tg = synth_targets(3, 20, 16, False, seed=5 if S == 64 else 6, img_size=S, edge_cases=True)
    an = _anchors(mode)
    gs = [S // s for s in STRIDES]
    m = R.reach_mask(tg.numpy(), an, gs, 0 if mode == "csl" else 1)
    want = _oracle_pairs(tg, an, gs, mode)
    for i in range(3):
        got = set(zip(*[x.tolist() for x in np.nonzero(m[i])]))
        assert got == want[i], (mode, case, i)
    counts, summary = R.reach(tg.numpy(), an, gs, 0 if mode == "csl" else 1)
    for i in range(3):
        assert summary[i] == len({t for _, t in want[i]})
    lost = set(range(len(tg))) - {t for w in want for _, t in w}
    assert summary[3] == len(lost)
    assert summary[4] == sum(len(w) for w in want) == counts.sum()
    if case == "hand":
        assert {1, 2, 3, 5} <= lost and 0 not in lost


def test_fitness_hand_cases():
    k = R.REF_ANCHORS
    f, reached, passes = R.fitness(k[4:5], k)                  # a label equal to an anchor
    assert f == 1.0 and reached == 1 and passes >= 1
    one = np.array([[40.0, 28.0]], dtype=np.float32)
    f, reached, passes = R.fitness(one * np.float32(4.0001), one)
    assert f == 0.0 and reached == 0 and passes == 0           # bpr = aat = 0
    f, reached, passes = R.fitness(one * np.float32(3.9), one)
    assert reached == 1 and passes == 1 and abs(f - 1 / 3.9) < 1e-6
    # two labels, one out of reach: the mean runs over ALL labels
    f, reached, _ = R.fitness(np.concatenate([one, one * np.float32(5)]), one)
    assert f == 0.5 and reached == 1


def test_evolution_never_lowers_fitness_and_c1_is_the_sequential_loop():
    wh = R.lognormal_sizes(500)
    v = R.mutation_table(3, 25, 4, 9)
    trace = []
    k, (f, reached, passes), acc = R.evolve(wh, R.REF_ANCHORS, v, trace=trace)
    cur = [t[0] for t in trace] + [f]
    assert all(b >= a for a, b in zip(cur, cur[1:])) and f > cur[0]
    assert acc == sum(b > a for a, b in zip(cur, cur[1:])) > 0
    assert (f, reached, passes) == R.fitness(wh, k)
    assert (k >= 2.0).all()
    v1 = R.mutation_table(3, 40, 1, 9)
    ka, (fa, _, _), _ = R.evolve(wh, R.REF_ANCHORS, v1)
    kb, fb = R.evolve_sequential(wh, R.REF_ANCHORS, v1)
    assert np.array_equal(ka, kb) and fa == fb


def test_mutation_table_is_reproducible_and_matches_the_product():
    a, b = R.mutation_table(11, 6, 3, 9), R.mutation_table(11, 6, 3, 9)
    assert a.dtype == np.float32 and a.shape == (6, 3, 9, 2) and np.array_equal(a, b)
    assert not np.array_equal(a, R.mutation_table(12, 6, 3, 9))
    assert (a >= np.float32(0.3)).all() and (a <= np.float32(3.0)).all()
    assert not (a.reshape(18, -1) == 1).all(1).any()           # no child is the parent
    assert np.array_equal(a, product.mutation_table(11, 6, 3, 9))
    # the table of a longer run starts with the table of a shorter one only per generation block of equal C and K: same seed, same draws
    assert np.array_equal(R.mutation_table(11, 2, 3, 9), a[:2])


def test_kmeans_restatement():
    wh = R.lognormal_sizes(400, seed=9)
    k0 = R.kmeans_init(wh, 9)
    area = k0[:, 0] * k0[:, 1]
    assert (np.diff(area) >= 0).all()                          # quantiles of the area order
    k1, a1 = R.kmeans(wh, 9, 1)
    assert np.array_equal(a1, R.kmeans_assign(wh, k0))
    # Lloyd's iteration never raises the distortion
    def cost(k):
        return float(((wh[:, None, :].astype(np.float64) - k[None].astype(np.float64)) ** 2).sum(2).min(1).sum())
    k30, _ = R.kmeans(wh, 9, 30)
    assert cost(k30) <= cost(k1) <= cost(k0)
    # an empty cluster keeps its centroid
    far = np.concatenate([k0[:8], np.array([[1e6, 1e6]], dtype=np.float32)])
    kf, _ = R.kmeans(wh, 9, 2, start=far)
    assert np.array_equal(kf[8], far[8])


def test_product_refuses_cpu_tensors():
    wh = torch.from_numpy(R.lognormal_sizes(16))
    with pytest.raises(RuntimeError):
        product.fit_anchors(wh)
    with pytest.raises(RuntimeError):
        product.label_sizes(torch.zeros(4, 7), 64)
    with pytest.raises(RuntimeError):
        product.anchor_reach(torch.zeros(4, 7), _anchors("csl"), [8, 4, 2], 0)
