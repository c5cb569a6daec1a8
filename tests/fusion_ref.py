"""Host restatement of the cluster fusion of the full-scene merge (include/ryolo.h ryolo_nms_owner / ryolo_tile_fuse, lib/tiled.py
fuse="box" | "wbf"), written from the definition, not from the kernels: numpy scalars of one dtype, one operation per step, members in
ascending sorted position with the owner first.  Owners come from the greedy pass over oracle.nms_mask (the smallest kept row whose bit
is set), and the keep set that pass produces is asserted equal to oracle.nms_rotated's.  The dtype is a parameter so that the float64
run of the same formulas can guard the fp32 one (tests/test_tiled_fusion_cpu.py)."""
import numpy as np

import oracle
from tests import views_ref as V

f32 = np.float32
MODES = ("box", "wbf")


# The synthetic merge scenes shared by the CPU and the GPU tests: tests.test_gpu_tiled_views._synth_dets over the entries of a
# 250 x 300 scene.  (nc, rates, views, seed, thr, max_nms, max_det)
SH, SW, S, OV, B, MK = 250, 300, 128, 32, 4, 24
CONFIGS = (
    (3, (1.0,), V.NAMES, 1, 0.3, 5000, 5000),
    (3, (1.0, 0.5), ("rot270", "id", "hflip"), 2, 0.3, 5000, 5000),
    (3, (1.0,), V.NAMES, 3, 0.3, 9, 13),
    (1, (1.0,), V.NAMES, 4, 0.1, 5000, 5000),
    (3, (1.0,), V.NAMES, 5, 0.1, 5000, 5000),
)
_SCENES = {}


def scene(i):
    """-> (entries, dets, nums) of CONFIGS[i], built once."""
    if i not in _SCENES:
        from ryolov4_amd.lib import tiled
        from tests.test_gpu_tiled_views import _synth_dets
        nc, rates, views, seed = CONFIGS[i][:4]
        entries = tiled.tile_entries(SH, SW, S, OV, rates, views)
        e_pad = -(-len(entries) // B) * B
        dets, nums = _synth_dets(entries, e_pad, MK, nc, S, seed)
        dets.setflags(write=False)
        nums.setflags(write=False)
        _SCENES[i] = (entries, dets, nums)
    return _SCENES[i]


def owners_from_mask(mask, n):
    """mask [n, ceil(n / 64)] uint64 (bit (k, p), p > k: k suppresses p) -> (owner [n] int64, keep list): the greedy pass.  owner[p] = p
    for a kept p, otherwise the smallest kept k < p with bit (k, p) set."""
    owner = np.full(n, -1, dtype=np.int64)
    keep = []
    for p in range(n):
        if owner[p] >= 0:
            continue
        owner[p] = p
        keep.append(p)
        bits = np.unpackbits(np.ascontiguousarray(mask[p]).view(np.uint8), bitorder="little")[:n].astype(bool)
        bits[:p + 1] = False
        owner[bits & (owner < 0)] = p
    return owner, keep


def fuse_cluster(rows, mode, n_ens, ft=f32, stats=None):
    """rows [m, >= 6] (x, y, w, h, theta, s, ...), the owner first, then the members in ascending position -> (x, y, w, h, theta, score) as
    scalars of dtype `ft`.  A single row comes back unchanged (theta unwrapped); its score follows the mode."""
    PI, HALF_PI, QUARTER_PI = ft(f32(np.pi)), ft(f32(np.pi / 2)), ft(f32(np.pi / 4))
    r = np.asarray(rows)
    xk, yk, wk, hk, tk, sk = (ft(v) for v in r[0, :6])
    m = 1
    W, ax, ay, aw, ah, ad = sk, ft(0), ft(0), sk * wk, sk * hk, ft(0)
    for i in range(1, len(r)):
        xi, yi, wi, hi, ti, si = (ft(v) for v in r[i, :6])
        d = ti - tk
        if d >= HALF_PI:
            d = d - PI
            _count(stats, "wraps")
        if d < -HALF_PI:
            d = d + PI
            _count(stats, "wraps")
        if d > QUARTER_PI:
            wi, hi = hi, wi
            d = d - HALF_PI
            _count(stats, "swaps")
        elif d < -QUARTER_PI:
            wi, hi = hi, wi
            d = d + HALF_PI
            _count(stats, "swaps")
        W = W + si
        ax = ax + si * (xi - xk)
        ay = ay + si * (yi - yk)
        aw = aw + si * wi
        ah = ah + si * hi
        ad = ad + si * d
        m = m + 1
    if m == 1:
        x, y, w, h, t = xk, yk, wk, hk, tk
    else:
        x = xk + ax / W
        y = yk + ay / W
        w = aw / W
        h = ah / W
        t = tk + ad / W
        if t >= HALF_PI:
            t = t - PI
            _count(stats, "wraps")
        if t < -HALF_PI:
            t = t + PI
            _count(stats, "wraps")
    if mode == "box":
        s = sk
    elif mode == "wbf":
        s = (W / ft(m)) * (ft(min(m, n_ens)) / ft(n_ens))
    else:
        raise ValueError(mode)
    out = (x, y, w, h, t, s)
    assert all(type(v) is ft for v in out), [type(v) for v in out]
    return out


def _count(stats, name, k=1):
    if stats is not None:
        stats[name] = stats.get(name, 0) + k


def candidates(entries, rates, S, dets, nums, mk):
    """views_ref.oracle_merge's first half: every entry's rows through the inverse view map and the fp32 shift -> (rows [N, 7], slots [N])."""
    rows, slots = [], []
    for e, (ri, x0, y0, name) in enumerate(entries):
        n = int(nums[e])
        if n:
            rows.append(V.shift_rows(V.map_rows(dets[e, :n], name, S), x0, y0, rates[ri]))
            slots.extend(e * mk + j for j in range(n))
    rows = np.concatenate(rows).astype(f32) if rows else np.zeros((0, 7), f32)
    return rows, np.array(slots, dtype=np.int64)


def class_clusters(rows, slots, c, thr, gt, max_nms):
    """-> (o, owner, keep): o the candidate indices of class c in (score desc, slot asc) order capped at max_nms, owner / keep in positions
    of that order."""
    idx = np.nonzero(rows[:, 6] == c)[0]
    o = np.array(sorted(idx, key=lambda i: (-rows[i, 5], slots[i]))[:max_nms], dtype=np.int64)
    if len(o) == 0:
        return o, np.zeros(0, np.int64), []
    b = rows[o, :5].copy()
    b[:, 4] = b[:, 4] / f32(np.pi) * f32(180.0)
    owner, keep = owners_from_mask(oracle.nms_mask(b, thr, gt), len(o))
    assert np.array_equal(np.array(keep, dtype=np.int64), oracle.nms_rotated(b, rows[o, 5], thr, gt)), "greedy pass over the mask != oracle NMS"
    return o, owner, keep


def fused_merge(entries, rates, S, dets, nums, mk, nc, thr, gt, max_nms, max_det, mode, n_ens=None, ft=f32, stats=None):
    """views_ref.oracle_merge with cluster fusion: the same candidates, order and NMS; every kept box absorbs the positions it owns; final
    order (fused score desc, owner's slot asc) capped at max_det -> rows [n, 7] of dtype ft.  n_ens defaults to len(rates) * the number
    of distinct views among the entries.  stats (a dict) receives cluster sizes, wrap / swap counts and candidates per class."""
    assert mode in MODES
    if n_ens is None:
        n_ens = len(rates) * len({e[3] for e in entries})
    rows, slots = candidates(entries, rates, S, dets, nums, mk)
    res = []
    for c in range(nc):
        o, owner, keep = class_clusters(rows, slots, c, thr, gt, max_nms)
        if stats is not None:
            stats.setdefault("per_class", []).append(len(o))
        for k in keep:
            members = np.nonzero(owner == k)[0]
            assert members[0] == k and (np.diff(members) > 0).all()
            if stats is not None:
                stats.setdefault("sizes", []).append(len(members))
            x, y, w, h, t, s = fuse_cluster(rows[o[members]], mode, n_ens, ft, stats)
            res.append((s, slots[o[k]], np.array([x, y, w, h, t, s, ft(rows[o[k], 6])], dtype=ft), len(members)))
    res.sort(key=lambda r: (-r[0], r[1]))
    out = [r[2] for r in res[:max_det]]
    if stats is not None:
        stats["out_sizes"] = [r[3] for r in res[:max_det]]                     # cluster size of every output row
    return np.stack(out).reshape(-1, 7) if out else np.zeros((0, 7), ft)
