"""Anchors fitted to a dataset on the device, and the labels no anchor reaches (csrc/anchors.hip).

The reference has no such stage: its nine anchors are constants of the model file (model/yolo.py:54-72), and a label that no anchor of
any scale passes in build_targets (lib/loss.py:297-298, :454-461) is dropped from training without a word.

    label_sizes(dataset_or_targets, img_size)   the (w, h) of every label in pixels of the network input
    fit_anchors(wh, k=9, ...)                   k-means start + (1 + C) evolution strategy, everything between the upload of the mutation
                                                table and the final read on the device -> AnchorFit
    anchor_report(targets, model, img_size)     per scale and in total: the target rows the loss can assign with the model's anchors

tests/anchor_ref.py restates the semantics in numpy.  CPU tensors raise; there is no host path.
"""
import numpy as np
import torch

from .. import hip
from ..engine import structs as S

_STRIDES = (8, 16, 32)
KMEANS_MAX_N = 1 << 24                                  # ryolo_argsort_desc's limit (the area order of the k-means start)
_DEFAULT_ANGLES = [-90, -60, -30, 0, 30, 60]            # data/hyp.yaml of the reference (synth.CFG)


def label_sizes(dataset_or_targets, img_size=None, return_dropped=False):
    """wh float32 [n, 2] on the device, in pixels of the network input: targets[:, 4:6] * img_size of a target tensor in the loss's layout,
    or of `dataset.label_table()` (img_size then defaults to the dataset's).  Rows whose w or h is not finite or not positive are removed
    and counted (the one host read); return_dropped: -> (wh, number of rows removed)."""
    src = dataset_or_targets
    if not isinstance(src, torch.Tensor):
        img_size = src.img_size if img_size is None else img_size
        src = src.label_table()
    hip.require_device(src, "label_sizes")
    if img_size is None:
        raise ValueError("label_sizes: img_size is needed to turn normalised targets into pixels")
    if src.dim() != 2 or src.shape[1] < 6:
        raise ValueError("label_sizes: expected targets [n, >= 6] = (item, cls, x, y, w, h, ...)")
    wh = src[:, 4:6].float() * float(img_size)
    ok = torch.isfinite(wh).all(1) & (wh > 0).all(1)
    wh = wh[ok].contiguous()                                   # boolean mask: the host read
    return (wh, int(src.shape[0] - wh.shape[0])) if return_dropped else wh


def mutation_table(seed, generations, children, k):
    """v float32 [G, C, K, 2], drawn once on the host from a private numpy Generator(PCG64(seed)).  Per child: mask = random((K, 2)) < 0.9,
    one uniform scale, standard normals; v = clip(mask * scale * normal * 0.1 + 1, 0.3, 3.0), redrawn while every entry is 1.  The draws
    never depend on the anchors, so the whole table exists before the first generation runs."""
    rng = np.random.Generator(np.random.PCG64(seed))
    v = np.ones((generations, children, k, 2), dtype=np.float64)
    for g in range(generations):
        for c in range(children):
            one = np.ones((k, 2))
            while (one == 1).all():
                mask = rng.random((k, 2)) < 0.9
                scale = rng.random()
                one = (mask * scale * rng.standard_normal((k, 2)) * 0.1 + 1.0).clip(0.3, 3.0)
            v[g, c] = one
    return v.astype(np.float32)


def _check_wh(wh, what):
    hip.require_device(wh, what)
    if wh.dtype != torch.float32 or wh.dim() != 2 or wh.shape[1] != 2 or wh.shape[0] < 1:
        raise ValueError(f"{what}: wh must be a float32 tensor [n >= 1, 2]")
    return wh.contiguous()


def _stats(st, n):
    """stats tensor (int64 [4] on the host; element 0 holds a double) -> dict."""
    return dict(fitness=float(st[:1].view(torch.float64)[0]), reached=int(st[1]), passes=int(st[2]), accepted=int(st[3]),
                bpr=int(st[1]) / n, aat=int(st[2]) / n)


def fitness_device(wh, k, thr=4.0):
    """-> stats int64 [4] on the device ([0] = the fitness, a double; reached labels; anchor passes; 0) of anchor set k [K, 2]."""
    wh = _check_wh(wh, "anchor_fitness")
    k = k.to(device=wh.device, dtype=torch.float32).reshape(-1, 2).contiguous()
    ws = hip.workspace("ryolo_anchor_workspace_bytes", wh.shape[0], device=wh.device)
    st = torch.empty(4, dtype=torch.int64, device=wh.device)
    hip.call("ryolo_anchor_fitness", hip.ptr(wh), wh.shape[0], hip.ptr(k), k.shape[0], float(thr), hip.ptr(ws), ws.numel(), hip.ptr(st), hip.stream())
    return st


def anchor_fitness(wh, k, thr=4.0):
    """dict(fitness, bpr, aat, reached, passes) of anchor set k on sizes wh (one host read)."""
    return _stats(fitness_device(wh, k, thr).cpu(), wh.shape[0])


def evolve_device(wh, k, v, thr=4.0):
    """(1 + C) evolution strategy from anchor set k [K, 2] with mutation table v [G, C, K, 2] (device tensors) -> (k, stats) on the device;
    no host read."""
    wh = _check_wh(wh, "anchor_evolve")
    hip.require_device(v, "anchor_evolve")
    k = k.to(device=wh.device, dtype=torch.float32).reshape(-1, 2).contiguous().clone()
    K = k.shape[0]
    if v.dtype != torch.float32 or v.dim() != 4 or v.shape[2] != K or v.shape[3] != 2 or not 1 <= v.shape[1] <= 16:
        raise ValueError("anchor_evolve: v must be float32 [G, 1 <= C <= 16, K, 2]")
    v = v.contiguous()
    ws = hip.workspace("ryolo_anchor_workspace_bytes", wh.shape[0], device=wh.device)
    st = torch.empty(4, dtype=torch.int64, device=wh.device)
    hip.call("ryolo_anchor_evolve", hip.ptr(wh), wh.shape[0], hip.ptr(k), K, hip.ptr(v) if v.shape[0] else None, v.shape[0], v.shape[1],
             float(thr), hip.ptr(ws), ws.numel(), hip.ptr(st), hip.stream())
    return k, st


def kmeans_device(wh, k, iters=30, start=None, want_assign=False):
    """Lloyd's k-means on (w, h) from the area-quantile start (or `start` [K, 2]) -> centroids [K, 2] on the device (and the int32
    assignment the last iteration made, None when iters == 0); no host read.  n <= 2^24."""
    wh = _check_wh(wh, "anchor_kmeans")
    n, dev = wh.shape[0], wh.device
    if n > KMEANS_MAX_N:
        raise ValueError(f"anchor_kmeans: {n} labels; the k-means start sorts the areas on the device and takes at most 2^24 = {KMEANS_MAX_N} "
                         "(subsample wh, or pass start= to fit_anchors: fitness and evolution take up to 2^31 - 1)")
    if start is None:
        cen = torch.empty((int(k), 2), dtype=torch.float32, device=dev)
    else:
        cen = start.to(device=dev, dtype=torch.float32).reshape(-1, 2).contiguous().clone()
    assign = torch.empty(n, dtype=torch.int32, device=dev) if want_assign and int(iters) > 0 else None      # (no iteration: no assignment)
    ws = hip.workspace("ryolo_anchor_kmeans_workspace_bytes", n, device=dev)
    hip.call("ryolo_anchor_kmeans", hip.ptr(wh), n, hip.ptr(cen), cen.shape[0], int(iters), 1 if start is None else 0, hip.ptr(assign),
             hip.ptr(ws), ws.numel(), hip.stream())
    return (cen, assign) if want_assign else cen


class AnchorFit:
    """Result of fit_anchors.  anchors: float32 numpy [K, 2], (w, h) in pixels of the network input, sorted by area; fitness / bpr / aat of
    the result and start_fitness / start_bpr / start_aat of the start (the k-means centroids, or `start`); accepted: generations whose
    best child replaced the parent; n: labels used."""

    def __init__(self, anchors, start, end, begin, n, thr):
        self.anchors, self.start_anchors, self.n, self.thr = anchors, start, n, thr
        self.fitness, self.bpr, self.aat, self.accepted = end["fitness"], end["bpr"], end["aat"], end["accepted"]
        self.start_fitness, self.start_bpr, self.start_aat = begin["fitness"], begin["bpr"], begin["aat"]

    def to_model_config(self, angles=None):
        """{"anchors": [[w, h, ...] x K / 3] x 3, "angles": angles} as Yolo(n_classes, model_config, mode, ver) takes it: the smallest third
        of the anchors goes to stride 8.  `angles` (degrees) pass through unchanged; None: the reference's six."""
        K = len(self.anchors)
        if K % 3:
            raise ValueError(f"to_model_config: {K} anchors do not split over 3 scales")
        per = K // 3
        rows = [[float(x) for a in self.anchors[i * per:(i + 1) * per] for x in a] for i in range(3)]
        return {"anchors": rows, "angles": list(_DEFAULT_ANGLES) if angles is None else angles}

    def __repr__(self):
        return "AnchorFit(K={}, n={}, fitness={:.4f} (start {:.4f}), bpr={:.4f} (start {:.4f}), aat={:.3f}, accepted={})".format(
            len(self.anchors), self.n, self.fitness, self.start_fitness, self.bpr, self.start_bpr, self.aat, self.accepted)


def _by_area(k):
    return k[np.argsort(k[:, 0] * k[:, 1], kind="stable")]


def fit_anchors(wh, k=9, thr=4.0, generations=1000, children=8, kmeans_iters=30, seed=0, start=None):
    """Fit k anchors to the sizes wh [n, 2] (label_sizes).  Start: `start` [k, 2] if given, else Lloyd's k-means from the area quantiles;
    then `generations` of a (1 + children) evolution strategy on the fitness (mean best side ratio of the labels within `thr`), mutation
    table from `seed`.  One upload (the table), one read (anchors and statistics) — the device decides every generation.  With start=None
    n is limited to 2^24 labels (the k-means start; ValueError beyond), with a start of the caller's to 2^31 - 1.  -> AnchorFit."""
    wh = _check_wh(wh, "fit_anchors")
    if not (1 <= int(k) <= 32 and 1 <= int(children) <= 16 and generations >= 0 and kmeans_iters >= 0 and float(thr) > 0):
        raise ValueError("fit_anchors: 1 <= k <= 32, 1 <= children <= 16, generations >= 0, kmeans_iters >= 0, thr > 0")
    dev = wh.device
    if start is None:
        k0 = kmeans_device(wh, int(k), kmeans_iters)
    else:
        k0 = torch.as_tensor(np.asarray(start, dtype=np.float32) if not isinstance(start, torch.Tensor) else start).to(dev).float().reshape(-1, 2)
        if k0.shape[0] != int(k):
            raise ValueError(f"fit_anchors: start has {k0.shape[0]} anchors, k = {k}")
    v = torch.from_numpy(mutation_table(seed, int(generations), int(children), int(k))).to(dev)
    st0 = fitness_device(wh, k0, thr)
    k1, st1 = evolve_device(wh, k0, v, thr)
    both = torch.cat([st0, st1, k0.reshape(-1).view(torch.int32).to(torch.int64), k1.reshape(-1).view(torch.int32).to(torch.int64)]).cpu()   # the one read
    n, m = wh.shape[0], 2 * int(k)
    a0 = both[8:8 + m].to(torch.int32).view(torch.float32).numpy().reshape(-1, 2)
    a1 = both[8 + m:8 + 2 * m].to(torch.int32).view(torch.float32).numpy().reshape(-1, 2)
    return AnchorFit(_by_area(a1), _by_area(a0), _stats(both[4:8], n), _stats(both[0:4], n), n, float(thr))


def reach_params(targets, anchors, gs, mode):
    """LossParams carrying what ryolo_anchor_reach reads: targets, anchors [3][na][2 | 3] in grid units, grid sizes, mode."""
    p = S.LossParams()
    p.mode, p.na = int(mode), len(anchors[0])
    p.nt = targets.shape[0]
    p.tcols = targets.shape[1] if targets.dim() == 2 else 0
    p.targets = targets.data_ptr() if p.nt else None
    for i in range(3):
        p.gs[i] = int(gs[i])
        if len(anchors[i]) != p.na or p.na > 18:
            raise ValueError("anchor_reach: every scale has the same number (<= 18) of anchors")
        for a, an in enumerate(anchors[i]):
            for j in range(len(an)):
                p.anchors[i][a][j] = float(an[j])
    return p


def anchor_reach(targets, anchors, gs, mode):
    """targets [nt, >= 7] in the loss's layout on the device -> (counts int32 [nt, 3]: anchors of each scale that pass the loss's rule for
    the row, summary int64 [5]: rows reached per scale, rows reached by no scale, anchor passes), both on the device."""
    hip.require_device(targets, "anchor_reach")
    S.check_layouts()
    targets = targets.float().contiguous()
    p = reach_params(targets, anchors, gs, mode)
    counts = torch.empty((p.nt, 3), dtype=torch.int32, device=targets.device)
    summary = torch.empty(5, dtype=torch.int64, device=targets.device)
    hip.call("ryolo_anchor_reach", p, hip.ptr(counts) if p.nt else None, hip.ptr(summary), hip.stream())
    return counts, summary


def anchor_report(targets, model, img_size):
    """Which rows of `targets` (loss layout, device) the loss can assign with `model`'s anchors at network size img_size: dict(rows,
    reached [3], reached_share [3], lost, lost_share, passes) — `lost` rows produce no target on any scale and are silently left out of
    training.  One host read.  The image index is not looked at."""
    if img_size % 32:
        raise ValueError("anchor_report: img_size must be a multiple of 32")
    mode = 0 if getattr(model, "mode", "kfiou") == "csl" else 1
    _, summary = anchor_reach(targets, model.anchors, [img_size // s for s in _STRIDES], mode)
    s = summary.tolist()
    nt = int(targets.shape[0])
    return dict(rows=nt, reached=s[:3], reached_share=[x / nt if nt else 0.0 for x in s[:3]], lost=s[3], lost_share=s[3] / nt if nt else 0.0,
                passes=s[4])
