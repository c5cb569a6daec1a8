"""numpy restatement of csrc/anchors.hip, written for this build — the reference has no anchor fitting and no reach report.

Float32 where the kernels are float32 (side ratios, mutation products, squared distances), float64 sums, integer counts.  The sums here run in
numpy's order, the device's in its own fixed order: fitness values agree to rounding of a double sum, every count and every float32 result exactly.
"""
import numpy as np

F = np.float32
REF_ANCHORS = np.array([[12, 16], [19, 36], [40, 28], [36, 75], [76, 55], [72, 146], [142, 110], [192, 243], [459, 401]], dtype=np.float32)


# ------------------------------------------------------------------------------------------------ reach
def reach_mask(targets, anchors, gs, mode):
    """targets [nt, >= 7] normalised (loss layout), anchors [3][na][2 | 3] in grid units, gs [3] -> bool [3, na, nt]: anchor a of scale i
    passes the loss's rule for row t (csrc/loss.hip cand_test, offset 0; the image index is not looked at)."""
    tg = np.asarray(targets, dtype=F).reshape(-1, np.shape(targets)[1] if np.ndim(targets) == 2 else 7)
    nt = len(tg)
    na = len(anchors[0])
    out = np.zeros((3, na, nt), dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(3):
            fg = F(gs[i])
            gw, gh = tg[:, 4] * fg, tg[:, 5] * fg
            for a in range(na):
                an = anchors[i][a]
                rw, rh = gw / F(an[0]), gh / F(an[1])
                mw, mh = np.fmax(rw, F(1) / rw), np.fmax(rh, F(1) / rh)
                ok = np.fmax(mw, mh) < F(4)
                if mode != 0:
                    ok &= np.abs(np.cos((tg[:, 6] - F(an[2])).astype(F), dtype=F)) > F(0.866)
                out[i, a] = ok
    return out


def reach(targets, anchors, gs, mode):
    """-> (counts int32 [nt, 3], summary int64 [5] = rows reached per scale, lost rows, anchor passes)."""
    m = reach_mask(targets, anchors, gs, mode)
    counts = m.sum(1).T.astype(np.int32).reshape(-1, 3)
    got = counts > 0
    summary = np.array([got[:, 0].sum(), got[:, 1].sum(), got[:, 2].sum(), (~got.any(1)).sum(), counts.sum()], dtype=np.int64)
    return counts, summary


# ------------------------------------------------------------------------------------------------ fitness
def best_ratio(wh, k):
    """-> (x float32 [n], m float32 [n, K]): per (label, anchor) m = min(min(rw, 1 / rw), min(rh, 1 / rh)), x = max over anchors."""
    wh, k = np.asarray(wh, dtype=F).reshape(-1, 2), np.asarray(k, dtype=F).reshape(-1, 2)
    r = wh[:, None, :] / k[None, :, :]
    m = np.minimum(r, F(1) / r).min(2)
    return m.max(1), m


def fitness(wh, k, thr=4.0):
    """-> (fitness float64, reached int, passes int); bpr = reached / n, aat = passes / n."""
    inv = F(1.0 / thr)
    x, m = best_ratio(wh, k)
    hit = x > inv
    return float(x[hit].astype(np.float64).sum() / len(x)), int(hit.sum()), int((m > inv).sum())


# ------------------------------------------------------------------------------------------------ evolution
def mutation_table(seed, G, C, K):
    """v float32 [G, C, K, 2] from a private Generator(PCG64(seed)); per child: mask = random < 0.9, one uniform scale, standard normals,
    v = clip(mask * scale * normal * 0.1 + 1, 0.3, 3.0), redrawn while all ones.  The draws never depend on the anchors."""
    rng = np.random.Generator(np.random.PCG64(seed))
    v = np.ones((G, C, K, 2), dtype=np.float64)
    for g in range(G):
        for c in range(C):
            one = np.ones((K, 2))
            while (one == 1).all():
                mask = rng.random((K, 2)) < 0.9
                scale = rng.random()
                one = (mask * scale * rng.standard_normal((K, 2)) * 0.1 + 1.0).clip(0.3, 3.0)
            v[g, c] = one
    return v.astype(F)


def children(k, vg):
    """max(k * v[g][c], 2.0f) in float32: [C, K, 2]."""
    return np.maximum(np.asarray(k, dtype=F)[None] * np.asarray(vg, dtype=F), F(2.0))


def evolve(wh, k, v, thr=4.0, trace=None):
    """(1 + C) evolution strategy.  -> (k float32 [K, 2], (fitness, reached, passes), accepted generations).  trace (a list): per generation
    (fitness of k before, sorted child fitnesses descending) for the gap precondition of the device test."""
    k = np.asarray(k, dtype=F).reshape(-1, 2).copy()
    cur = fitness(wh, k, thr)
    accepted = 0
    for vg in v:
        kids = children(k, vg)
        sc = [fitness(wh, kid, thr) for kid in kids]
        fits = np.array([s[0] for s in sc])
        best = int(np.argmax(fits))                    # first maximum: lowest c among equals
        if trace is not None:
            trace.append((cur[0], np.sort(fits)[::-1]))
        if fits[best] > cur[0]:
            k, cur, accepted = kids[best], sc[best], accepted + 1
    return k, cur, accepted


def evolve_sequential(wh, k, v, thr=4.0):
    """The classic auto-anchor loop (C = 1), written as a plain loop over v [G, 1, K, 2]."""
    k = np.asarray(k, dtype=F).reshape(-1, 2).copy()
    f = fitness(wh, k, thr)[0]
    for g in range(len(v)):
        kg = np.maximum(k * v[g, 0], F(2.0))
        fg = fitness(wh, kg, thr)[0]
        if fg > f:
            f, k = fg, kg
    return k, f


def gaps(trace):
    """Every accept / reject gap and every best-versus-second-child gap of a trace, as absolute values."""
    out = []
    for cur, fits in trace:
        out.append(abs(fits[0] - cur))
        if len(fits) > 1:
            out.append(abs(fits[0] - fits[1]))
    return np.array(out)


# ------------------------------------------------------------------------------------------------ k-means start
def kmeans_init(wh, K):
    """The labels at ranks floor((j + 0.5) / K * n) of the labels in ascending area order, the order being the stable DESCENDING argsort
    (key descending, index ascending) read backwards."""
    wh = np.asarray(wh, dtype=F).reshape(-1, 2)
    n = len(wh)
    area = wh[:, 0] * wh[:, 1]
    order = np.argsort(-area, kind="stable")
    q = [min(n - 1, ((2 * j + 1) * n) // (2 * K)) for j in range(K)]
    return wh[order[[n - 1 - x for x in q]]].copy()


def kmeans_assign(wh, k):
    wh, k = np.asarray(wh, dtype=F).reshape(-1, 2), np.asarray(k, dtype=F).reshape(-1, 2)
    d = wh[:, None, :] - k[None, :, :]
    d0, d1 = d[..., 0] * d[..., 0], d[..., 1] * d[..., 1]
    return np.argmin(d0 + d1, axis=1).astype(np.int32)          # first minimum: lowest centroid among equals


def kmeans(wh, K, iters=30, start=None):
    """-> (k float32 [K, 2], assignment of the last iteration int32 [n])."""
    wh = np.asarray(wh, dtype=F).reshape(-1, 2)
    k = kmeans_init(wh, K) if start is None else np.asarray(start, dtype=F).reshape(-1, 2).copy()
    a = np.zeros(len(wh), dtype=np.int32)
    for _ in range(iters):
        a = kmeans_assign(wh, k)
        for j in range(K):
            sel = a == j
            if sel.any():
                k[j] = (wh[sel].astype(np.float64).sum(0) / sel.sum()).astype(F)
    return k, a


def lognormal_sizes(n, seed=7):
    """The synthetic label sizes of the tests and the benchmark: w = exp(N(3, 0.8)), h = w * exp(|N(0.6, 0.5)|), float32 [n, 2]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    w = np.exp(rng.normal(3.0, 0.8, n))
    h = w * np.exp(np.abs(rng.normal(0.6, 0.5, n)))
    return np.stack([w, h], 1).astype(F)
