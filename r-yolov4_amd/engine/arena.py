"""Liveness-based placement of a plan's activation and activation-gradient buffers in ONE arena.

A plan (engine/graph.py) is a fixed sequence of launches, so every buffer has a known first and last use.  The network is planned
twice: a DRY pass hands out virtual addresses (tag bit 60, never dereferenced — the C-ABI plan helpers only do arithmetic on them),
this module finds every launch that mentions a buffer by scanning the launch arguments and parameter blocks for tagged addresses,
turns the uses into lifetimes on the main stream's timeline, and packs the buffers (largest first, lowest free offset); the second
pass emits the same launches with arena addresses.  In training every forward activation lives until its backward use, so the gain is
the gradient twins: the gradients of the early (largest) layers are written at the end of backward, into the memory of the late layers'
activations and gradients, dead by then.  In inference plans the activations themselves are recycled.

Concurrency: a launch on a side stream may run later / earlier than its tape position, so each of its uses is widened to the interval of
main-stream positions it can overlap with.  Which launch runs where and what waits for what is stated in engine/schedule.py, and the
intervals are read off that statement (schedule.intervals) — this module holds no rule about streams.  Two buffers share memory only if
their lifetimes are disjoint.  Serial replays (timing passes, CPU) are a special case of the scheduled order.
"""
import ctypes as C

from . import schedule

VTAG = 1 << 60
_IDSHIFT = 42
ALIGN = 256


class Virt:
    """Stand-in for a device tensor in the dry pass: an address that nobody dereferences."""

    def __init__(self, ident, nbytes):
        self.ident, self.nbytes = ident, nbytes

    def data_ptr(self):
        return VTAG | (self.ident << _IDSHIFT)


def _tagged(obj, out):
    """Collect the buffer ids of every tagged address inside a launch argument (int, ctypes struct / array, nested)."""
    if obj is None:
        return
    if isinstance(obj, int):
        if obj >> 60 == 1:
            out.add((obj & (VTAG - 1)) >> _IDSHIFT)
        return
    if isinstance(obj, C.Structure):
        for name, *_ in obj._fields_:
            _tagged(getattr(obj, name), out)
        return
    if isinstance(obj, C.Array):
        if issubclass(obj._type_, (C.Structure, C.Array)) or obj._type_ in (C.c_void_p, C.c_uint64, C.c_int64, C.c_size_t):
            for e in obj:
                _tagged(e, out)


class Layout:
    def __init__(self):
        self.off = {}            # buffer ident (2k: activation of Buf k, 2k + 1: its gradient) -> byte offset
        self.total = 0
        self.sum_bytes = 0
        self.names = None        # (forward, backward) kernel-name sequences of the dry pass: the second pass must repeat them
        self.life = {}           # ident -> (first, last) on the main stream's timeline (forward then backward positions)


def uses(g):
    """g: a finished DRY Graph.  ident -> positions of the launches that mention the buffer, on ONE timeline: forward tape positions, then
    len(g.fwd) + backward tape positions."""
    out, base = {}, 0
    for tape in (g.fwd, g.bwd):
        for i in range(len(tape)):
            ids = set()
            for a in g._raw.get((id(tape), i), ()):
                _tagged(a, ids)
            for k in ids:
                out.setdefault(k, []).append(base + i)
        base += len(tape)
    return out


def lifetimes(g):
    """ident -> (first, last) on the main stream's timeline: the hull of the intervals its uses can overlap with under the tapes' schedules."""
    F = len(g.fwd)
    span = schedule.intervals(g.schedule(g.fwd), F) + [(F + lo, F + hi) for lo, hi in schedule.intervals(g.schedule(g.bwd), len(g.bwd))]
    return {k: (min(span[p][0] for p in at), max(span[p][1] for p in at)) for k, at in uses(g).items()}


def pack(sizes, life):
    """sizes: ident -> bytes; life: ident -> (first, last).  Greedy by size: each buffer takes the lowest offset free of every already
    placed buffer whose lifetime intersects its own."""
    order = sorted(sizes, key=lambda k: (-sizes[k], life[k][0], k))
    placed = []                                      # (offset, end, first, last)
    off = {}
    total = 0
    for k in order:
        n = (sizes[k] + ALIGN - 1) // ALIGN * ALIGN
        lo, hi = life[k]
        busy = sorted((o, e) for o, e, a, b in placed if not (b < lo or hi < a))
        at = 0
        for o, e in busy:
            if o - at >= n:
                break
            at = max(at, e)
        off[k] = at
        placed.append((at, at + n, lo, hi))
        total = max(total, at + n)
    return off, total


def plan(g):
    """g: a finished DRY Graph.  Returns the Layout for the real pass."""
    life = lifetimes(g)
    sizes = {}
    F, B = len(g.fwd), len(g.bwd)
    for ident, v in g._virt.items():
        sizes[ident] = v.nbytes
        if ident not in life:                        # allocated but never handed to a launch: keep it apart for the whole plan
            life[ident] = (0, max(F + B - 1, 0))
    lay = Layout()
    lay.off, lay.total = pack(sizes, life)
    lay.sum_bytes = sum((n + ALIGN - 1) // ALIGN * ALIGN for n in sizes.values())
    lay.life = life
    lay.sizes = sizes
    lay.names = ([e[2] for e in g.fwd], [e[2] for e in g.bwd])
    return lay


def check(lay):
    """No two buffers with intersecting lifetimes intersect in memory (test helper)."""
    items = [(lay.off[k], lay.off[k] + lay.sizes[k], lay.life[k]) for k in lay.off]
    items.sort()
    for i, (o, e, (a, b)) in enumerate(items):
        for o2, e2, (a2, b2) in items[i + 1:]:
            if o2 >= e:
                break
            if not (b < a2 or b2 < a):
                return False
    return True
