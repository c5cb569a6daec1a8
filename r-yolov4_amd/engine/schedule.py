"""The stream schedule of a tape: which launch runs on which stream, and what waits for what.  Stated HERE once: Graph.run
(engine/graph.py) executes these operations and decides nothing about streams itself, engine/arena.py lets two buffers share memory
only where these operations order their uses, and the planner asks wgrad_lane() which weight gradients share a split-K workspace.
Pure Python (no torch, no hip): streams and events are small integers that Graph.run binds to HIP objects once per plan.

Streams: 0 is the main stream, s > 0 the engine's side stream that Runtime.side_stream(s) hands out.
An operation is (REC, event, stream) — record the event on the stream — or (WAIT, event, stream) — the stream waits for the event.

Forward (forward()): the planner marks sibling branches of a block for lane 1 and the detection-head tails for lane 2 (Graph.fwd_side) and
the points where a lane-1 branch's output is consumed (Graph.fwd_join).
  * fork: the first entry of a branch runs behind an event recorded on the main stream — the branch may read everything enqueued so far;
  * join (lane 1 only): at a join point lane 1 records an event — a snapshot: branches forked later are not waited for — and the first
    main-stream launch from there on waits for it;
  * lane 2 is joined at the end of the tape only, lane 1 there once more.
Backward (backward()): the weight gradients (Graph.side_idx; results needed only by the optimizer) leave the main stream.
  * weight gradient n runs on lane wgrad_lane(n, lanes) behind an event recorded on the main stream: its operands are final once everything
    before it ran;
  * bounded lag: each records a completion event, and the main stream waits for number n - lag before it enqueues number n — so what
    weight gradient n reads can be handed out again from weight gradient n + lag on.  lag = 0: no such waits, the operands stay until the end;
  * a gradient-bucket hook fired after position i gets ONE event to wait for (`hook[i]`): the other lanes funnel into lane 0's stream, which
    records it; the main stream is not stalled;
  * the end of the tape joins every lane that was used.
A tape with nothing on a side stream has no schedule (None), and neither has a serial or a CPU replay: everything in tape order on one stream.
"""

REC, WAIT = 0, 1
NO_HOOK = ((), None)


def wgrad_lane(n, lanes):
    """Lane of the n-th side-stream launch of a backward tape: round-robin (with small batches one weight-gradient kernel does not fill the
    GPU).  Launches of one lane are ordered, so they may share one split-K workspace."""
    return n % max(1, lanes)


def wgrad_stream(lane):
    """Side stream of a weight-gradient lane: lane 0 shares stream 1 with the forward branches; stream 2 belongs to the head tails."""
    return 1 if lane == 0 else 2 + lane


class Schedule:
    def __init__(self, n):
        self.stream = [0] * n                    # per tape position: the stream its launch runs on
        self.before = [()] * n                   # per tape position: operations issued before its launch ...
        self.after = [()] * n                    # ... and after it
        self.hook = [NO_HOOK] * n                # per tape position: (operations before a hook fired there, the event the hook is handed | None)
        self.end = ()                            # operations after the last launch
        self.events = 0                          # events are numbered 0 .. events - 1

    def event(self):
        self.events += 1
        return self.events - 1


def forward(n, fwd_side, fwd_join):
    """fwd_side: {position: (first entry of its branch, lane)}; fwd_join: positions before which lane 1 is joined."""
    if not fwd_side:
        return None
    s = Schedule(n)
    joined = {1: s.event(), 2: s.event()}
    used, pending = set(), None
    for i in range(n):
        ops = []
        if 1 in used and i in fwd_join:
            pending = s.event()
            ops.append((REC, pending, 1))
        ent = fwd_side.get(i)
        if ent is not None:
            first, lane = ent
            s.stream[i] = lane = 2 if lane == 2 else 1
            used.add(lane)
            if first:
                e = s.event()
                ops += [(REC, e, 0), (WAIT, e, lane)]
        elif pending is not None:
            ops.append((WAIT, pending, 0))
            pending = None
        s.before[i] = tuple(ops)
        if 1 in used:
            s.hook[i] = (((REC, joined[1], 1),), joined[1])
    s.end = tuple(op for lane in sorted(used) for op in ((REC, joined[lane], lane), (WAIT, joined[lane], 0)))
    return s


def backward(n, side_idx, lanes, lag):
    """side_idx: positions of the launches that leave the main stream; lanes: streams they are dealt to; lag: see the module docstring."""
    if not side_idx:
        return None
    s = Schedule(n)
    joined = s.event()
    funnel = [s.event() for _ in range(max(1, lanes))]
    order = sorted(side_idx)
    done, used = [], set()

    def gather(into):
        """Everything enqueued so far on any lane, as the one event `joined` recorded on lane 0's stream."""
        ops = []
        for k in sorted(used - {0}):
            ops += [(REC, funnel[k], wgrad_stream(k)), (WAIT, funnel[k], into)]
        return tuple(ops) + ((REC, joined, 1),)

    for k, i in enumerate(order):
        lane = wgrad_lane(k, lanes)
        st = s.stream[i] = wgrad_stream(lane)
        e = s.event()
        s.before[i] = (((WAIT, done[k - lag], 0),) if lag and k >= lag else ()) + ((REC, e, 0), (WAIT, e, st))
        if lag:
            done.append(s.event())
            s.after[i] = ((REC, done[k], st),)
        used.add(lane)
        hook = (gather(1), joined)
        for j in range(i, order[k + 1] if k + 1 < len(order) else n):
            s.hook[j] = hook
    s.end = gather(0) + ((WAIT, joined, 0),)
    return s


def intervals(s, n):
    """Per position of an n-entry tape the interval (lo, hi) of main-stream positions its launch can overlap with.  Read off the
    operations: lo = where on the main stream the last event was recorded that the launch's stream waited for; hi = the position before
    the main stream's first wait that covers the launch (transitively: each event carries what its stream knew when it recorded it).
    A main-stream launch overlaps with itself only."""
    out = [(i, i) for i in range(n)]
    if s is None:
        return out
    # knows[a][b] = t: everything stream b launched at tape positions < t has finished before what stream a enqueues next starts
    knows, at_record, open_ = {0: {}}, {}, {}

    def apply(ops, now, last):
        for kind, e, st in ops:
            mine = knows.setdefault(st, {})
            if kind == REC:
                if st == 0:
                    mine[0] = now
                at_record[e] = dict(mine)
                continue
            for b, t in at_record[e].items():
                if t > mine.get(b, 0):
                    mine[b] = t
            if st == 0:
                for b, waiting in open_.items():
                    while waiting and waiting[0] < mine.get(b, 0):
                        i = waiting.pop(0)
                        out[i] = (out[i][0], last)
    for i in range(n):
        apply(s.before[i], i, i - 1)
        st = s.stream[i]
        if st:
            mine = knows.setdefault(st, {})
            out[i] = (mine.get(0, 0), None)
            mine[st] = i + 1
            open_.setdefault(st, []).append(i)
        apply(s.after[i], i + 1, i)
    apply(s.end, n, n - 1)
    left = [i for w in open_.values() for i in w]
    if left:
        raise RuntimeError(f"engine: the stream schedule ends with positions {left} never joined by the main stream")
    return out
