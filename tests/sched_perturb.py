"""Schedule perturbation of the step engine's command lists (tests/test_schedule_independence_gpu.py).

A command list moves blocks of ops onto the executor's side stream (OP_SIDE_BEGIN ... OP_SIDE_END(event)); the main stream runs on and
meets OP_WAIT_SIDE(event) where it needs the block's result.  A side block S forks behind everything listed before it, so it can only
conflict with the main-stream launches M between its fork and its wait.  The serial schedule (`serial()`: control ops skipped, blocks
inline) runs S, then M; natural timing leaves the order open; `late_side` forces M, then S, by opening every block with a bounded hold.
The kernels are deterministic, so every legal schedule gives the serial schedule's bits, and a list with a missing edge does not.

Nothing here touches a GPU by itself: the rewrites work on `Plan.ops` lists (tuples `(kind, i0, i1, i2, a, b, c)`), `perturbed` on any
object with the engine's attributes."""
import contextlib

KIND, I0 = 0, 1         # positions in an op tuple (volta_amd/engine/plan.py: op)
HOLD_MAX_US = 100000    # what vk_hold_cus accepts


def _L():
    from volta_amd import _lib as L
    return L


def hold_op(hold_us):
    """One generic op FN_HOLD, n = (1, hold_us, 0): vk_hold_cus(1, hold_us, 0) -- one resident wave without LDS for hold_us microseconds, on
    whichever stream the executor issues it.  The tuple carries its GenericArgs, so the structure lives as long as the list it is put in."""
    L = _L()
    assert 0 < int(hold_us) <= HOLD_MAX_US, "vk_hold_cus holds for at most 0.1 s (asked for %r us)" % (hold_us,)
    g = L.GenericArgs()
    g.fn = L.FN_HOLD
    g.n[0], g.n[1], g.n[2] = 1, int(hold_us), 0
    return (L.OP_GENERIC, 0, 0, 0, g, None, None)


def late_side(ops, hold_us, make_hold=None):
    """A copy of `ops` with one hold op (`make_hold(hold_us)`, default `hold_op`) directly behind every OP_SIDE_BEGIN: the executor issues it
    on the side stream, so every side block starts hold_us late while the main stream runs on until it meets a wait.  The ops themselves are
    the same objects as in `ops`."""
    begin = _L().OP_SIDE_BEGIN
    make_hold = make_hold or hold_op
    out = []
    for o in ops:
        out.append(o)
        if o[KIND] == begin:
            out.append(make_hold(hold_us))
    return out


def without_wait(ops, event):
    """A copy of `ops` without its first OP_WAIT_SIDE of `event` (sensitivity cases only); raises if there is none."""
    wait = _L().OP_WAIT_SIDE
    for i, o in enumerate(ops):
        if o[KIND] == wait and o[I0] == event:
            return list(ops[:i]) + list(ops[i + 1:])
    raise ValueError("no OP_WAIT_SIDE of event %d in the list" % event)


def implied_by(ops, event):
    """The index of an op that orders the main stream behind `event`'s side block before the first OP_WAIT_SIDE of `event` is met, or None
    when that wait is the only edge.  The side stream runs its blocks in list order, so a wait for a block that was opened behind
    `event`'s block (or an OP_JOIN) also waits for `event`'s block: taking the wait of `event` out of such a list removes no edge, and no
    schedule can show that it is gone."""
    L = _L()
    rec = next(i for i, o in enumerate(ops) if o[KIND] == L.OP_SIDE_END and o[I0] == event)
    later = set()
    for i in range(rec + 1, len(ops)):
        kind, ev = ops[i][KIND], ops[i][I0]
        if kind == L.OP_WAIT_SIDE and ev == event:
            return None
        if kind == L.OP_SIDE_END:
            later.add(ev)
        elif kind == L.OP_JOIN or (kind == L.OP_WAIT_SIDE and ev in later):
            return i
    raise ValueError("no OP_WAIT_SIDE of event %d behind its OP_SIDE_END" % event)


def count_holds(ops):
    L = _L()
    return sum(1 for o in ops if o[KIND] == L.OP_GENERIC and isinstance(o[4], L.GenericArgs) and o[4].fn == L.FN_HOLD)


def boundary_map(old, new):
    """`new` is `old` with ops put in and ops taken out, the rest the same objects in the same order.  Returns m with len(old) + 1 entries:
    m[i] = the position in `new` of the first op of old[i:] that `new` still has, len(new) if none is left -- where a boundary that stood in
    front of old[i] stands in `new`.  An op put in directly in front of a surviving old[i] lands before the boundary."""
    pos, j = [None] * len(old), 0
    for i, o in enumerate(old):
        k = j
        while k < len(new) and new[k] is not o:
            k += 1
        if k < len(new):            # found: everything between j and k was put in; not found: old[i] was taken out
            pos[i], j = k, k + 1
    m, nxt = [0] * (len(old) + 1), len(new)
    m[len(old)] = nxt
    for i in range(len(old) - 1, -1, -1):
        if pos[i] is not None:
            nxt = pos[i]
        m[i] = nxt
    return m


INDEX_TABLES = (("bwd_marks", "bwd"), ("fwd_sub_start", "fwd"), ("fwd_heads_start", "fwd"))      # every op-index table a StepEngine keeps


@contextlib.contextmanager
def perturbed(eng, fwd_ops=None, bwd_ops=None):
    """Run `eng` on rewritten lists: on entry `fwd_ops` / `bwd_ops` (None: leave that list alone) become eng.fwd.ops / eng.bwd.ops and are
    frozen, every op-index table of the engine (INDEX_TABLES) is moved to the new positions and the `_fwd_segments` cache, which holds such
    positions, is emptied; on exit the original lists, frozen arrays, tables and cache are back -- the same objects."""
    saved = {"_fwd_segments": eng._fwd_segments}
    for attr, _ in INDEX_TABLES:
        saved[attr] = getattr(eng, attr)
    plans = [(eng.fwd, fwd_ops, "fwd"), (eng.bwd, bwd_ops, "bwd")]
    saved_plans = [(p, p.ops, p.c_ops) for p, _, _ in plans]
    try:
        maps = {}
        for plan, ops, which in plans:
            if ops is None:
                continue
            maps[which] = boundary_map(plan.ops, ops)
            plan.ops = list(ops)
            plan.freeze()
        for attr, which in INDEX_TABLES:
            if which in maps:
                old = saved[attr]
                setattr(eng, attr, maps[which][old] if isinstance(old, int) else [maps[which][i] for i in old])
        eng._fwd_segments = {}
        yield eng
    finally:
        for p, ops, c_ops in saved_plans:
            p.ops, p.c_ops = ops, c_ops
        for attr, val in saved.items():
            setattr(eng, attr, val)


@contextlib.contextmanager
def serial():
    """The reference schedule: vk_side_enable(0) makes the executor skip every control op and run each side block inline, in list order.
    The switch is process-wide; it is back on when the block leaves, however it leaves."""
    lib = _L().lib
    lib.vk_side_enable(0)
    try:
        yield
    finally:
        lib.vk_side_enable(1)


def events(ops):
    """(recorded, waited): the side events the list's OP_SIDE_END ops record, in list order with repeats, and the set its OP_WAIT_SIDE ops wait for."""
    L = _L()
    return [o[I0] for o in ops if o[KIND] == L.OP_SIDE_END], {o[I0] for o in ops if o[KIND] == L.OP_WAIT_SIDE}
