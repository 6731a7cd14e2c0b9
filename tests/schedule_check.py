"""Checker of the stream and event schedule of one exec (test infrastructure, numpy only).

run_chain (distributedfft_amd/csrc/dfft.hip) decides which stream every launch and exchange of an exec runs on and which events order
them.  tests/layout_sim.py replays the same steps one after the other: it proves the data flow correct IF the steps run in that
order.  This module checks that the streams and events force an order that is good enough: input is ONE rank's trace
(MPIcuFFT.debugTrace: the list the executor's own loop produces), its chain steps (debugChain) and the footprints of its data
operations; output is a list of violations, each naming the rule and the two operations.

Happens-before.  Operations on one stream are ordered as issued.  A wait on event e is ordered after the latest record of e issued
before it (rule "event": a wait on an event that was never recorded before it).  The relation is the transitive closure.  ENTRY is the
head of stream 0 (the caller's earlier work), EXIT its tail (what the caller enqueues next).

Rules.
  1  every launch and exchange happens after ENTRY
  2  every launch and exchange happens before EXIT
  3  two data operations whose footprints conflict on a buffer (one writes what the other reads or writes): the one issued first
     happens before the other.  A launch conflicts with itself if it stores to elements it loads: its workgroups are not ordered
     and no kernel of the library works in place
  4  replayed in issue order, every element a data operation reads from the work area, from `out`, or from `in` after the chain's
     first write to `in`, was last written by an operation that happens before it (and was written at all)
  5  the trace is consistent with the chain: every launch of every step exactly once, chunk c = launches c*per_chunk ..
     (c+1)*per_chunk-1, one exchange per chunk of a step with an exchange, from its dst to the next step's src
No pair of operations is exempt by step, group, chunk or name: two unordered operations on one buffer are acceptable only if their
footprints are disjoint.

Out of scope.  Operations of OTHER ranks: how a transport orders a peer's access to this rank's send and receive buffers is the
contract of comm.hip (covered by the relay, gloo and MPI tests).  The relay's internal staging and side stream likewise: a trace with
the relay on equals the trace with it off.

Footprints are in units of one real element per buffer: "in", "out", "W" (the work area: slice k starts at k * domain size, so that a
launch that runs over the end of its slice meets the next one) and "S" (the shared level scratch of two-level and long-Bluestein
passes: one token element that every launch with scratch = 1 reads and writes).
"""
import numpy as np

LAUNCH, EXCHANGE, RECORD, WAIT = 0, 1, 2, 3
KIND = ["launch", "exchange", "record", "wait"]


def describe(i, op):
    if op["kind"] == LAUNCH:
        return f"#{i} launch step {op['step']} chunk {op['chunk']} launch {op['launch']} on stream {op['stream']} ({op['src']} -> {op['dst']})"
    if op["kind"] == EXCHANGE:
        return f"#{i} exchange {op['which']} of step {op['step']} chunk {op['chunk']} on stream {op['stream']} ({op['src']} -> {op['dst']})"
    return f"#{i} {KIND[op['kind']]} event {op['event']} on stream {op['stream']}"


class Violation:
    def __init__(self, rule, a, b, text):
        self.rule, self.a, self.b, self.text = rule, a, b, text

    def __repr__(self):
        return f"rule {self.rule}: {self.text}"


def bits(idx, size=None):
    """a set of element indices as a Python int (bit i = element i): intersections of footprints are one `&`"""
    idx = np.asarray(idx, dtype=np.int64)
    if idx.size == 0:
        return 0
    m = np.zeros((int(idx.max()) // 8 + 1) * 8, dtype=np.uint8)
    m[idx] = 1
    return int.from_bytes(np.packbits(m, bitorder="little").tobytes(), "little")


def happens_before(trace):
    """hb[i]: bit j set = operation j happens before operation i.  Indices are those of `trace`; ENTRY = len(trace), EXIT =
    len(trace) + 1.  Also returns the violations of rule "event"."""
    n = len(trace)
    ENTRY, EXIT = n, n + 1
    hb = [0] * (n + 2)
    last_on = {0: ENTRY}       # stream -> last operation issued on it
    last_rec = {}              # event -> latest record
    bad = []
    for i, op in enumerate(trace):
        pred = []
        if op["stream"] in last_on:
            pred.append(last_on[op["stream"]])
        if op["kind"] == WAIT:
            if op["event"] in last_rec:
                pred.append(last_rec[op["event"]])
            else:
                bad.append(Violation("event", i, None, f"{describe(i, op)} waits for an event that no earlier operation recorded"))
        for q in pred:
            hb[i] |= hb[q] | (1 << q)
        last_on[op["stream"]] = i
        if op["kind"] == RECORD:
            last_rec[op["event"]] = i
    q = last_on[0]
    hb[EXIT] = hb[q] | (1 << q)
    return hb, bad


def data_relation(trace, hb=None):
    """the happens-before relation restricted to data operations, ENTRY and EXIT (what the mutation test compares)"""
    if hb is None:
        hb, _ = happens_before(trace)
    n = len(trace)
    keep = [i for i, op in enumerate(trace) if op["kind"] in (LAUNCH, EXCHANGE)] + [n, n + 1]
    key = lambda i: "ENTRY" if i == n else "EXIT" if i == n + 1 else tuple(sorted(trace[i].items()))      # noqa: E731
    return {(key(a), key(b)) for b in keep for a in keep if hb[b] >> a & 1}


def check(trace, steps, footprint):
    """trace: list of dicts (dfft_trace_op); steps: list of dicts (dfft_chain_step); footprint(i, op) -> (reads, writes), each a dict
    buffer -> array of real-element indices, for the data operation at index i.  Returns the list of violations."""
    n = len(trace)
    ENTRY, EXIT = n, n + 1
    hb, out = happens_before(trace)
    data = [i for i, op in enumerate(trace) if op["kind"] in (LAUNCH, EXCHANGE)]
    fp = {i: footprint(i, trace[i]) for i in data}
    # rules 1 and 2
    for i in data:
        if not hb[i] >> ENTRY & 1:
            out.append(Violation(1, ENTRY, i, f"{describe(i, trace[i])} is not ordered after ENTRY (the caller's earlier work on stream 0)"))
        if not hb[EXIT] >> i & 1:
            out.append(Violation(2, i, EXIT, f"{describe(i, trace[i])} is not ordered before EXIT (what the caller enqueues next on stream 0)"))
    # rule 4
    raw = set()            # (producer, consumer) pairs reported here
    last = {}              # buffer -> last writer per element (-1: none)
    in_written = False

    def writer_array(b, upto):
        a = last.get(b)
        if a is None or len(a) <= upto:
            g = np.full(upto + 1, -1, dtype=np.int64)
            if a is not None:
                g[:len(a)] = a
            last[b] = a = g
        return a
    for i in data:
        reads, writes = fp[i]
        for b, idx in reads.items():
            if b == "S" or len(idx) == 0 or (b == "in" and not in_written):
                continue
            who = np.unique(writer_array(b, int(idx.max()))[idx])
            for w in who:
                if w < 0:
                    out.append(Violation(4, None, i, f"{describe(i, trace[i])} reads {int(np.sum(writer_array(b, int(idx.max()))[idx] < 0))} elements of buffer {b} that no operation of the chain wrote"))
                elif not hb[i] >> int(w) & 1:
                    raw.add((int(w), i))
                    out.append(Violation(4, int(w), i, f"{describe(i, trace[i])} reads from buffer {b} what {describe(int(w), trace[int(w)])} wrote, which does not happen before it"))
        for b, idx in writes.items():
            if len(idx):
                writer_array(b, int(idx.max()))[idx] = i
                in_written = in_written or b == "in"
    # rule 3 (a read-after-write pair that rule 4 has just reported with its producer is not reported twice)
    rb = {i: {b: bits(v) for b, v in fp[i][0].items()} for i in data}
    wb = {i: {b: bits(v) for b, v in fp[i][1].items()} for i in data}
    for x, j in enumerate(data):
        for b, w in wb[j].items():
            if b != "S" and trace[j]["kind"] == LAUNCH and w & rb[j].get(b, 0):
                out.append(Violation(3, j, j, f"{describe(j, trace[j])} writes elements of buffer {b} that it reads itself: the workgroups of one launch are not ordered"))
        for i in data[:x]:
            if hb[j] >> i & 1:
                continue
            for b, w in wb[i].items():
                if w & wb[j].get(b, 0) or (w & rb[j].get(b, 0) and (i, j) not in raw):
                    out.append(Violation(3, i, j, f"{describe(i, trace[i])} writes buffer {b} where {describe(j, trace[j])} reads or writes it, and does not happen before it"))
            for b, w in wb[j].items():
                if w & rb[i].get(b, 0):
                    out.append(Violation(3, i, j, f"{describe(i, trace[i])} reads buffer {b} where {describe(j, trace[j])} writes it, and does not happen before it"))
    # rule 5
    seen = {}
    for i in data:
        op = trace[i]
        s = op["step"]
        if not 0 <= s < len(steps):
            out.append(Violation(5, i, None, f"{describe(i, op)}: the chain has no such step"))
            continue
        st = steps[s]
        if op["kind"] == LAUNCH:
            seen.setdefault((s, op["launch"]), []).append(i)
            if op["launch"] // st["per_chunk"] != op["chunk"] or (op["src"], op["dst"]) != (st["src"], st["dst"]):
                out.append(Violation(5, i, None, f"{describe(i, op)}: chunk or buffers are not those of step {s} ({st})"))
        else:
            seen.setdefault((s, "x", op["chunk"]), []).append(i)
            ok = st["exchange"] == op["which"] and s + 1 < len(steps) and (op["src"], op["dst"]) == (st["dst"], steps[s + 1]["src"])
            if not ok:
                out.append(Violation(5, i, None, f"{describe(i, op)}: not the exchange of step {s} ({st})"))
    for s, st in enumerate(steps):
        want = [(s, k) for k in range(st["launches"])]
        if st["exchange"]:
            want += [(s, "x", c) for c in range(st["launches"] // st["per_chunk"])]
        for k in want:
            if len(seen.get(k, [])) != 1:
                out.append(Violation(5, None, None, f"step {s} ({st['group']}): {'exchange of chunk' if len(k) == 3 else 'launch'} {k[-1]} appears {len(seen.get(k, []))} times in the trace"))
    for k in seen:
        if k[0] < len(steps) and k[1] != "x" and not 0 <= k[1] < steps[k[0]]["launches"]:
            out.append(Violation(5, seen[k][0], None, f"{describe(seen[k][0], trace[seen[k][0]])}: step {k[0]} has no such launch"))
    return out


# ---- footprints of a real plan -------------------------------------------------------------------------------------------------
class PlanFootprints:
    """footprints of the data operations of one rank's plan, from the plan's own descriptors (layout_sim.Pass.footprint) and chunked
    exchange tables (getPipelineTables); cached per (group, launch, line form) and per (direction, exchange, chunk)"""

    def __init__(self, plan, shape):
        import layout_sim
        self.sim = layout_sim
        self.plan = plan
        self.length = (shape[2], shape[1], shape[0])      # by axis: z, y, x
        self.half = (16 if plan.precision == 1 else 8) // 2      # bytes per real element
        self.slice = plan.getDomainSize() // self.half
        self.cache = {}

    def where(self, b, idx):
        return ("in", idx) if b == -2 else ("out", idx) if b == -1 else ("W", idx + b * self.slice)

    def launch(self, st, k):
        key = (st["group"], k, st["form"])
        if key not in self.cache:
            self.cache[key] = self.sim.Pass(self.plan, st["group"], k).footprint(self.length[st["axis"]], self.sim.MODES[st["form"]])
        return self.cache[key]

    def exchange(self, direction, which, c):
        key = ("x", direction, which, c)
        if key not in self.cache:
            sc, sd, rc, rd = self.plan.getPipelineTables(direction, which, c)
            rng = lambda cnt, dsp: np.concatenate([np.arange(d // self.half, (d + n) // self.half, dtype=np.int64) for n, d in zip(cnt, dsp)] + [np.zeros(0, dtype=np.int64)])      # noqa: E731
            self.cache[key] = (rng(sc, sd), rng(rc, rd))
        return self.cache[key]

    def of(self, direction, steps):
        def footprint(i, op):
            if op["kind"] == LAUNCH:
                ld, st = self.launch(steps[op["step"]], op["launch"])
                rb, ri = self.where(op["src"], ld)
                wb, wi = self.where(op["dst"], st)
                reads, writes = {rb: ri}, {wb: wi}
                if op["scratch"]:
                    reads["S"] = writes["S"] = np.zeros(1, dtype=np.int64)
                return reads, writes
            ld, st = self.exchange(direction, op["which"], op["chunk"])
            rb, ri = self.where(op["src"], ld)
            wb, wi = self.where(op["dst"], st)
            return {rb: ri}, {wb: wi}
        return footprint


def check_plan(plan, shape, direction, dims=3, fps=None, trace=None):
    """the violations of the schedule the plan's next exec would issue (or of `trace`)"""
    steps = plan.debugChain(direction, dims)
    fps = fps or PlanFootprints(plan, shape)
    return check(plan.debugTrace(direction, dims) if trace is None else trace, steps, fps.of(direction, steps))
