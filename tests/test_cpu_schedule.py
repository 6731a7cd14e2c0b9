"""The stream and event schedule of every execution chain, checked without a GPU: the trace that run_chain's own loop produces
(MPIcuFFT.debugTrace, csrc/dfft.hip) against the footprints of its launches and exchanges (tests/schedule_check.py: happens-before
from streams and events, rules 1-5).  tests/test_cpu_layout.py proves the data flow of the steps run one after the other; this file
proves that the streams and events force an order that is as good."""
import numpy as np
import pytest

import distributedfft_amd as dfft
import schedule_check as sc
from layout_sim import World
from schedule_check import EXCHANGE, LAUNCH, RECORD, WAIT

F, I = dfft.FORWARD, dfft.INVERSE


# ------------------------------------------------------------------------------------------------------------------------------
# the checker checks: hand-written traces with exactly one defect each
# ------------------------------------------------------------------------------------------------------------------------------
def L(stream, step, chunk, src, dst, launch=None, scratch=0):
    return dict(kind=LAUNCH, stream=stream, event=-1, step=step, chunk=chunk, launch=chunk if launch is None else launch, src=src, dst=dst, which=0, scratch=scratch)


def X(stream, step, chunk, src, dst, which=1):
    return dict(kind=EXCHANGE, stream=stream, event=-1, step=step, chunk=chunk, launch=-1, src=src, dst=dst, which=which, scratch=0)


def R(stream, event):
    return dict(kind=RECORD, stream=stream, event=event, step=-1, chunk=-1, launch=-1, src=-1, dst=-1, which=0, scratch=0)


def W(stream, event):
    return dict(kind=WAIT, stream=stream, event=event, step=-1, chunk=-1, launch=-1, src=-1, dst=-1, which=0, scratch=0)


def step(group, launches, src, dst, exchange=0, per_chunk=1):
    return dict(group=group, axis=0, launches=launches, per_chunk=per_chunk, src=src, dst=dst, conj=0, form=0, exchange=exchange, split=1)


# a toy chain of two chunks: a: in -> W0 (chunk c: elements 10c .. 10c+9), exchange 1: W0 -> W1 (slice size 100), b: W1 -> out
TOY_STEPS = [step("a", 2, -2, 0, exchange=1), step("b", 2, 1, -1)]
BUF = {-2: ("in", 0), -1: ("out", 0), 0: ("W", 0), 1: ("W", 100)}


def toy_footprint(i, op):
    rng = np.arange(10 * op["chunk"], 10 * op["chunk"] + 10)
    (rb, ro), (wb, wo) = BUF[op["src"]], BUF[op["dst"]]
    reads, writes = {rb: rng + ro}, {wb: rng + wo}
    if op["scratch"]:
        reads["S"] = writes["S"] = np.zeros(1, dtype=np.int64)
    return reads, writes


def toy_trace(two=False, scratch=0):
    """the executor's pattern for TOY_STEPS: entry fence, chunk -> ready -> exchange -> done, consumer chunk c behind done[c], final join"""
    s1 = 1 if two else 0
    t = [R(0, 0), W(2, 0)] + ([W(1, 0)] if two else [])
    t += [L(0, 0, 0, -2, 0, scratch=scratch), R(0, 1), W(2, 1), X(2, 0, 0, 0, 1), R(2, 2)]
    t += [L(s1, 0, 1, -2, 0, scratch=scratch), R(s1, 3), W(2, 3), X(2, 0, 1, 0, 1), R(2, 4)]
    t += [W(0, 2), L(0, 1, 0, 1, -1), W(s1, 4), L(s1, 1, 1, 1, -1)]
    return t + ([R(1, 5), W(0, 5)] if two else [])


def rules(trace, steps=TOY_STEPS, fp=toy_footprint):
    return sorted({str(v.rule) for v in sc.check(trace, steps, fp)})


def without(trace, *ops):
    t = list(trace)
    for op in ops:
        t.remove(op)
    return t


def test_checker_accepts_the_correct_toy_traces():
    assert sc.check(toy_trace(False), TOY_STEPS, toy_footprint) == []
    assert sc.check(toy_trace(True), TOY_STEPS, toy_footprint) == []


def test_checker_no_entry_fence():
    """the fence event dropped (its record and the waits of the second compute and the communication stream): what stream 1 runs no
    longer follows the caller's earlier work.  The communication stream still does in this pattern -- its first wait is for a chunk
    that ran on stream 0 -- so the launches on stream 1 are what rule 1 names."""
    t = toy_trace(True)
    bad = sc.check(without(t, R(0, 0), W(2, 0), W(1, 0)), TOY_STEPS, toy_footprint)
    assert {v.rule for v in bad} == {1} and {v.a for v in bad} == {len(t) - 3}      # ENTRY
    assert "ENTRY" in bad[0].text and "launch step 0 chunk 1 launch 1 on stream 1" in bad[0].text
    assert sc.check(without(t, W(2, 0)), TOY_STEPS, toy_footprint) == []      # (the communication stream's own wait is implied)


def test_checker_no_final_join_of_stream_1():
    bad = sc.check(without(toy_trace(True), R(1, 5), W(0, 5)), TOY_STEPS, toy_footprint)
    assert {v.rule for v in bad} == {2} and "launch step 1 chunk 1" in bad[-1].text and "EXIT" in bad[-1].text


def test_checker_consumer_waits_for_the_wrong_chunks_event():
    t = toy_trace(True)
    k = t.index(W(1, 4))
    t[k:k + 2] = [W(1, 2), t[k + 1], W(1, 4)]      # chunk 1 of b behind the exchange of chunk 0; the right event only afterwards
    bad = sc.check(t, TOY_STEPS, toy_footprint)
    assert {v.rule for v in bad} == {4}
    assert "exchange 1 of step 0 chunk 1" in bad[0].text and "launch step 1 chunk 1" in bad[0].text


def test_checker_write_into_a_buffer_an_exchange_still_sends_from():
    """b writes where a wrote (dst = W0, chunk 0 of b over the send range of chunk 1): chunk 0 of b waits for exchange chunk 0 only"""
    steps = [step("a", 2, -2, 0, exchange=1), step("b", 2, 1, 0)]

    def fp(i, op):
        reads, writes = toy_footprint(i, op)
        if op["step"] == 1:
            writes = {"W": np.arange(10, 20) if op["chunk"] == 0 else np.arange(0, 10)}
        return reads, writes
    t = [dict(o, dst=0) if o["kind"] == LAUNCH and o["step"] == 1 else o for o in toy_trace(False)]
    bad = sc.check(t, steps, fp)
    assert {v.rule for v in bad} == {3}
    assert "exchange 1 of step 0 chunk 1" in bad[0].text and "launch step 1 chunk 0" in bad[0].text
    # corrected: every chunk of b behind the last exchange chunk
    t2 = without(t, W(0, 2), W(0, 4))
    k = t2.index(next(o for o in t2 if o["kind"] == LAUNCH and o["step"] == 1))
    assert sc.check(t2[:k] + [W(0, 4)] + t2[k:], steps, fp) == []


def test_checker_two_scratch_launches_on_different_streams():
    bad = sc.check(toy_trace(True, scratch=1), TOY_STEPS, toy_footprint)
    assert {v.rule for v in bad} == {3} and "buffer S" in bad[0].text
    assert "launch step 0 chunk 0" in bad[0].text and "launch step 0 chunk 1" in bad[0].text
    assert sc.check(toy_trace(False, scratch=1), TOY_STEPS, toy_footprint) == []


def test_checker_launch_that_writes_what_it_reads():
    steps = [step("a", 2, 0, 0)]
    t = [L(0, 0, 0, 0, 0), L(0, 0, 1, 0, 0)]
    fp = lambda i, op: ({"in": np.arange(4)}, {"W": np.arange(10 * op["chunk"], 10 * op["chunk"] + 10)})      # noqa: E731
    assert sc.check(t, steps, fp) == []
    bad = sc.check(t, steps, toy_footprint)      # reads W0 chunk c, writes W0 chunk c
    assert {v.rule for v in bad} == {3, 4} and "reads itself" in bad[-1].text      # (4: nothing wrote what it reads)


def test_checker_wait_before_its_record():
    t = toy_trace(False)
    bad = sc.check([W(0, 4)] + t, TOY_STEPS, toy_footprint)      # (redundant for the order: only the event rule may fire)
    assert {v.rule for v in bad} == {"event"} and "event 4" in bad[0].text


def test_checker_trace_that_does_not_match_the_chain():
    t = toy_trace(False)
    assert rules(without(t, X(2, 0, 1, 0, 1))) == ["4", "5"]      # (the consumer reads what nothing wrote, too)
    assert rules(t + [L(0, 1, 1, 1, -1)]) == ["5"]
    assert rules([dict(o, chunk=0) if o == L(0, 1, 1, 1, -1) else o for o in t])[-1] == "5"


# ------------------------------------------------------------------------------------------------------------------------------
# real traces
# ------------------------------------------------------------------------------------------------------------------------------
def make_world(cls, shape, P1, P2, c2c, chunks, options=None):
    return World(cls, shape, P1, P2, c2c, chunks, options=options)


def clean(violations, what=""):
    """no violation -- or all of them in the message: the data hazards (rules 3, 4) first"""
    bad = sorted(violations, key=lambda v: v.rule not in (3, 4))
    assert not bad, f"{what}: {len(bad)} violations\n" + "\n".join(repr(v) for v in bad[:10])
    return True


MUTATION_PLANS = [(dfft.MPIcuFFT_Pencil_Opt1, (12, 10, 14), 2, 4), (dfft.MPIcuFFT_Pencil_Opt1, (18, 15, 10), 3, 2),
                  (dfft.MPIcuFFT_Slab_Opt1, (24, 20, 16), 4, 1), (dfft.MPIcuFFT_Pencil_Opt1, (16, 24, 20), 1, 4)]


@pytest.mark.parametrize("chunks", [3, 4, 5])
@pytest.mark.parametrize("c2c", [True, False])
@pytest.mark.parametrize("cls,shape,P1,P2", MUTATION_PLANS)
def test_deleting_a_wait_is_reported_or_redundant(cls, shape, P1, P2, c2c, chunks):
    """every wait of a real two-stream trace deleted in turn: the checker reports it, or the happens-before relation between the data
    operations (ENTRY and EXIT included) is unchanged (the wait was redundant), or -- a `whole` join orders all chunks of two steps,
    also where chunk c of the second only touches what chunk c of the first wrote -- every pair of data operations that lost its
    order has disjoint footprints on every buffer (intersected here with numpy, not with the checker's own bit sets) and neither is
    ENTRY or EXIT.  In every trace at least one deletion is a data hazard (rule 3 or 4)."""
    w = make_world(cls, shape, P1, P2, c2c, chunks)
    assert w.C == chunks
    for r in (0, w.P - 1):
        pl = w.plans[r]
        pl.setOption("compute_streams", 2)
        fps = sc.PlanFootprints(pl, shape)
        for direction in (F, I):
            trace, steps = pl.debugTrace(direction), pl.debugChain(direction)
            fp = fps.of(direction, steps)
            assert {o["stream"] for o in trace} == ({0, 1, 2, 3} if P1 > 1 and P2 > 1 else {0, 1, 2})
            clean(sc.check(trace, steps, fp), f"rank {r} direction {direction}")
            base = sc.data_relation(trace)
            op_of = {tuple(sorted(o.items())): o for o in trace}
            hazards = redundant = stronger = 0
            waits = [i for i, o in enumerate(trace) if o["kind"] == WAIT]
            for i in waits:
                t = trace[:i] + trace[i + 1:]
                bad = sc.check(t, steps, fp)
                if bad:
                    hazards += any(v.rule in (3, 4) for v in bad)
                    continue
                now = sc.data_relation(t)
                assert now <= base
                for a, b in base - now:
                    assert "ENTRY" not in (a, b) and "EXIT" not in (a, b), f"deleting {sc.describe(i, trace[i])} is not reported"
                    (ra, wa), (rb, wb) = fp(0, op_of[a]), fp(0, op_of[b])
                    for x, y in ((wa, rb), (wa, wb), (ra, wb)):
                        for buf in set(x) & set(y):
                            assert len(np.intersect1d(x[buf], y[buf])) == 0, f"deleting {sc.describe(i, trace[i])} is not reported"
                redundant += now == base
                stronger += now != base
            assert hazards >= 1
            print(f"{cls.__name__} {shape} {P1}x{P2} c2c={c2c} chunks={chunks} rank {r} {'forward' if direction == F else 'inverse'}: "
                  f"{len(waits)} waits, {redundant} redundant, {stronger} order only operations with disjoint footprints")


@pytest.mark.parametrize("cls,shape,P1,P2", MUTATION_PLANS)
def test_moving_odd_chunks_to_stream_1_without_waits_is_reported(cls, shape, P1, P2):
    w = make_world(cls, shape, P1, P2, True, 4)
    pl = w.plans[0]
    pl.setOption("compute_streams", 1)
    fps = sc.PlanFootprints(pl, shape)
    for direction in (F, I):
        trace, steps = pl.debugTrace(direction), pl.debugChain(direction)
        clean(sc.check(trace, steps, fps.of(direction, steps)), f"direction {direction}")
        for s, st in enumerate(steps):
            if st["launches"] // st["per_chunk"] < 2:
                continue
            t = [dict(o, stream=1) if o["kind"] == LAUNCH and o["step"] == s and o["chunk"] & 1 else o for o in trace]
            assert sc.check(t, steps, fps.of(direction, steps)), (direction, s)


# ---- every chain, every schedule ---------------------------------------------------------------------------------------------
PENCIL = [dfft.MPIcuFFT_Pencil_Opt1, dfft.MPIcuFFT_Pencil]
SLAB = [dfft.MPIcuFFT_Slab, dfft.MPIcuFFT_Slab_Opt1, dfft.MPIcuFFT_Slab_Z_Then_YX, dfft.MPIcuFFT_Slab_Z_Then_YX_Opt1, dfft.MPIcuFFT_Slab_Y_Then_ZX]
GRIDS = [(1, 1), (2, 1), (1, 2), (2, 2), (3, 2), (2, 4), (4, 1), (1, 4), (8, 1)]
SHAPES = [(16, 16, 16), (12, 10, 14), (9, 7, 10)]      # even, uneven, odd (every grid but 8 x 1 fits the last)
DEPTHS = [1, 2, 3, 4, 5]
STREAMS = [-1, 1, 2]


def fits(cls, shape, P1, P2, c2c):
    """a grid takes a shape when no rank is left without data at any stage: Nx >= P1, Ny >= P1 and P2 (the spectrum's y extent --
    Ny/2+1 for Y_Then_ZX R2C -- is split over P1), the z extent of the spectrum >= P2 (over P1 for Z_Then_YX); slab classes need
    P2 == 1"""
    Nx, Ny, Nz = shape
    if cls in SLAB and P2 != 1:
        return False
    nzc = Nz if c2c else Nz // 2 + 1
    nyc = Ny // 2 + 1 if cls is dfft.MPIcuFFT_Slab_Y_Then_ZX and not c2c else Ny
    zsplit = P1 if cls in (dfft.MPIcuFFT_Slab_Z_Then_YX, dfft.MPIcuFFT_Slab_Z_Then_YX_Opt1) else P2
    return Nx >= P1 and min(Ny, nyc) >= max(P1, P2) and nzc >= zsplit


def check_world(w, shape, streams=STREAMS, options=None, expect_scratch=False):
    """every rank, dims 3, 2, 1, both directions, the given compute_streams settings (set AFTER initFFT: the option is read at exec);
    returns the number of traces checked"""
    cls = type(w.plans[0])
    sequence = cls in (dfft.MPIcuFFT_Slab_Z_Then_YX, dfft.MPIcuFFT_Slab_Z_Then_YX_Opt1, dfft.MPIcuFFT_Slab_Y_Then_ZX)
    n = 0
    for r, pl in enumerate(w.plans):
        fps = sc.PlanFootprints(pl, shape)
        seen = {}
        for direction in (F,) if cls is dfft.MPIcuFFT_Slab_Y_Then_ZX else (F, I):      # (forward only, as in the library)
            for dims in (3,) if sequence else (3, 2, 1):                                 # (no partial transforms, as in the library)
                steps = pl.debugChain(direction, dims)
                by_cs = {}
                for cs in streams:
                    pl.setOption("compute_streams", cs)
                    trace = by_cs[cs] = pl.debugTrace(direction, dims)
                    what = f"{cls.__name__} {shape} {w.P1}x{w.P2} c2c={w.c2c} C={w.C} {options} rank {r} direction {direction} dims {dims} compute_streams {cs}"
                    key = (direction, dims, tuple(tuple(o.values()) for o in trace))
                    if key not in seen:      # (compute_streams = -1 issues one of the other two traces)
                        seen[key] = sc.check(trace, steps, fps.of(direction, steps))
                        n += 1
                    clean(seen[key], what)
                    launches = [o for o in trace if o["kind"] == LAUNCH]
                    assert len(launches) == sum(s["launches"] for s in steps) > 0, what
                    scratch = any(o["scratch"] for o in launches)
                    assert scratch or not expect_scratch or dims < 3, what
                    on1 = [o for o in trace if o["stream"] == 1]
                    graph = (options or {}).get("graph") and w.P == 1
                    if cs == 1 or graph:
                        assert not on1, what
                    if cs == 2 and w.C >= 2 and steps[0]["split"] and not scratch and not graph:
                        # stream 1 really carries the odd chunks (a schedule that serialises everything is not "safe", it is slow)
                        for o in launches:
                            chunks = steps[o["step"]]["launches"] // steps[o["step"]]["per_chunk"]
                            assert o["stream"] == (o["chunk"] & 1 if chunks > 1 else 0), what
                        assert on1, what
                    if scratch and {o["stream"] for o in launches if o["scratch"]} != {0}:
                        assert False, what + ": level-scratch launches on two streams"
                    if w.P1 > 1 and w.P2 > 1:      # the local world has concurrent channels
                        assert all(o["stream"] == (3 if o["which"] == 2 else 2) for o in trace if o["kind"] == EXCHANGE), what
                if -1 in by_cs and 1 in by_cs and 2 in by_cs:
                    assert by_cs[-1] == by_cs[2 if w.C >= 3 else 1]
    return n


def rows(classes, shapes):
    return [pytest.param(cls, P1, P2, shape, c2c, id=f"{cls.__name__[8:]}-{P1}x{P2}-{'x'.join(map(str, shape))}-{'c2c' if c2c else 'r2c'}")
            for cls in classes for P1, P2 in GRIDS for shape in shapes for c2c in (True, False) if fits(cls, shape, P1, P2, c2c)]


@pytest.mark.parametrize("cls,P1,P2,shape,c2c", rows(PENCIL + SLAB, SHAPES))
def test_every_chain_every_schedule(cls, P1, P2, shape, c2c):
    """the base rows: class x grid x shape x C2C / R2C, and inside: every rank x dims 3, 2, 1 x both directions x pipeline depths
    1 .. 5 (depths that do not divide the extents included; a depth the extents cannot hold is clipped by dfft_init) x compute_streams
    -1, 1, 2.  Nothing is thinned here; the combinations `fits` rules out would leave a rank without data."""
    depths = set()
    for C in DEPTHS:
        w = make_world(cls, shape, P1, P2, c2c, C)
        if w.C in depths:      # clipped to a depth already checked
            continue
        depths.add(w.C)
        assert check_world(w, shape) > 0


# Option rows, one option at a time on top of the base rows.  Thinned by this rule (the base rows are not): class MPIcuFFT_Pencil_Opt1
# (the slab class too where the option changes a slab chain: spectral_layout, two_level), shape (12, 10, 14) -- every axis length splits
# into two levels -- and (16, 16, 16), pipeline depths 1 and 4 (4 does not divide the extents of the first shape), compute_streams 1 and 2
# (the base rows assert that -1 is one of the two);
# single-rank options (mirror_inverse, single_order, graph) on the 1 x 1 grid, C2C, where they apply.
OPTION_DEPTHS = [1, 4]
OPTION_STREAMS = [1, 2]


@pytest.mark.parametrize("cls,P1,P2,shape,c2c", rows([dfft.MPIcuFFT_Pencil_Opt1, dfft.MPIcuFFT_Slab_Opt1], [(12, 10, 14), (16, 16, 16)]))
@pytest.mark.parametrize("option", ["spectral_layout", "two_level"])
def test_option_rows(cls, option, P1, P2, shape, c2c):
    for C in OPTION_DEPTHS:
        w = make_world(cls, shape, P1, P2, c2c, C, options={option: 1})
        assert check_world(w, shape, OPTION_STREAMS, {option: 1}, expect_scratch=option == "two_level") > 0


@pytest.mark.parametrize("shape", [(12, 10, 14), (16, 16, 16)])
@pytest.mark.parametrize("options", [{"mirror_inverse": 1}, {"single_order": 1}, {"single_order": 1, "mirror_inverse": 1}, {"graph": 1}, {"single_order": 0}])
def test_single_rank_option_rows(options, shape):
    for C in OPTION_DEPTHS:
        w = make_world(dfft.MPIcuFFT_Pencil_Opt1, shape, 1, 1, True, C, options=options)
        assert w.single == (options.get("single_order") == 1)
        assert check_world(w, shape, OPTION_STREAMS, options) > 0
        if options.get("graph"):      # run_graphed captures the plan's stream alone
            w.plans[0].setOption("compute_streams", 2)
            assert {o["stream"] for d in (F, I) for o in w.plans[0].debugTrace(d)} == {0}


@pytest.mark.parametrize("c2c", [True, False])
@pytest.mark.parametrize("shape,P1,P2", [((2, 4, 4099), 1, 1), ((2, 4, 4099), 2, 1), ((4, 2, 4099), 1, 2), ((4, 4099, 2), 2, 2)])
def test_long_bluestein_axis_shares_the_level_scratch(shape, P1, P2, c2c):
    """one axis of 4099 points (a prime above 4096: Bluestein over a two-level padded length, four launches through the level scratch)"""
    assert dfft.axis_plan_info(4099)["kind"] == "long_bluestein"
    for C in (1, 3):
        w = make_world(dfft.MPIcuFFT_Pencil_Opt1, shape, P1, P2, c2c, C)
        assert check_world(w, shape, OPTION_STREAMS, None, expect_scratch=True) > 0


def test_compute_streams_set_after_init_takes_effect_at_the_next_exec():
    """the trace says what the next exec does (include/dfft_c.h: "compute_streams" is read at every exec)"""
    w = make_world(dfft.MPIcuFFT_Pencil_Opt1, (12, 10, 14), 2, 2, True, 2)
    pl = w.plans[0]
    assert pl.getOption("compute_streams") == -1 and all(o["stream"] != 1 for o in pl.debugTrace(F))      # two chunks: one stream by default
    pl.setOption("compute_streams", 2)
    assert {o["chunk"] for o in pl.debugTrace(F) if o["stream"] == 1 and o["kind"] == LAUNCH} == {1}
    pl.setOption("compute_streams", 1)
    assert all(o["stream"] != 1 for o in pl.debugTrace(F))
    assert pl.debugTrace(F, 0) == []      # nothing was executed with option trace


def test_trace_is_the_same_with_the_relay_on():
    """the relay's staging and side stream are inside the exchange (comm.hip's contract), not in the plan's schedule"""
    traces = []
    for relay in (0, 3):
        comm = dfft.Comm.local(8)
        comm.setOption("relay", relay)
        pl = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), comm, precision="double", rank=3)
        pl.setPipelineChunks(3)
        pl.initFFT(dfft.GlobalSize(12, 10, 14), dfft.Partition(2, 4), allocate=False, c2c=True)
        traces.append([pl.debugTrace(d) for d in (F, I)])
    assert traces[0] == traces[1] and len(traces[0][0]) > 10
