"""The chain of execSpectralSum (option "spectral_inputs" = K >= 2, include/dfft_c.h: dfft_exec_spectral_sum) without a GPU: K forward
halves, z -> ex1 -> y -> ex2 -> xx, triple j with the buffer and the operator of input j, the xx launches of inputs j >= 1 ADDING to
the accumulator slice A that xx of input 0 stored; then one inverse half, ex2^-1 -> y^-1 -> ex1^-1 -> z^-1.

Data flow: the library's own steps (debugChain(SPECTRAL_SUM)) replayed like tests/test_cpu_spectral_multi.py's run_multi, every xx step
with the multiplier of its input and `+=` where its form is 6.  Schedule: the executor's trace (debugTrace(SPECTRAL_SUM)) against the
footprints of its launches and exchanges (tests/schedule_check.py, rules 1-5), an accumulating launch reading its destination as well.
The rows are those of test_cpu_spectral_op.py."""
import numpy as np
import pytest

import distributedfft_amd as dfft
import schedule_check as sc
from layout_sim import MODES, Pass, World
from schedule_check import EXCHANGE, LAUNCH
from test_cpu_spectral_op import DEPTHS, PENCIL, ROWS, SpectralFootprints, multiplier

F, I, S, M, Q = dfft.FORWARD, dfft.INVERSE, dfft.SPECTRAL_OP, dfft.SPECTRAL_OPS, dfft.SPECTRAL_SUM
VALUES = [2, 3]      # of the option
ACC = 6              # dfft_chain_step::form of an accumulating xx step


def world(cls, shape, P1, P2, c2c, chunks, spectral, K, op=1, outputs=None):
    options = {"spectral_op": op, "spectral_layout": spectral}
    if K is not None:
        options["spectral_inputs"] = K
    if outputs is not None:
        options["spectral_outputs"] = outputs
    return World(cls, shape, P1, P2, c2c, chunks, options=options)


def in_index(b):
    """the input a buffer number of dfft_chain_step / dfft_trace_op names: -2 is input 0, -(9 + j) input j >= 1; else None"""
    return 0 if b == -2 else -b - 9 if b <= -10 else None


def field(shape, c2c, seed):
    rng = np.random.default_rng(seed)
    u = rng.uniform(0, 255, shape) - 127.5
    return u + 1j * (rng.uniform(0, 255, shape) - 127.5) if c2c else u


def blocks(w, us, mults):
    """per input and rank: the flat input block and the multiplier block (Nx, yo, zs); per rank: the expected block of the sum"""
    n = int(np.prod(w.shape))
    term = lambda u, m: np.fft.ifftn(np.fft.fftn(u) * m) * n if w.c2c else np.fft.irfftn(np.fft.rfftn(u) * m, s=w.shape, axes=(0, 1, 2)) * n      # noqa: E731
    full = sum(term(u, m) for u, m in zip(us, mults))
    ins, ms, wants = [[] for _ in us], [[] for _ in us], []
    for pl in w.plans:
        (nx, ny, nz), (x0, y0, z0) = pl.getInSize(), pl.getInStart()
        (_, ky, kz), (_, k0, kz0) = pl.getOutSize(), pl.getOutStart()
        wants.append(full[x0:x0 + nx, y0:y0 + ny, z0:z0 + nz])
        for j, (u, m) in enumerate(zip(us, mults)):
            ins[j].append(np.ascontiguousarray(u[x0:x0 + nx, y0:y0 + ny, z0:z0 + nz]).ravel().copy())
            ms[j].append(m[:, k0:k0 + ky, kz0:kz0 + kz])
    return ins, ms, wants


def accumulator(steps):
    return steps[2]["dst"]


def run_sum(w, ins, ms):
    """one execSpectralSum on every rank, step by step; ins[j][r], ms[j][r]: input and multiplier block of input j on rank r.
    Returns out[r]"""
    steps = w.plans[0].debugChain(Q)
    assert all(pl.debugChain(Q) == steps for pl in w.plans[1:])
    K = len(ms)
    assert len(steps) == 3 * K + 2
    Nx = w.shape[0]
    length = (w.shape[2], w.shape[1], w.shape[0])
    size = [int(np.prod(pl.getInSize())) for pl in w.plans]
    out = [np.full(n, np.nan, dtype=np.complex128 if w.c2c else np.float64) for n in size]
    keep = [[a.copy() for a in row] for row in ins]
    W = w.buffers(1 + max(b for s in steps for b in (s["src"], s["dst"])))
    buf = lambda b: out if b == -1 else ins[in_index(b)] if b < 0 else [W[r][b] for r in range(w.P)]      # noqa: E731
    A = accumulator(steps)
    for i, s in enumerate(steps):
        j = min(i // 3, K - 1)      # the input the step belongs to
        assert s["src"] != -1 and in_index(s["dst"]) is None, "`out` is never read, no input is ever written"
        assert (s["dst"] == -1) == (i == len(steps) - 1), "only z^-1 writes `out`"
        assert (in_index(s["src"]) is not None) == (i < 3 * K and i % 3 == 0), "only the z pass of a triple reads an input"
        if 2 <= i < 3 * K:      # from the first xx to the inverse y pass nothing but the xx steps writes the accumulator
            touches = s["dst"] == A or (s["exchange"] and steps[i + 1]["src"] == A)
            assert touches == (s["group"] == "xx"), (i, s)
            assert s["src"] != A, (i, s)
        src, dst, per = buf(s["src"]), buf(s["dst"]), s["per_chunk"]
        for c in range(s["launches"] // per):
            for r, pl in enumerate(w.plans):
                for k in range(c * per, (c + 1) * per):
                    p = Pass(pl, s["group"], k)
                    if s["group"] != "xx":
                        p.run(src[r], dst[r], length[s["axis"]], MODES[s["form"]])
                        continue
                    assert s["form"] in (2, ACC)
                    k0 = sum(pl.debugPass("xx", q).na for q in range(k))      # first ky row of the chunk
                    for a in range(p.d.na):
                        for line in range(p.d.LB):
                            x = src[r][p.load_offset(a, line, np.arange(Nx), Nx)]
                            y = np.fft.ifft(np.fft.fft(x) * ms[j][r][:, k0 + a, line]) * Nx
                            at = p.store_offset(a, line, np.arange(Nx), Nx)
                            dst[r][at] = dst[r][at] + y if s["form"] == ACC else y
            if s["exchange"]:
                w.exchange(s["tables"], s["exchange"], c, dst, buf(steps[i + 1]["src"]))
    for row, krow in zip(ins, keep):
        for a, b in zip(row, krow):
            assert np.array_equal(a, b), "an input changed"
    return out


@pytest.mark.parametrize("K", VALUES)
@pytest.mark.parametrize("cls,P1,P2,shape,c2c,spectral", ROWS)
def test_data_flow(cls, P1, P2, shape, c2c, spectral, K):
    us = [field(shape, c2c, 11 + j) for j in range(K)]
    mults = [multiplier(shape, c2c, seed=7 + j) for j in range(K)]
    for C in DEPTHS:
        w = world(cls, shape, P1, P2, c2c, C, spectral, K)
        ins, ms, wants = blocks(w, us, mults)
        out = run_sum(w, ins, ms)
        for r in range(w.P):
            got = out[r].reshape(wants[r].shape)
            assert not np.isnan(got).any(), f"rank {r}, depth {w.C}: NaN from a work slice reached the output"
            err = np.abs(got - wants[r]).max() / np.abs(wants[r]).max()
            assert err <= 1e-9, f"rank {r}, depth {w.C}: {err}"


@pytest.mark.parametrize("K", VALUES)
@pytest.mark.parametrize("cls,P1,P2,shape,c2c,spectral", ROWS)
def test_shape_of_the_chain(cls, P1, P2, shape, c2c, spectral, K):
    x1, x2 = int(P2 > 1), 2 * int(P1 > 1)
    top = lambda st: max(b for s in st for b in (s["src"], s["dst"]))      # noqa: E731
    for C in DEPTHS:
        w = world(cls, shape, P1, P2, c2c, C, spectral, K)
        for pl in w.plans:
            single, steps = pl.debugChain(S), pl.debugChain(Q)
            assert [s["group"] for s in steps] == ["fz", "fy", "xx"] * K + ["iy", "iz"]
            assert [s["form"] for s in steps if s["group"] == "xx"] == [2] + [ACC] * (K - 1)
            assert [s["tables"] for s in steps] == [F, F, I] * K + [I, I]
            assert [s["exchange"] for s in steps] == [x1, x2, 0] * (K - 1) + [x1, x2, x2] + [x1, 0]      # exchange 2 backwards: after the last xx only
            assert [s["src"] for s in steps if s["src"] < 0] == [-2] + [-(9 + j) for j in range(1, K)]
            assert [i for i, s in enumerate(steps) if s["src"] < 0] == [3 * j for j in range(K)]
            assert [s["dst"] for s in steps if s["dst"] < 0] == [-1] and steps[-1]["dst"] == -1
            assert all(s["launches"] == w.C and s["per_chunk"] == 1 for s in steps if s["group"] == "xx")
            # the forward half of every input and the inverse half are the single chain's, but for the accumulator in the place of xx's dst
            A = accumulator(steps)
            assert all(s["dst"] == A for s in steps if s["group"] == "xx")
            for j in range(K):
                assert [dict(s, src=0) for s in steps[3 * j:3 * j + 2]] == [dict(s, src=0) for s in single[:2]]
                assert steps[3 * j + 2]["src"] == single[2]["src"]
            assert [s["dst"] for s in steps[-2:]] == [s["dst"] for s in single[-2:]] and steps[-1]["src"] == single[-1]["src"]
            # one slice above the single chain's in every grid class, and exactly the work area says so
            assert A == top(steps) == top(single) + 1 == int(P1 > 1) + int(P2 > 1) + 2
            assert (top(steps) + 1) * pl.getDomainSize() <= pl.getWorkSizeDevice()


# ---- schedule ------------------------------------------------------------------------------------------------------------------
class SumFootprints(SpectralFootprints):
    """every input is a buffer of its own: "in" for input 0 (as schedule_check names it), "in<j>" for input j >= 1; an accumulating
    launch (form 6) has the footprint of the plain one (form 2) and READS what it writes as well"""

    def where(self, b, idx):
        return (f"in{-b - 9}", idx) if b <= -10 else super().where(b, idx)

    def launch(self, st, k):
        return super().launch(dict(st, form=2) if st["form"] == ACC else st, k)

    def of(self, direction, steps):
        plain = super().of(direction, steps)

        def footprint(i, op):
            reads, writes = plain(i, op)
            # the caller's inputs hold data before the chain starts and nothing in the chain writes them (asserted in test_schedule):
            # schedule_check knows that of "in" alone, so the reads of the further inputs are left out of the footprint
            reads = {b: idx for b, idx in reads.items() if not (b.startswith("in") and b != "in")}
            if op["kind"] == LAUNCH and steps[op["step"]]["form"] == ACC:
                (rb, ri), = reads.items()
                (wb, wi), = writes.items()
                assert rb == wb == "W" and not np.intersect1d(ri, wi).size, "the accumulating launch loads from one slice and stores to another"
                reads = {rb: np.concatenate([ri, wi])}
            return reads, writes
        return footprint


def check(trace, steps, footprint):
    """schedule_check.check for a chain with accumulating launches.  Rule 3 reports every launch that writes elements it reads itself,
    because the workgroups of a launch are not ordered; an accumulating launch does so on purpose and safely -- every element of its
    destination is read and then written by one lane of one workgroup, and what it LOADS through its source side is another slice
    (asserted in SumFootprints.of) -- so that one finding about such a launch and itself is taken out, and nothing else"""
    own = lambda v: v.rule == 3 and v.a == v.b and trace[v.a]["kind"] == LAUNCH and steps[trace[v.a]["step"]]["form"] == ACC      # noqa: E731
    return [v for v in sc.check(trace, steps, footprint) if not own(v)]


@pytest.mark.parametrize("K", VALUES)
@pytest.mark.parametrize("cls,P1,P2,shape,c2c,spectral", ROWS)
def test_schedule(cls, P1, P2, shape, c2c, spectral, K):
    for C in DEPTHS:
        w = world(cls, shape, P1, P2, c2c, C, spectral, K)
        for r, pl in enumerate(w.plans):
            fps = SumFootprints(pl, shape)
            steps = pl.debugChain(Q)
            for cs in (1, 2):
                pl.setOption("compute_streams", cs)
                trace = pl.debugTrace(Q)
                what = f"rank {r} depth {w.C} compute_streams {cs}"
                bad = sorted(check(trace, steps, fps.of(Q, steps)), key=lambda v: v.rule not in (3, 4))
                assert not bad, f"{what}: {len(bad)} violations\n" + "\n".join(repr(v) for v in bad[:10])
                launches = [o for o in trace if o["kind"] == LAUNCH]
                assert len(launches) == sum(s["launches"] for s in steps) > 0, what
                assert not any(o["scratch"] for o in launches), what
                assert not any(o["dst"] < 0 for o in trace if o["kind"] == EXCHANGE), what
                assert not any(in_index(o["dst"]) is not None for o in trace if o["kind"] in (LAUNCH, EXCHANGE)), what + ": an input is written"
                assert [o["step"] for o in launches if o["dst"] == -1] == [3 * K + 1] * steps[-1]["launches"], what
                for j in range(K):      # input j is read by the launches of its own z step and by nothing else
                    assert [o["step"] for o in trace if o["kind"] in (LAUNCH, EXCHANGE) and in_index(o["src"]) == j] == [3 * j] * steps[3 * j]["launches"], what
                if cs == 1:
                    assert not [o for o in trace if o["stream"] == 1], what
                elif w.C >= 2:
                    assert all(o["stream"] == (o["chunk"] & 1) for o in launches), what


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 2)])
def test_a_trace_that_accumulates_before_the_first_store_is_caught(P1, P2, C):
    """Negative control of the checker on this chain.  The hand-made trace exchanges two launches of the executor's trace: the last chunk
    of xx of input 1, which accumulates, takes the place of the same chunk of xx of input 0, which stores, and the other way round.  The
    accumulating launch then reads elements of the accumulator that nothing has written yet (rule 4), and every finding must be about
    the two exchanged launches alone."""
    shape, XX0, XX1 = (8, 10, 38), 2, 5
    pl = world(PENCIL, shape, P1, P2, False, C, 0, 2).plans[0]
    pl.setOption("compute_streams", 1)
    steps, trace = pl.debugChain(Q), pl.debugTrace(Q)
    assert steps[XX0]["form"] == 2 and steps[XX1]["form"] == ACC and steps[XX0]["dst"] == steps[XX1]["dst"]
    fps = SumFootprints(pl, shape)
    assert not check(trace, steps, fps.of(Q, steps))
    c = pl.getPipelineChunks() - 1
    at = {o["step"]: i for i, o in enumerate(trace) if o["kind"] == LAUNCH and o["chunk"] == c and o["step"] in (XX0, XX1)}
    hand = list(trace)
    hand[at[XX0]], hand[at[XX1]] = trace[at[XX1]], trace[at[XX0]]
    bad = check(hand, steps, fps.of(Q, steps))
    assert any(v.rule == 4 and v.a is None and v.b == at[XX0] for v in bad), "the read of the unwritten accumulator was not reported"
    for v in bad:
        assert {hand[i]["step"] for i in (v.a, v.b) if i is not None} <= {XX0, XX1}, repr(v)


# ---- the default, the cost, error paths ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 2)])
@pytest.mark.parametrize("c2c", [True, False])
def test_value_1_changes_nothing(P1, P2, c2c):
    shape = (16, 12, 14)
    for op in (0, 1):
        plain = world(PENCIL, shape, P1, P2, c2c, 3, 0, None, op=op)      # a plan that never heard of the option
        one = world(PENCIL, shape, P1, P2, c2c, 3, 0, 1, op=op)
        for a, b in zip(plain.plans, one.plans):
            assert b.getOption("spectral_inputs") == 1 == a.getOption("spectral_inputs")
            assert a.getWorkSizeDevice() == b.getWorkSizeDevice()
            for d in (F, I, S, M):
                assert a.debugChain(d) == b.debugChain(d)
                assert a.debugTrace(d) == b.debugTrace(d)
            assert (a.debugChain(S) != []) == bool(op)
            for pl in (a, b):
                assert pl.debugChain(Q) == [] and pl.debugTrace(Q) == [] and pl.debugTrace(Q, 0) == []
                with pytest.raises(dfft.DfftError, match="error 3.*set spectral_inputs before dfft_init"):      # ERR_STATE
                    pl.execSpectralSum(1, [2, 3], [dict(tables=(4, 5, 6)), dict(tables=(4, 5, 6))])


@pytest.mark.parametrize("cls,P1,P2,shape,c2c,spectral", ROWS)
def test_cost_is_one_slice_whatever_the_value(cls, P1, P2, shape, c2c, spectral):
    sizes, both = {}, {}
    for K in (1, 2, 3, 8):
        w = world(cls, shape, P1, P2, c2c, 3, spectral, K)
        sizes[K] = [pl.getWorkSizeDevice() for pl in w.plans]
        domain = [pl.getDomainSize() for pl in w.plans]      # a slice: the domain rounded up to 256 bytes, as the plan rounds it
    assert all(d % 256 == 0 for d in domain)
    assert [a - b for a, b in zip(sizes[3], sizes[1])] == domain
    assert sizes[2] == sizes[3] == sizes[8]
    # with spectral_outputs set as well the two chains share the slice: still one above the plan with neither
    for K, outputs in ((3, 2), (2, 8)):
        w = world(cls, shape, P1, P2, c2c, 3, spectral, K, outputs=outputs)
        both = [pl.getWorkSizeDevice() for pl in w.plans]
        assert both == sizes[3]
        for pl in w.plans:
            top = max(b for d in (M, Q) for s in pl.debugChain(d) for b in (s["src"], s["dst"]))
            assert (top + 1) * pl.getDomainSize() <= pl.getWorkSizeDevice()


def test_bad_values_fail_at_init():
    def init(**options):
        pl = PENCIL(dfft.Configurations(), None, rank=0)
        for k, v in options.items():
            pl.setOption(k, v)
        pl.initFFT(dfft.GlobalSize(16, 12, 14), dfft.Partition(1, 1), allocate=False)
        return pl
    for v in (0, 9, -1):
        with pytest.raises(dfft.DfftError, match="error 2.*spectral_inputs"):      # ERR_ARG
            init(spectral_op=1, spectral_inputs=v)
    with pytest.raises(dfft.DfftError, match="error 2.*spectral_inputs.*spectral_op"):
        init(spectral_inputs=2)
    for v in (1, 2, 8):
        assert len(init(spectral_op=1, spectral_inputs=v).debugChain(Q)) == (0 if v == 1 else 3 * v + 2)


def test_operator_keywords_are_those_of_execSpectralOp():
    pl = world(PENCIL, (16, 12, 14), 1, 1, True, 1, 0, 2).plans[0]
    with pytest.raises(dfft.DfftError, match="one operator per input"):
        pl.execSpectralSum(1, [2, 3], [dict(tables=(4, 5, 6))])
    with pytest.raises(dfft.DfftError, match="unknown operator keyword table"):
        pl.execSpectralSum(1, [3], [dict(table=(4, 5, 6))])
    with pytest.raises(dfft.DfftError, match="either multiplier= or tables= / factors="):
        pl.execSpectralSum(1, [3], [dict(scale=2.0)])
    with pytest.raises(dfft.DfftError, match="reciprocal=True needs tables="):
        pl.execSpectralSum(1, [3], [dict(factors=(4, None, None), reciprocal=True)])
