"""The chain of execSpectralOps (option "spectral_outputs" = K >= 2, include/dfft_c.h: dfft_exec_spectral_ops) without a GPU: one
forward half, z -> ex1 -> y -> ex2, then K times xx -> ex2^-1 -> y^-1 -> ex1^-1 -> z^-1, triple j with the operator and the buffer of
output j.

Data flow: the library's own steps (debugChain(SPECTRAL_OPS)) replayed like tests/test_cpu_spectral_op.py's run_spectral, every xx
step with the multiplier of its output.  Schedule: the executor's trace (debugTrace(SPECTRAL_OPS)) against the footprints of its
launches and exchanges (tests/schedule_check.py, rules 1-5), every output a buffer of its own.  The rows are those of
test_cpu_spectral_op.py."""
import numpy as np
import pytest

import distributedfft_amd as dfft
import schedule_check as sc
from layout_sim import MODES, Pass, World
from schedule_check import EXCHANGE, LAUNCH, RECORD, WAIT
from test_cpu_spectral_op import DEPTHS, PENCIL, ROWS, SpectralFootprints, multiplier

F, I, S, M = dfft.FORWARD, dfft.INVERSE, dfft.SPECTRAL_OP, dfft.SPECTRAL_OPS
VALUES = [2, 3]      # of the option


def world(cls, shape, P1, P2, c2c, chunks, spectral, K, op=1):
    options = {"spectral_op": op, "spectral_layout": spectral}
    if K is not None:
        options["spectral_outputs"] = K
    return World(cls, shape, P1, P2, c2c, chunks, options=options)


def out_index(b):
    """the output a buffer number of dfft_chain_step / dfft_trace_op names: -1 is output 0, -(2 + j) output j >= 1; else None"""
    return 0 if b == -1 else -b - 2 if b <= -3 else None


def field(shape, c2c, seed=11):
    rng = np.random.default_rng(seed)
    u = rng.uniform(0, 255, shape) - 127.5
    return u + 1j * (rng.uniform(0, 255, shape) - 127.5) if c2c else u


def blocks(w, u, mults):
    """per rank: the flat input block; per output and rank: the multiplier block (Nx, yo, zs) and the expected output block"""
    n = int(np.prod(w.shape))
    fulls = [np.fft.ifftn(np.fft.fftn(u) * m) * n if w.c2c else np.fft.irfftn(np.fft.rfftn(u) * m, s=w.shape, axes=(0, 1, 2)) * n for m in mults]
    ins, ms, wants = [], [[] for _ in mults], [[] for _ in mults]
    for pl in w.plans:
        (nx, ny, nz), (x0, y0, z0) = pl.getInSize(), pl.getInStart()
        ins.append(np.ascontiguousarray(u[x0:x0 + nx, y0:y0 + ny, z0:z0 + nz]).ravel().copy())
        (_, ky, kz), (_, k0, kz0) = pl.getOutSize(), pl.getOutStart()
        for j, m in enumerate(mults):
            wants[j].append(fulls[j][x0:x0 + nx, y0:y0 + ny, z0:z0 + nz])
            ms[j].append(m[:, k0:k0 + ky, kz0:kz0 + kz])
    return ins, ms, wants


def run_multi(w, ins, ms):
    """one execSpectralOps on every rank, step by step; ms[j][r]: the multiplier block of output j on rank r.  Returns outs[j][r]"""
    steps = w.plans[0].debugChain(M)
    assert all(pl.debugChain(M) == steps for pl in w.plans[1:])
    K = len(ms)
    assert len(steps) == 2 + 3 * K
    Nx = w.shape[0]
    length = (w.shape[2], w.shape[1], w.shape[0])
    nin = [int(np.prod(pl.getInSize())) for pl in w.plans]
    outs = [[np.full(n, np.nan, dtype=np.complex128 if w.c2c else np.float64) for n in nin] for _ in range(K)]
    keep = [a.copy() for a in ins]
    W = w.buffers(1 + max(b for s in steps for b in (s["src"], s["dst"])))
    buf = lambda b: ins if b == -2 else outs[out_index(b)] if b < 0 else [W[r][b] for r in range(w.P)]      # noqa: E731
    xsrc = steps[2]["src"]
    for i, s in enumerate(steps):
        j = max(0, i - 2) // 3      # the output the step belongs to
        assert s["src"] >= -2 and s["dst"] != -2      # `in` is never written, no output is ever read
        assert (out_index(s["dst"]) is not None) == (i >= 2 and (i - 2) % 3 == 2), "only the last step of a triple writes an output"
        if i >= 2:      # nothing writes the slice xx reads once the forward half has filled it
            assert s["dst"] != xsrc and not (s["exchange"] and steps[i + 1]["src"] == xsrc), (i, s)
        src, dst, per = buf(s["src"]), buf(s["dst"]), s["per_chunk"]
        for c in range(s["launches"] // per):
            for r, pl in enumerate(w.plans):
                for k in range(c * per, (c + 1) * per):
                    p = Pass(pl, s["group"], k)
                    if s["group"] != "xx":
                        p.run(src[r], dst[r], length[s["axis"]], MODES[s["form"]])
                        continue
                    k0 = sum(pl.debugPass("xx", q).na for q in range(k))      # first ky row of the chunk
                    for a in range(p.d.na):
                        for line in range(p.d.LB):
                            x = src[r][p.load_offset(a, line, np.arange(Nx), Nx)]
                            y = np.fft.ifft(np.fft.fft(x) * ms[j][r][:, k0 + a, line]) * Nx
                            dst[r][p.store_offset(a, line, np.arange(Nx), Nx)] = y
            if s["exchange"]:
                w.exchange(s["tables"], s["exchange"], c, dst, buf(steps[i + 1]["src"]))
    for a, b in zip(ins, keep):
        assert np.array_equal(a, b), "`in` changed"
    return outs


@pytest.mark.parametrize("K", VALUES)
@pytest.mark.parametrize("cls,P1,P2,shape,c2c,spectral", ROWS)
def test_data_flow(cls, P1, P2, shape, c2c, spectral, K):
    u = field(shape, c2c)
    mults = [multiplier(shape, c2c, seed=7 + j) for j in range(K)]
    for C in DEPTHS:
        w = world(cls, shape, P1, P2, c2c, C, spectral, K)
        ins, ms, wants = blocks(w, u, mults)
        outs = run_multi(w, ins, ms)
        for j in range(K):
            for r in range(w.P):
                got = outs[j][r].reshape(wants[j][r].shape)
                assert not np.isnan(got).any(), f"output {j}, rank {r}, depth {w.C}: NaN from a work slice reached the output"
                err = np.abs(got - wants[j][r]).max() / np.abs(wants[j][r]).max()
                assert err <= 1e-9, f"output {j}, rank {r}, depth {w.C}: {err}"


@pytest.mark.parametrize("K", VALUES)
@pytest.mark.parametrize("cls,P1,P2,shape,c2c,spectral", ROWS)
def test_shape_of_the_chain(cls, P1, P2, shape, c2c, spectral, K):
    x1, x2 = int(P2 > 1), 2 * int(P1 > 1)
    for C in DEPTHS:
        w = world(cls, shape, P1, P2, c2c, C, spectral, K)
        single = w.plans[0].debugChain(S)
        for pl in w.plans:
            steps = pl.debugChain(M)
            assert [s["group"] for s in steps] == ["fz", "fy"] + ["xx", "iy", "iz"] * K
            assert [s["tables"] for s in steps] == [F, F] + [I] * (3 * K)
            assert [s["exchange"] for s in steps] == [x1, x2] + [x2, x1, 0] * K
            assert [s["dst"] for s in steps if s["dst"] < 0] == [-1] + [-(2 + j) for j in range(1, K)]
            assert [i for i, s in enumerate(steps) if s["dst"] < 0] == [4 + 3 * j for j in range(K)]
            assert all(s["launches"] == w.C and s["per_chunk"] == 1 for s in steps if s["group"] == "xx")
            # the slices do not depend on the output, so fewer outputs are a prefix of the chain
            for j in range(1, K):
                assert [dict(s, dst=0) for s in steps[2:5]] == [dict(s, dst=0) for s in steps[2 + 3 * j:5 + 3 * j]]
            # at most one slice more than the single-output chain, and exactly the work area says so
            top = lambda st: max(b for s in st for b in (s["src"], s["dst"]))      # noqa: E731
            assert top(steps) - top(single) == (0 if P1 > 1 and P2 > 1 else 1)
            assert (top(steps) + 1) * pl.getDomainSize() <= pl.getWorkSizeDevice()


# ---- schedule ------------------------------------------------------------------------------------------------------------------
class MultiFootprints(SpectralFootprints):
    """every output is a buffer of its own: "out" for output 0 (as schedule_check names it), "out<j>" for output j >= 1"""

    def where(self, b, idx):
        return (f"out{-b - 2}", idx) if b <= -3 else super().where(b, idx)


@pytest.mark.parametrize("K", VALUES)
@pytest.mark.parametrize("cls,P1,P2,shape,c2c,spectral", ROWS)
def test_schedule(cls, P1, P2, shape, c2c, spectral, K):
    for C in DEPTHS:
        w = world(cls, shape, P1, P2, c2c, C, spectral, K)
        for r, pl in enumerate(w.plans):
            fps = MultiFootprints(pl, shape)
            steps = pl.debugChain(M)
            for cs in (1, 2):
                pl.setOption("compute_streams", cs)
                trace = pl.debugTrace(M)
                what = f"rank {r} depth {w.C} compute_streams {cs}"
                bad = sorted(sc.check(trace, steps, fps.of(M, steps)), key=lambda v: v.rule not in (3, 4))
                assert not bad, f"{what}: {len(bad)} violations\n" + "\n".join(repr(v) for v in bad[:10])
                launches = [o for o in trace if o["kind"] == LAUNCH]
                assert len(launches) == sum(s["launches"] for s in steps) > 0, what
                assert not any(o["scratch"] for o in launches), what
                assert all(o["src"] >= -2 and o["dst"] != -2 for o in trace if o["kind"] in (LAUNCH, EXCHANGE)), what
                assert not any(o["dst"] < 0 for o in trace if o["kind"] == EXCHANGE), what
                for j in range(K):      # output j is written by the launches of its own z^-1 step and by nothing else
                    assert [o["step"] for o in launches if out_index(o["dst"]) == j] == [4 + 3 * j] * steps[4 + 3 * j]["launches"], what
                if cs == 1:
                    assert not [o for o in trace if o["stream"] == 1], what
                elif w.C >= 2:
                    assert all(o["stream"] == (o["chunk"] & 1) for o in launches), what
                if P1 > 1 and P2 > 1:
                    assert all(o["stream"] == (3 if o["which"] == 2 else 2) for o in trace if o["kind"] == EXCHANGE), what


@pytest.mark.parametrize("P1,P2", [(2, 2), (2, 3)])
def test_a_trace_that_starts_xx_of_output_1_before_iz_of_output_0_is_caught(P1, P2):
    """Negative control of the checker on this chain.  On a P1 x P2 pencil xx of output 1 writes the slice z^-1 of output 0 reads; the
    executor orders them because xx waits for the whole step before it.  The hand-made trace here takes exactly that edge away: the xx
    launch of output 1 moves to a stream of its own behind an event recorded just before z^-1 of output 0 starts (so it still follows
    everything up to y^-1 of output 0 and its exchange), and the caller's stream waits for it before it goes on.  Every violation must
    then be one of rule 3 between steps 4 (z^-1 of output 0) and 5 (xx of output 1).
    On every other grid (one rank, slab, 1 x P2) z^-1 reads the slice F that only y^-1 / exchange 1 backwards write, and xx writes
    another one: the two steps share no slice, there is nothing for this control to catch, and the second half of the test asserts just
    that instead."""
    shape, IZ0, XX1 = (8, 10, 38), 4, 5
    pl = world(PENCIL, shape, P1, P2, False, 1, 0, 2).plans[0]
    pl.setOption("compute_streams", 1)
    steps, trace = pl.debugChain(M), pl.debugTrace(M)
    assert steps[XX1]["dst"] == steps[IZ0]["src"] and steps[XX1]["launches"] == 1
    fps = MultiFootprints(pl, shape)
    assert not sc.check(trace, steps, fps.of(M, steps))
    e1 = 1 + max(o["event"] for o in trace)
    sync = lambda kind, stream, event: dict(kind=kind, stream=stream, event=event, step=-1, chunk=-1, launch=-1, src=-1, dst=-1, which=0, scratch=0)      # noqa: E731
    hand = []
    for i, o in enumerate(trace):
        first_iz0 = o["kind"] == LAUNCH and o["step"] == IZ0 and not any(q["kind"] == LAUNCH and q["step"] == IZ0 for q in trace[:i])
        if first_iz0:
            hand.append(sync(RECORD, 0, e1))
        if o["kind"] == LAUNCH and o["step"] == XX1:
            hand += [sync(WAIT, 1, e1), dict(o, stream=1), sync(RECORD, 1, e1 + 1), sync(WAIT, 0, e1 + 1)]
        else:
            hand.append(o)
    bad = sc.check(hand, steps, fps.of(M, steps))
    assert bad
    for v in bad:
        assert v.rule == 3 and {hand[v.a]["step"], hand[v.b]["step"]} == {IZ0, XX1}, repr(v)
    for Q1, Q2 in [(1, 1), (2, 1), (1, 2)]:
        st = world(PENCIL, shape, Q1, Q2, False, 1, 0, 2).plans[0].debugChain(M)
        assert st[XX1]["dst"] != st[IZ0]["src"] and st[XX1]["src"] != st[IZ0]["src"]


# ---- the default, the cost, error paths ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 2)])
@pytest.mark.parametrize("c2c", [True, False])
def test_value_1_changes_nothing(P1, P2, c2c):
    shape = (16, 12, 14)
    for op in (0, 1):
        plain = world(PENCIL, shape, P1, P2, c2c, 3, 0, None, op=op)      # a plan that never heard of the option
        one = world(PENCIL, shape, P1, P2, c2c, 3, 0, 1, op=op)
        for a, b in zip(plain.plans, one.plans):
            assert b.getOption("spectral_outputs") == 1 == a.getOption("spectral_outputs")
            assert a.getWorkSizeDevice() == b.getWorkSizeDevice()
            for d in (F, I, S):
                assert a.debugChain(d) == b.debugChain(d)
                assert a.debugTrace(d) == b.debugTrace(d)
            assert (a.debugChain(S) != []) == bool(op)
            for pl in (a, b):
                assert pl.debugChain(M) == [] and pl.debugTrace(M) == [] and pl.debugTrace(M, 0) == []
                with pytest.raises(dfft.DfftError, match="error 3.*set spectral_outputs before dfft_init"):      # ERR_STATE
                    pl.execSpectralOps([1, 2], 3, [dict(multiplier=4), dict(multiplier=5)])


@pytest.mark.parametrize("cls,P1,P2,shape,c2c,spectral", ROWS)
def test_cost_is_at_most_one_slice_whatever_the_value(cls, P1, P2, shape, c2c, spectral):
    sizes = {}
    for K in (1, 2, 3, 8):
        w = world(cls, shape, P1, P2, c2c, 3, spectral, K)
        sizes[K] = [pl.getWorkSizeDevice() for pl in w.plans]
        domain = [pl.getDomainSize() for pl in w.plans]      # a slice: the domain rounded up to 256 bytes, as the plan rounds it
    assert all(d % 256 == 0 for d in domain)
    extra = [a - b for a, b in zip(sizes[3], sizes[1])]
    assert extra == ([0] * w.P if P1 > 1 and P2 > 1 else domain)
    assert sizes[2] == sizes[3] == sizes[8]


def test_bad_values_fail_at_init():
    def init(**options):
        pl = PENCIL(dfft.Configurations(), None, rank=0)
        for k, v in options.items():
            pl.setOption(k, v)
        pl.initFFT(dfft.GlobalSize(16, 12, 14), dfft.Partition(1, 1), allocate=False)
        return pl
    for v in (0, 9, -1):
        with pytest.raises(dfft.DfftError, match="error 2.*spectral_outputs"):      # ERR_ARG
            init(spectral_op=1, spectral_outputs=v)
    with pytest.raises(dfft.DfftError, match="error 2.*spectral_outputs.*spectral_op"):
        init(spectral_outputs=2)
    for v in (1, 2, 8):
        assert len(init(spectral_op=1, spectral_outputs=v).debugChain(M)) == (0 if v == 1 else 2 + 3 * v)


def test_operator_keywords_are_those_of_execSpectralOp():
    pl = world(PENCIL, (16, 12, 14), 1, 1, True, 1, 0, 2).plans[0]
    with pytest.raises(dfft.DfftError, match="one operator per output"):
        pl.execSpectralOps([1, 2], 3, [dict(multiplier=4)])
    with pytest.raises(dfft.DfftError, match="unknown operator keyword table"):
        pl.execSpectralOps([1], 3, [dict(table=(4, 5, 6))])
    with pytest.raises(dfft.DfftError, match="either multiplier= or tables= / factors="):
        pl.execSpectralOps([1], 3, [dict(scale=2.0)])
    with pytest.raises(dfft.DfftError, match="reciprocal=True needs tables="):
        pl.execSpectralOps([1], 3, [dict(multiplier=4, reciprocal=True)])
