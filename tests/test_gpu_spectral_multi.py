"""execSpectralOps (option "spectral_outputs", include/dfft_c.h: dfft_exec_spectral_ops): outs[j] = IFFT(m_j * FFT(in)) for several
operators with one forward half -- the z and y passes and the forward exchanges once, the fused x kernel and the inverse half once per
output.

1. Bit identity with execSpectralOp on the same plan.  Derived, not measured: both paths issue the same launches with the same
   arguments except buffer bases, and the footprint contract (include/dfft_c.h) says results do not depend on what the buffers held.
2. The gradient of a Poisson solution as one call against numpy, metric and bound of test_gpu_spectral_op.check.
3. `in` comes back bit for bit (every call of run_ops).
4. The footprint on guarded buffers (tests/guarded.py).
5. What the C layer refuses."""
import ctypes as C
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import distributedfft_amd as dfft  # noqa: E402
from distributedfft_amd._lib import SpectralOp, lib  # noqa: E402

import guarded  # noqa: E402
from test_gpu_parity import CDT, NPDT, NPR  # noqa: E402
from test_gpu_spectral_factors import device_factors, factor_reference  # noqa: E402
from test_gpu_spectral_op import GRIDS, check, device_multiplier, device_tables, in_block, make_plans, reference, table_reference  # noqa: E402

M = dfft.SPECTRAL_OPS
SHAPES = [(16, 12, 10), (8, 10, 38), (12, 10, 14)]      # the last: a mixed-radix x length, option spectral_op = 2
ERR_ARG, ERR_STATE = 2, 3


def multi_plans(shape, P1, P2, prec, c2c, layout, K=3, chunks=None, arena=None, **more):
    options = dict(more, spectral_op=1 if shape[0] & (shape[0] - 1) == 0 else 2, spectral_outputs=K)
    return make_plans(shape, P1, P2, prec, c2c, layout, chunks=chunks, options=options, arena=arena)


def run_ops(plans, prec, c2c, u, ops, arena=None, single=False):
    """execSpectralOps on every rank (one host thread each) with ops[r]: the rank's list of operator dicts; single=True: one execSpectralOp
    per operator instead, on the same plans.  The outputs are NaN-filled before the call and `in` must come back bit for bit.  Returns
    outs[r][j] as host arrays.  arena (tests/guarded.py): `in` and the outputs come from it at the first call and are used again at every
    later one; the outputs and the work areas are refilled before the exec, the guards and every input are checked after it"""
    P, dt = len(plans), NPDT[prec] if c2c else NPR[prec]
    nout = len(ops[0])
    if arena is not None:
        def setup():
            ins = [arena.input(in_block(pl, u).astype(dt), f"in[{r}]") for r, pl in enumerate(plans)]
            return ins, [[arena.buffer(t.numel() * t.element_size(), t.dtype, name=f"out{j}[{r}]").reshape(t.shape) for j in range(nout)]
                         for r, t in enumerate(ins)]
        ins, outs = arena.once("run_ops", setup)
        arena.refill()
    else:
        ins = [torch.from_numpy(in_block(pl, u).astype(dt)).cuda() for pl in plans]
        outs = [[torch.full_like(t, float("nan")) for _ in range(nout)] for t in ins]
    before = [t.cpu().numpy().tobytes() for t in ins]
    torch.cuda.synchronize()

    def rank(r):
        if single:
            for j in range(nout):
                plans[r].execSpectralOp(outs[r][j], ins[r], **ops[r][j])
        else:
            plans[r].execSpectralOps(outs[r], ins[r], ops[r])
    with ThreadPoolExecutor(P) as ex:
        list(ex.map(rank, range(P)))
    torch.cuda.synchronize()
    for r in range(P):
        assert ins[r].cpu().numpy().tobytes() == before[r], f"rank {r}: the input was modified"
    if arena is not None:
        arena.check_guards("execSpectralOps")
        arena.check_inputs("execSpectralOps")
    return [[t.cpu().numpy() for t in row] for row in outs]


def three_kinds(plans, prec, c2c, shape, arena=None):
    """per rank: operators of kinds 0 (array), 2 (reciprocal of a sum of tables) and 5 (factor tables over the sum), every array and table
    in a device buffer of its own (guarded inputs of the arena where there is one)"""
    m = reference(shape, prec, c2c)[1]
    tables = table_reference(shape, prec, c2c)[1]
    _, factors, ftables, _, _ = factor_reference(shape, prec, c2c)
    if arena is None:
        return [[dict(multiplier=device_multiplier(pl, prec, m)),
                 dict(tables=device_tables(pl, prec, tables), reciprocal=True, scale=0.5),
                 dict(factors=device_factors(pl, prec, factors), tables=device_tables(pl, prec, ftables), reciprocal=True, scale=0.25)] for pl in plans]
    ops = []
    for r, pl in enumerate(plans):
        (_, ny, nz), (_, y0, z0) = pl.getOutSize(), pl.getOutStart()
        local = lambda t: (t[0], t[1][y0:y0 + ny], t[2][z0:z0 + nz])      # noqa: E731
        put = lambda t, dt, name: tuple(arena.input(np.asarray(v).astype(dt), f"{name}{'xyz'[i]}[{r}]") for i, v in enumerate(local(t)))      # noqa: E731
        mt = torch.zeros(pl.getDomainSize() // (16 if prec == "double" else 8), dtype=CDT[prec])
        pl.spectrumView(mt).copy_(torch.from_numpy(np.ascontiguousarray(m[:, y0:y0 + ny, z0:z0 + nz]).astype(NPDT[prec])))
        ops.append([dict(multiplier=arena.input(mt.numpy(), f"mult[{r}]")),
                    dict(tables=put(tables, NPR[prec], "a"), reciprocal=True, scale=0.5),
                    dict(factors=put(factors, NPDT[prec], "c"), tables=put(ftables, NPR[prec], "b"), reciprocal=True, scale=0.25)])
    return ops


# ---- 1. bit identity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("P1,P2", GRIDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_output_is_bit_for_bit_that_of_the_single_call(shape, P1, P2, c2c, prec):
    """kinds 0, 2 and 5 in one call on a plan with option value 3, then two and one of them on the same plan, each output against
    execSpectralOp with the same operator on the same plan; both layouts, depths 1 and 3.  On the 2 x 2 world the all-to-all-v calls of
    one multi-output exec are counted (dfft_comm_get_counter): (2 + 2 K) * depth per rank, against 4 K * depth for the K single calls."""
    u = reference(shape, prec, c2c)[0]
    P = P1 * P2
    for layout in (0, 1):
        for chunks in (1, 3):
            plans = multi_plans(shape, P1, P2, prec, c2c, layout, chunks=chunks)
            depth = plans[0].getPipelineChunks()
            assert depth == chunks and len(plans[0].debugChain(M)) == 11
            ops = three_kinds(plans, prec, c2c, shape)
            what = f"layout {layout} depth {depth}"
            singles = run_ops(plans, prec, c2c, u, ops, single=True)
            for r in range(P):
                for j in range(3):
                    assert not np.isnan(singles[r][j]).any(), f"{what} rank {r}: execSpectralOp left NaN in output {j}"
                assert singles[r][0].tobytes() != singles[r][1].tobytes() != singles[r][2].tobytes()
            count = (lambda: plans[0].comm.getCounter("alltoallv")) if P > 1 else (lambda: 0)
            for nout in (3, 2, 1):
                c0 = count()
                multi = run_ops(plans, prec, c2c, u, [row[:nout] for row in ops])
                calls = count() - c0
                for r in range(P):
                    for j in range(nout):
                        assert multi[r][j].tobytes() == singles[r][j].tobytes(), \
                            f"{what} nout {nout} rank {r}: output {j} differs from execSpectralOp in {int(np.sum(multi[r][j] != singles[r][j]))} of {singles[r][j].size} entries"
                if (P1, P2) == (2, 2):
                    assert calls == P * (2 + 2 * nout) * depth, f"{what} nout {nout}: {calls} all-to-all-v calls on {P} ranks"
            if (P1, P2) == (2, 2):
                c0 = count()
                run_ops(plans, prec, c2c, u, ops, single=True)
                assert count() - c0 == P * 4 * 3 * depth


@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 2)])
def test_what_an_exec_issued_is_what_the_dry_trace_says(P1, P2):
    """option trace: debugTrace(SPECTRAL_OPS, 0) after an exec of all three outputs is the dry trace of the chain; after an exec of two it
    holds the launches and exchanges of the first 2 + 3 * 2 steps and nothing of the third output; the log of execSpectralOp is another one"""
    shape, prec, c2c = (16, 12, 10), "double", False
    u = reference(shape, prec, c2c)[0]
    plans = multi_plans(shape, P1, P2, prec, c2c, 0, chunks=3, trace=1)
    ops = three_kinds(plans, prec, c2c, shape)
    assert all(pl.debugTrace(M, 0) == [] for pl in plans)
    run_ops(plans, prec, c2c, u, ops, single=True)
    single_logs = [pl.debugTrace(dfft.SPECTRAL_OP, 0) for pl in plans]
    assert all(single_logs) and all(pl.debugTrace(M, 0) == [] for pl in plans)
    run_ops(plans, prec, c2c, u, ops)
    data = lambda t, below: [o for o in t if o["kind"] in (0, 1) and o["step"] < below]      # noqa: E731
    for pl, log in zip(plans, single_logs):
        dry = pl.debugTrace(M, 3)
        assert pl.debugTrace(M, 0) == dry and max(o["step"] for o in dry) == 10
        assert pl.debugTrace(dfft.SPECTRAL_OP, 0) == log
        assert {o["dst"] for o in dry if o["kind"] == 0 and o["dst"] < 0} == {-1, -3, -4}
    run_ops(plans, prec, c2c, u, [row[:2] for row in ops])
    for pl in plans:
        issued = pl.debugTrace(M, 0)
        assert data(issued, 99) == data(pl.debugTrace(M, 3), 8) and max(o["step"] for o in issued) == 7


# ---- 2. against numpy: the gradient of a Poisson solution in one call ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gradient_reference(shape, prec, c2c):
    """(u, wants): the zero-mean input of test_gpu_spectral_op.reference() and numpy's three components of grad(laplace^-1 u), built as
    test_null_factors_and_gradient_of_a_poisson_solution builds them: m_d = i k_d / -(kx^2 + ky^2 + kz^2), 0 at k = 0, |m_d| <= 1; R2C:
    i k_d is zeroed at the Nyquist point"""
    u = reference(shape, prec, c2c)[0]
    gk = [np.round(np.fft.fftfreq(m) * m) for m in shape]
    if not c2c:
        gk[2] = np.arange(shape[2] // 2 + 1, dtype=np.float64)
    nyquist = [np.abs(k) * 2 == m for k, m in zip(gk, shape)]
    s = -(gk[0][:, None, None] ** 2 + gk[1][None, :, None] ** 2 + gk[2][None, None, :] ** 2)
    U = np.fft.fftn(u) if c2c else np.fft.rfftn(u)
    wants = []
    for d in range(3):
        kd = np.where(nyquist[d], 0.0, gk[d]) if not c2c else gk[d]
        m = 1j * kd.reshape([-1 if a == d else 1 for a in range(3)]) * np.where(s != 0, 1.0 / np.where(s != 0, s, 1.0), 0.0)
        want = np.fft.ifftn(U * m) if c2c else np.fft.irfftn(U * m, s=shape, axes=(0, 1, 2))
        want.setflags(write=False)
        wants.append(want)
    return u, tuple(wants)


def gradient_ops(plans, prec, c2c, shape):
    """per rank: three kind-5 operators, the d-th with the factor table i * k_d and the other two None, sums -(kx^2 + ky^2 + kz^2), every
    table from the plan's own wavenumbers()"""
    n = float(np.prod(shape))
    dev = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).cuda()      # noqa: E731
    ops = []
    for pl in plans:
        k = pl.wavenumbers()
        sums = tuple(dev(-(t.astype(np.float64) ** 2), NPR[prec]) for t in k)
        row = []
        for d in range(3):
            kl = k[d].astype(np.float64)
            if not c2c:
                kl = np.where(np.abs(kl) * 2 == shape[d], 0.0, kl)
            factors = [None, None, None]
            factors[d] = dev(1j * kl, NPDT[prec])
            row.append(dict(factors=tuple(factors), tables=sums, reciprocal=True, scale=1.0 / n))
        ops.append(row)
    return ops


def gradient_case(shape, P1, P2, c2c, prec):
    u, wants = gradient_reference(shape, prec, c2c)
    plans = multi_plans(shape, P1, P2, prec, c2c, 0)
    # on the reference alone, before anything runs on the GPU: every rank's block of every component has something to check
    for d, want in enumerate(wants):
        assert all(np.any(in_block(pl, want) != 0) for pl in plans), f"component {d}: a rank's expected block is all zeros"
    outs = run_ops(plans, prec, c2c, u, gradient_ops(plans, prec, c2c, shape))
    for d, want in enumerate(wants):
        check(plans, [outs[r][d] for r in range(len(plans))], want, prec, f"d/d{'xyz'[d]} of the Poisson solution, one call")


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 2)])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gradient_of_a_poisson_solution_in_one_call(shape, P1, P2, c2c, prec):
    gradient_case(shape, P1, P2, c2c, prec)


@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
def test_gradient_on_2048_point_x_lines(c2c):
    gradient_case((2048, 8, 16), 1, 1, c2c, "double")


# ---- 4. footprint --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 2)])
def test_footprint_on_guarded_buffers(P1, P2, prec):
    """R2C, depth 3, the ragged shape: `in`, the three outputs, every operator array and table and the caller-owned work areas of
    getWorkSizeDevice() bytes are guarded buffers.  Once with outputs and work areas filled with 0xFF and once with 0x00: no guard byte
    and no input changes, every output entry is written, and the two results are identical bit for bit -- and they are those of
    execSpectralOp."""
    shape, c2c = (8, 10, 38), False
    u = reference(shape, prec, c2c)[0]
    arena = guarded.Arena("cuda")
    results = []
    for fill in (0xFF, 0x00):
        arena.fill = fill
        plans = arena.once("plans", lambda: multi_plans(shape, P1, P2, prec, c2c, 0, chunks=3, arena=arena))
        ops = arena.once("ops", lambda: three_kinds(plans, prec, c2c, shape, arena=arena))
        assert all(pl.getPipelineChunks() == 3 and pl.getWorkAreaDevice() for pl in plans)
        results.append(run_ops(plans, prec, c2c, u, ops, arena=arena))
    singles = run_ops(plans, prec, c2c, u, ops, single=True)
    for r in range(P1 * P2):
        for j in range(3):
            what = f"execSpectralOps {shape} {P1}x{P2} R2C {prec}, rank {r}, output {j}"
            guarded.assert_written(results[0][r][j], what + ", buffers filled with 0xFF")
            guarded.assert_written(results[1][r][j], what + ", buffers filled with 0x00")
            assert results[0][r][j].tobytes() == results[1][r][j].tobytes(), what + ": the result depends on what the outputs or the work area held before"
            assert results[0][r][j].tobytes() == singles[r][j].tobytes(), what + ": differs from execSpectralOp"


# ---- 5. what the C layer refuses -------------------------------------------------------------------------------------------------------
def test_argument_errors_in_the_c_layer():
    shape = (16, 12, 10)
    n = int(np.prod(shape))
    pl = multi_plans(shape, 1, 1, "double", True, 0)[0]
    a = torch.zeros(n, dtype=CDT["double"], device="cuda")
    outs = [torch.full_like(a, 7.0) for _ in range(4)]
    t = torch.ones(16, dtype=torch.float64, device="cuda")
    good = lambda: SpectralOp(1, 1.0, None, t.data_ptr(), t.data_ptr(), t.data_ptr())      # noqa: E731

    def call(plan, nout, out_tensors, in_, ops):
        c_outs = None if out_tensors is None else (C.c_void_p * len(out_tensors))(*[None if o is None else o.data_ptr() for o in out_tensors])
        c_ops = None if ops is None else (SpectralOp * len(ops))(*ops)
        rc = lib().dfft_exec_spectral_ops(plan._h, nout, c_outs, None if in_ is None else C.c_void_p(in_.data_ptr()), c_ops)
        msg = lib().dfft_last_error().decode()
        assert rc == 0 or msg, "a refused call left no message"
        return rc, msg

    four = [good() for _ in range(4)]
    assert call(pl, 0, outs, a, four)[0] == ERR_ARG
    assert call(pl, 4, outs, a, four)[0] == ERR_ARG      # the option's value + 1
    assert call(pl, 2, [outs[0], outs[0]], a, four)[0] == ERR_ARG
    assert call(pl, 3, [outs[0], outs[1], outs[0]], a, four)[0] == ERR_ARG
    assert call(pl, 2, [outs[0], a], a, four)[0] == ERR_ARG
    assert call(pl, 2, outs, a, None)[0] == ERR_ARG
    assert call(pl, 2, None, a, four)[0] == ERR_ARG
    assert call(pl, 2, outs, None, four)[0] == ERR_ARG
    assert call(pl, 2, [outs[0], None], a, four)[0] == ERR_ARG
    rc, msg = call(pl, 3, outs, a, [good(), SpectralOp(6, 1.0, None, t.data_ptr(), t.data_ptr(), t.data_ptr()), good()])
    assert rc == ERR_ARG and "ops[1]" in msg and "kind must be" in msg, msg
    rc, msg = call(pl, 3, outs, a, [good(), good(), SpectralOp(4, 1.0, None, t.data_ptr(), t.data_ptr(), t.data_ptr())])
    assert rc == ERR_ARG and "ops[2]" in msg and "at least one of cx, cy, cz" in msg, msg
    rc, msg = call(pl, 1, outs, a, [SpectralOp(0, 1.0, None)])
    assert rc == ERR_ARG and "ops[0]" in msg and "null multiplier" in msg, msg
    for options in ({"spectral_outputs": 1}, {}):      # the value 1, and a plan that never heard of the option
        off = make_plans(shape, 1, 1, "double", True, 0, options=options)[0]
        rc, msg = call(off, 1, outs, a, four)
        assert rc == ERR_STATE and "set spectral_outputs before dfft_init" in msg, msg
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs), "a refused call wrote to an output"
    assert call(pl, 3, outs, a, four)[0] == 0      # and the plan still runs
    torch.cuda.synchronize()
    assert not any(bool((o == 7.0).any()) for o in outs[:3]) and bool((outs[3] == 7.0).all())

    def init(**options):
        p = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), None, precision="double")
        for k, v in options.items():
            p.setOption(k, v)
        rc = lib().dfft_init(p._h, 16, 12, 10, 1, 1, 0, 1)
        return rc, lib().dfft_last_error().decode()
    for v in (9, 0):
        rc, msg = init(spectral_op=1, spectral_outputs=v)
        assert rc == ERR_ARG and "spectral_outputs" in msg, (rc, msg)
    rc, msg = init(spectral_outputs=2)
    assert rc == ERR_ARG and "spectral_op" in msg, (rc, msg)
    assert init(spectral_op=1, spectral_outputs=8)[0] == 0
