"""execSpectralSum (option "spectral_inputs", include/dfft_c.h: dfft_exec_spectral_sum): out = sum_j IFFT(m_j * FFT(in_j)) with one
inverse half -- per input the z and y passes, the forward exchanges and the fused x kernel, which from the second input on adds its
result to what the first stored; then the inverse y and z passes once.

1. Identities that are exact by construction (derived, not measured): one input is execSpectralOp bit for bit (the same launches but
   for buffer bases); a zero input adds nothing (x + 0 = x; compared by value, -0 + 0 is +0); two (input, operator) pairs commute bit
   for bit (a + b = b + a in IEEE arithmetic, and the accumulating kernels round their term before they add it).
2. Against numpy: a divergence, a component of a curl, a mix of kinds 2, 4 and 5; the project's per-entry metric with the bound of
   test_gpu_spectral_op.check, normalised by the SUM of the terms' rms.
3. The all-to-all-v count, the footprint on guarded buffers (tests/guarded.py), the trace, what the C layer refuses."""
import ctypes as C
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import distributedfft_amd as dfft  # noqa: E402
from distributedfft_amd._lib import SpectralOp, lib  # noqa: E402

import guarded  # noqa: E402
from parity_metric import CENTER, forward_bound, record, rms, rms_rel, worst_entry  # noqa: E402
from test_gpu_parity import CDT, NPDT, NPR  # noqa: E402
from test_gpu_spectral_factors import device_factors, factor_reference  # noqa: E402
from test_gpu_spectral_op import GRIDS, device_tables, in_block, make_plans, reference, table_reference  # noqa: E402

Q = dfft.SPECTRAL_SUM
SHAPES = [(16, 12, 10), (8, 10, 38), (12, 10, 14)]      # ragged with an odd pitch; a mixed-radix x length, option spectral_op = 2
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = 2, 3, 4


def sum_plans(shape, P1, P2, prec, c2c, layout, K=3, chunks=None, arena=None, **more):
    options = dict(more, spectral_op=1 if shape[0] & (shape[0] - 1) == 0 else 2, spectral_inputs=K)
    return make_plans(shape, P1, P2, prec, c2c, layout, chunks=chunks, options=options, arena=arena)


def run_sum(plans, prec, c2c, us, ops, arena=None, single=False):
    """execSpectralSum on every rank (one host thread each) with us: the inputs over the whole domain, ops[r]: the rank's list of operator
    dicts, one per input; single=True: execSpectralOp of (us[0], ops[r][0]) instead, on the same plans.  The output is NaN-filled before
    the call and every input must come back bit for bit.  Returns the ranks' output blocks as host arrays.  arena (tests/guarded.py): the
    inputs and the output come from it at the first call and are used again at every later one; the output and the work areas are
    refilled before the exec, the guards and every input are checked after it"""
    P, dt = len(plans), NPDT[prec] if c2c else NPR[prec]
    assert all(len(row) == len(us) for row in ops)
    if arena is not None:
        def setup():
            ins = [[arena.input(in_block(pl, u).astype(dt), f"in{j}[{r}]") for j, u in enumerate(us)] for r, pl in enumerate(plans)]
            return ins, [arena.buffer(row[0].numel() * row[0].element_size(), row[0].dtype, name=f"out[{r}]").reshape(row[0].shape)
                         for r, row in enumerate(ins)]
        ins, outs = arena.once("run_sum", setup)
        arena.refill()
    else:
        ins = [[torch.from_numpy(in_block(pl, u).astype(dt)).cuda() for u in us] for pl in plans]
        outs = [torch.full_like(row[0], float("nan")) for row in ins]
    before = [[t.cpu().numpy().tobytes() for t in row] for row in ins]
    torch.cuda.synchronize()

    def rank(r):
        if single:
            plans[r].execSpectralOp(outs[r], ins[r][0], **ops[r][0])
        else:
            plans[r].execSpectralSum(outs[r], ins[r], ops[r])
    with ThreadPoolExecutor(P) as ex:
        list(ex.map(rank, range(P)))
    torch.cuda.synchronize()
    for r in range(P):
        for j, t in enumerate(ins[r]):
            assert t.cpu().numpy().tobytes() == before[r][j], f"rank {r}: input {j} was modified"
    if arena is not None:
        arena.check_guards("execSpectralSum")
        arena.check_inputs("execSpectralSum")
    return [t.cpu().numpy() for t in outs]


def two_families(plans, prec, c2c, shape):
    """per rank: an operator of either kernel family -- kind 2 (the reciprocal of a sum of real tables: TABLES = 1) and kind 5 (factor
    tables over the sum: TABLES = 2) -- every table in a device buffer of its own"""
    tables = table_reference(shape, prec, c2c)[1]
    _, factors, ftables, _, _ = factor_reference(shape, prec, c2c)
    return [[dict(tables=device_tables(pl, prec, tables), reciprocal=True, scale=0.5),
             dict(factors=device_factors(pl, prec, factors), tables=device_tables(pl, prec, ftables), reciprocal=True, scale=0.25)] for pl in plans]


@functools.lru_cache(maxsize=None)
def fields(shape, prec, c2c, count=3):
    """`count` independent zero-mean fields, rounded to the plan's precision like test_gpu_spectral_op.reference()'s input"""
    rng = np.random.default_rng(20261020)
    out = []
    for _ in range(count):
        if c2c:
            u = ((rng.uniform(0, 255, shape) - CENTER) + 1j * (rng.uniform(0, 255, shape) - CENTER)).astype(NPDT[prec]).astype(np.complex128)
        else:
            u = (rng.uniform(0, 255, shape) - CENTER).astype(NPR[prec]).astype(np.float64)
        u.setflags(write=False)
        out.append(u)
    return tuple(out)


# ---- 1. exact identities ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("P1,P2", GRIDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_input_a_zero_input_and_the_order_of_two(shape, P1, P2, c2c, prec):
    """On a plan with option value 3, both layouts, depths 1 and 3, for an operator of either kernel family:
    one input is execSpectralOp bit for bit; [u, 0] and [0, u] equal execSpectralOp(u) by value (a form-6 launch that reads the wrong
    address, or a first xx that accumulates onto the NaN-filled slice, fails here); [u, v] with [a, b] and [v, u] with [b, a] give the
    same bytes."""
    u, v = fields(shape, prec, c2c)[:2]
    zero = np.zeros_like(u)
    P = P1 * P2
    for layout in (0, 1):
        for chunks in (1, 3):
            plans = sum_plans(shape, P1, P2, prec, c2c, layout, chunks=chunks)
            depth = plans[0].getPipelineChunks()
            assert depth == chunks and len(plans[0].debugChain(Q)) == 11
            ops = two_families(plans, prec, c2c, shape)
            what = f"layout {layout} depth {depth}"
            for a, b in ((0, 1), (1, 0)):
                pick = lambda *idx: [[row[i] for i in idx] for row in ops]      # noqa: E731
                single = run_sum(plans, prec, c2c, [u], pick(a), single=True)
                for r in range(P):
                    assert not np.isnan(single[r]).any() and np.any(single[r] != 0), f"{what} rank {r}: execSpectralOp left NaN or nothing"
                one = run_sum(plans, prec, c2c, [u], pick(a))
                behind = run_sum(plans, prec, c2c, [u, zero], pick(a, b))
                ahead = run_sum(plans, prec, c2c, [zero, u], pick(b, a))
                for r in range(P):
                    assert one[r].tobytes() == single[r].tobytes(), \
                        f"{what} operator {a} rank {r}: one input differs from execSpectralOp in {int(np.sum(one[r] != single[r]))} of {single[r].size} entries"
                    assert np.array_equal(behind[r], single[r]), f"{what} operator {a} rank {r}: a zero second input changed {int(np.sum(behind[r] != single[r]))} entries"
                    assert np.array_equal(ahead[r], single[r]), f"{what} operator {a} rank {r}: a zero first input changed {int(np.sum(ahead[r] != single[r]))} entries"
            uv = run_sum(plans, prec, c2c, [u, v], ops)
            vu = run_sum(plans, prec, c2c, [v, u], [row[::-1] for row in ops])
            for r in range(P):
                assert not np.isnan(uv[r]).any()
                assert uv[r].tobytes() == vu[r].tobytes(), f"{what} rank {r}: swapping the two pairs changed {int(np.sum(uv[r] != vu[r]))} of {uv[r].size} entries"


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("Nx", [1024, 2048])
def test_the_order_of_two_on_long_x_lines(Nx, prec):
    """the same two identities at the x lengths with the most registers per lane, one rank, C2C: [0, u] equals execSpectralOp(u) by value
    and the two pairs commute bit for bit -- both hold only while the accumulating kernel's term is the plain kernel's to the last bit,
    which nothing but the way the kernel is written asks of the compiler (fft_spectral_kernel, the ACC branch)"""
    shape, c2c = (Nx, 8, 16), True
    u, v = fields(shape, prec, c2c)[:2]
    plans = sum_plans(shape, 1, 1, prec, c2c, 0)
    ops = two_families(plans, prec, c2c, shape)
    for a, b in ((0, 1), (1, 0)):
        single = run_sum(plans, prec, c2c, [u], [[ops[0][a]]], single=True)[0]
        ahead = run_sum(plans, prec, c2c, [np.zeros_like(u), u], [[ops[0][b], ops[0][a]]])[0]
        assert np.any(single != 0) and np.array_equal(ahead, single), f"operator {a}: a zero first input changed {int(np.sum(ahead != single))} of {single.size} entries"
    uv = run_sum(plans, prec, c2c, [u, v], ops)[0]
    vu = run_sum(plans, prec, c2c, [v, u], [ops[0][::-1]])[0]
    assert not np.isnan(uv).any() and uv.tobytes() == vu.tobytes(), f"swapping the two pairs changed {int(np.sum(uv != vu))} of {uv.size} entries"


def test_alltoallv_calls_on_the_2x2_world():
    """(2 nin + 2) * depth per rank and call, for nin = 3, 2, 1 (dfft_comm_get_counter), against 4 * depth for every execSpectralOp"""
    shape, prec, c2c, P = (16, 12, 10), "double", False, 4
    us = fields(shape, prec, c2c)
    for chunks in (1, 3):
        plans = sum_plans(shape, 2, 2, prec, c2c, 0, chunks=chunks)
        depth = plans[0].getPipelineChunks()
        ops = [row + [row[0]] for row in two_families(plans, prec, c2c, shape)]
        count = lambda: plans[0].comm.getCounter("alltoallv")      # noqa: E731
        for nin in (3, 2, 1):
            c0 = count()
            run_sum(plans, prec, c2c, us[:nin], [row[:nin] for row in ops])
            assert count() - c0 == P * (2 * nin + 2) * depth, f"depth {depth} nin {nin}: {count() - c0} all-to-all-v calls on {P} ranks"
        c0 = count()
        run_sum(plans, prec, c2c, us[:1], [row[:1] for row in ops], single=True)
        assert count() - c0 == P * 4 * depth


# ---- 2. against numpy ------------------------------------------------------------------------------------------------------------------
def wave_tables(shape, c2c):
    """per axis d: i * k_d / kmax_d over the whole spectrum with the Nyquist entry zeroed for R2C (as
    test_gpu_spectral_multi.gradient_reference zeroes it); kmax_d = shape[d] / 2, the axis's own largest wavenumber, keeps |m_d| <= 1 and
    the terms of an anisotropic grid such as (2048, 8, 16) comparable (a derivative in units of each axis's own grid spacing)"""
    gk = [np.round(np.fft.fftfreq(m) * m) for m in shape]
    if not c2c:
        gk[2] = np.arange(shape[2] // 2 + 1, dtype=np.float64)
    return [1j * (k if c2c else np.where(np.abs(k) * 2 == m, 0.0, k)) / (m / 2.0) for k, m in zip(gk, shape)]


def term(u, m, shape, c2c):
    want = np.fft.ifftn(np.fft.fftn(u) * m) if c2c else np.fft.irfftn(np.fft.rfftn(u) * m, s=shape, axes=(0, 1, 2))
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def divergence_reference(shape, prec, c2c):
    """(us, wants): three fields and numpy's three terms d u_d / d x_d / kmax_d, m_d = i k_d / kmax_d"""
    us = fields(shape, prec, c2c)
    ik = wave_tables(shape, c2c)
    return us, tuple(term(us[d], ik[d].reshape([-1 if a == d else 1 for a in range(3)]), shape, c2c) for d in range(3))


@functools.lru_cache(maxsize=None)
def curl_reference(shape, prec, c2c):
    """(us, wants): the z component of a curl, d u_y / dx - d u_x / dy: inputs (u_y, u_x), m = (i kx / kmax_x, -i ky / kmax_y)"""
    ux, uy, _ = fields(shape, prec, c2c)
    ik = wave_tables(shape, c2c)
    return (uy, ux), (term(uy, ik[0][:, None, None], shape, c2c), term(ux, -ik[1][None, :, None], shape, c2c))


def derivative_ops(plans, prec, c2c, shape, axes, signs):
    """per rank: one kind-3 operator per entry of `axes`, its factor table i * k_d from the plan's own wavenumbers() (Nyquist zeroed for
    R2C) on axis d and None on the others, scale = sign / (n * kmax_d), kmax_d = shape[d] / 2"""
    n = float(np.prod(shape))
    ops = []
    for pl in plans:
        k = pl.wavenumbers()
        row = []
        for d, sign in zip(axes, signs):
            kl = k[d].astype(np.float64)
            if not c2c:
                kl = np.where(np.abs(kl) * 2 == shape[d], 0.0, kl)
            factors = [None, None, None]
            factors[d] = torch.from_numpy(np.ascontiguousarray(1j * kl).astype(NPDT[prec])).cuda()
            row.append(dict(factors=tuple(factors), scale=sign / (n * (shape[d] / 2.0))))
        ops.append(row)
    return ops


MIX_INPUT = (1.0, -2.0, 0.5)        # the mix runs on three multiples of one field (exact in binary: the references scale with them)
MIX_SCALE = (0.5, 1.0 / 32, 0.25)   # kinds 2, 4, 5: |1 / sum| <= 1; |P| <= 2 sqrt(2) and |sum| <= 9, so |P sum / 32| <= 0.8; |P / sum| / 4 <= 0.71


@functools.lru_cache(maxsize=None)
def mix_reference(shape, prec, c2c):
    """(us, wants) of a three-input mix of kinds 2, 4 and 5 out of the references of the table and factor tests (numpy, float64), each
    scaled to the input's multiple and to a scale that keeps |m| <= 1; unnormalised like those references, i.e. times n"""
    u, _, twants, _, _ = table_reference(shape, prec, c2c)
    _, _, _, fwants, _ = factor_reference(shape, prec, c2c)      # at scale 0.25
    us = tuple(u * c for c in MIX_INPUT)
    wants = (twants[1] * (MIX_INPUT[0] * MIX_SCALE[0]), fwants[1] * (MIX_INPUT[1] * MIX_SCALE[1] / 0.25), fwants[2] * (MIX_INPUT[2] * MIX_SCALE[2] / 0.25))
    n = float(np.prod(shape))
    return us, tuple(w / n for w in wants)


def mix_ops(plans, prec, c2c, shape):
    n = float(np.prod(shape))
    tables = table_reference(shape, prec, c2c)[1]
    _, factors, ftables, _, _ = factor_reference(shape, prec, c2c)
    return [[dict(tables=device_tables(pl, prec, tables), reciprocal=True, scale=MIX_SCALE[0] / n),
             dict(factors=device_factors(pl, prec, factors), tables=device_tables(pl, prec, ftables), scale=MIX_SCALE[1] / n),
             dict(factors=device_factors(pl, prec, factors), tables=device_tables(pl, prec, ftables), reciprocal=True, scale=MIX_SCALE[2] / n)]
            for pl in plans]


def check_sum(plans, outs, wants, prec, what):
    """every rank's block against its block of sum_j wants[j], each entry held to sum_j rms(wants[j]): every term is two transforms held to
    the per-entry forward bound with |m_j| <= 1, and the errors add; the K - 1 additions contribute an ulp each, far inside the bound's
    constant.  The worst rank's value goes to the table (parity_metric.record) before anything is asserted"""
    n = int(np.prod(wants[0].shape))
    scale, bound = sum(rms(w) for w in wants), 2 * forward_bound(prec, n)
    want = functools.reduce(lambda a, b: a + b, wants)
    refs = [in_block(pl, want) for pl in plans]
    vals = [rms_rel(outs[r], refs[r], scale) if np.isfinite(outs[r]).all() else float("inf") for r in range(len(plans))]
    record(os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0].split("::")[-1] + " " + what, prec, n, max(vals), bound)
    for r, v in enumerate(vals):
        assert not np.isnan(outs[r]).any(), f"{what} rank {r}: NaN in the output (a part that was not written, or a product with inf)"
        assert np.isfinite(outs[r]).all(), f"{what} rank {r}: inf in the output"
        assert v <= bound, f"{what} rank {r}: per-entry error {v:.3e} > {bound:.1e}; " + worst_entry(outs[r], refs[r], scale)


def reference_has_something_to_check(plans, wants, what):
    """on the reference alone, before anything runs on the GPU: every rank's expected block is non-zero, and no term is small against
    the others -- a dropped, doubled or mis-paired term then misses the bound by orders of magnitude"""
    want = functools.reduce(lambda a, b: a + b, wants)
    assert all(np.any(in_block(pl, want) != 0) for pl in plans), f"{what}: a rank's expected block is all zeros"
    total = sum(rms(w) for w in wants)
    for j, w in enumerate(wants):
        assert rms(w) >= 0.1 * total / len(wants), f"{what}: term {j} has rms {rms(w):.3e} of {total:.3e} in all"


def numpy_case(shape, P1, P2, c2c, prec, which):
    """both layouts, each at the default depth and at depth 3, against one reference"""
    for layout in (0, 1):
        for chunks in (None, 3):
            plans = sum_plans(shape, P1, P2, prec, c2c, layout, chunks=chunks)
            assert chunks is None or plans[0].getPipelineChunks() == chunks
            if which == "divergence":
                (us, wants), ops = divergence_reference(shape, prec, c2c), derivative_ops(plans, prec, c2c, shape, (0, 1, 2), (1, 1, 1))
            elif which == "curl":
                (us, wants), ops = curl_reference(shape, prec, c2c), derivative_ops(plans, prec, c2c, shape, (0, 1), (1, -1))
            else:
                (us, wants), ops = mix_reference(shape, prec, c2c), mix_ops(plans, prec, c2c, shape)
            reference_has_something_to_check(plans, wants, which)
            check_sum(plans, run_sum(plans, prec, c2c, us, ops), wants, prec,
                      f"{which}, layout {layout}, depth {plans[0].getPipelineChunks()}")


@pytest.mark.parametrize("which", ["divergence", "curl", "mix"])
@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("P1,P2", GRIDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_numpy(shape, P1, P2, c2c, prec, which):
    numpy_case(shape, P1, P2, c2c, prec, which)


@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
def test_divergence_on_2048_point_x_lines(c2c):
    numpy_case((2048, 8, 16), 1, 1, c2c, "double", "divergence")


# ---- 3. footprint, trace, refusals -----------------------------------------------------------------------------------------------------
def guarded_ops(arena, plans, prec, c2c, shape):
    """mix_ops with every table in a guarded input buffer of the arena"""
    n = float(np.prod(shape))
    tables = table_reference(shape, prec, c2c)[1]
    _, factors, ftables, _, _ = factor_reference(shape, prec, c2c)
    ops = []
    for r, pl in enumerate(plans):
        (_, ny, nz), (_, y0, z0) = pl.getOutSize(), pl.getOutStart()
        local = lambda t: (t[0], t[1][y0:y0 + ny], t[2][z0:z0 + nz])      # noqa: E731
        put = lambda t, dt, name: tuple(arena.input(np.asarray(v).astype(dt), f"{name}{'xyz'[i]}[{r}]") for i, v in enumerate(local(t)))      # noqa: E731
        a, c, b = put(tables, NPR[prec], "a"), put(factors, NPDT[prec], "c"), put(ftables, NPR[prec], "b")
        ops.append([dict(tables=a, reciprocal=True, scale=MIX_SCALE[0] / n), dict(factors=c, tables=b, scale=MIX_SCALE[1] / n),
                    dict(factors=c, tables=b, reciprocal=True, scale=MIX_SCALE[2] / n)])
    return ops


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 2)])
def test_footprint_on_guarded_buffers(P1, P2, prec):
    """R2C, depth 3, the ragged shape: the three inputs, `out`, every operator table and the caller-owned work areas of
    getWorkSizeDevice() bytes are guarded buffers.  Once with the output and the work areas filled with 0xFF and once with 0x00: no guard
    byte and no input changes, every output entry is written, and the two results are identical bit for bit -- a first xx that
    accumulates, or any read of the accumulator before it is written, makes them differ -- and they pass the numpy check."""
    shape, c2c = (8, 10, 38), False
    us, wants = mix_reference(shape, prec, c2c)
    arena = guarded.Arena("cuda")
    results = []
    for fill in (0xFF, 0x00):
        arena.fill = fill
        plans = arena.once("plans", lambda: sum_plans(shape, P1, P2, prec, c2c, 0, chunks=3, arena=arena))
        ops = arena.once("ops", lambda: guarded_ops(arena, plans, prec, c2c, shape))
        assert all(pl.getPipelineChunks() == 3 and pl.getWorkAreaDevice() for pl in plans)
        results.append(run_sum(plans, prec, c2c, us, ops, arena=arena))
    for r in range(P1 * P2):
        what = f"execSpectralSum {shape} {P1}x{P2} R2C {prec}, rank {r}"
        guarded.assert_written(results[0][r], what + ", buffers filled with 0xFF")
        guarded.assert_written(results[1][r], what + ", buffers filled with 0x00")
        assert results[0][r].tobytes() == results[1][r].tobytes(), what + ": the result depends on what the output or the work area held before"
    check_sum(plans, results[0], wants, prec, "mix on guarded buffers")


@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 2)])
def test_what_an_exec_issued_is_what_the_dry_trace_says(P1, P2):
    """option trace: debugTrace(SPECTRAL_SUM, 0) after an exec of all three inputs is the dry trace of the plan's chain; after an exec of
    two it is the dry trace of a plan whose option value is 2 (the chain for fewer inputs is built from the plan's own slices, which do
    not depend on the number of inputs); the log of execSpectralOp is another one"""
    shape, prec, c2c = (16, 12, 10), "double", False
    us = fields(shape, prec, c2c)
    plans = sum_plans(shape, P1, P2, prec, c2c, 0, chunks=3, trace=1)
    two = sum_plans(shape, P1, P2, prec, c2c, 0, K=2, chunks=3, trace=1)
    ops = [row + [row[0]] for row in two_families(plans, prec, c2c, shape)]
    assert all(pl.debugTrace(Q, 0) == [] for pl in plans)
    run_sum(plans, prec, c2c, us[:1], [row[:1] for row in ops], single=True)
    single_logs = [pl.debugTrace(dfft.SPECTRAL_OP, 0) for pl in plans]
    assert all(single_logs) and all(pl.debugTrace(Q, 0) == [] for pl in plans)
    run_sum(plans, prec, c2c, us, ops)
    for pl, log in zip(plans, single_logs):
        dry = pl.debugTrace(Q, 3)
        assert pl.debugTrace(Q, 0) == dry and max(o["step"] for o in dry) == 10
        assert pl.debugTrace(dfft.SPECTRAL_OP, 0) == log
        assert {o["src"] for o in dry if o["kind"] == 0 and o["src"] < 0} == {-2, -10, -11}
    run_sum(plans, prec, c2c, us[:2], [row[:2] for row in ops])
    for pl, other in zip(plans, two):
        issued = pl.debugTrace(Q, 0)
        assert issued == other.debugTrace(Q, 3) and max(o["step"] for o in issued) == 7


def test_argument_errors_in_the_c_layer():
    shape = (16, 12, 10)
    n = int(np.prod(shape))
    pl = sum_plans(shape, 1, 1, "double", True, 0)[0]
    ins = [torch.ones(n, dtype=CDT["double"], device="cuda") for _ in range(4)]
    out = torch.full_like(ins[0], 7.0)
    t = torch.ones(16, dtype=torch.float64, device="cuda")
    good = lambda: SpectralOp(1, 1.0, None, t.data_ptr(), t.data_ptr(), t.data_ptr())      # noqa: E731

    def call(plan, nin, out_, in_tensors, ops):
        c_ins = None if in_tensors is None else (C.c_void_p * len(in_tensors))(*[None if u is None else u.data_ptr() for u in in_tensors])
        c_ops = None if ops is None else (SpectralOp * len(ops))(*ops)
        rc = lib().dfft_exec_spectral_sum(plan._h, None if out_ is None else C.c_void_p(out_.data_ptr()), nin, c_ins, c_ops)
        msg = lib().dfft_last_error().decode()
        assert rc == 0 or msg, "a refused call left no message"
        return rc, msg

    four = [good() for _ in range(4)]
    assert call(pl, 0, out, ins, four)[0] == ERR_ARG
    assert call(pl, 4, out, ins, four)[0] == ERR_ARG      # the option's value + 1
    assert call(pl, 2, out, ins, None)[0] == ERR_ARG
    assert call(pl, 2, out, None, four)[0] == ERR_ARG
    assert call(pl, 2, None, ins, four)[0] == ERR_ARG
    assert call(pl, 2, out, [ins[0], None], four)[0] == ERR_ARG
    assert call(pl, 2, out, [ins[0], out], four)[0] == ERR_ARG      # `out` equal to an input
    assert call(pl, 1, out, [out], four)[0] == ERR_ARG
    rc, msg = call(pl, 3, out, ins, [good(), SpectralOp(6, 1.0, None, t.data_ptr(), t.data_ptr(), t.data_ptr()), good()])
    assert rc == ERR_ARG and "ops[1]" in msg and "kind must be" in msg, msg
    rc, msg = call(pl, 3, out, ins, [good(), good(), SpectralOp(4, 1.0, None, t.data_ptr(), t.data_ptr(), t.data_ptr())])
    assert rc == ERR_ARG and "ops[2]" in msg and "at least one of cx, cy, cz" in msg, msg
    rc, msg = call(pl, 1, out, ins, [SpectralOp(2, 1.0, None, t.data_ptr(), None, t.data_ptr())])
    assert rc == ERR_ARG and "ops[0]" in msg and "null multiplier" in msg, msg
    m = torch.ones(pl.getDomainSize() // 16, dtype=CDT["double"], device="cuda")
    rc, msg = call(pl, 2, out, ins, [good(), SpectralOp(0, 1.0, m.data_ptr())])
    assert rc == ERR_UNSUPPORTED and "ops[1]" in msg and "table forms, kinds 1-5" in msg, msg
    for options in ({"spectral_inputs": 1}, {}):      # the value 1, and a plan that never heard of the option
        off = make_plans(shape, 1, 1, "double", True, 0, options=options)[0]
        rc, msg = call(off, 1, out, ins, four)
        assert rc == ERR_STATE and "set spectral_inputs before dfft_init" in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote to the output"
    assert call(pl, 2, out, [ins[0], ins[0]], four)[0] == 0      # two equal inputs are allowed, and the plan still runs
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any()) and bool(torch.isfinite(torch.view_as_real(out)).all())
    assert call(pl, 3, out, ins, four)[0] == 0

    def init(**options):
        p = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), None, precision="double")
        for k, v in options.items():
            p.setOption(k, v)
        rc = lib().dfft_init(p._h, 16, 12, 10, 1, 1, 0, 1)
        return rc, lib().dfft_last_error().decode()
    for v in (9, 0):
        rc, msg = init(spectral_op=1, spectral_inputs=v)
        assert rc == ERR_ARG and "spectral_inputs" in msg, (rc, msg)
    rc, msg = init(spectral_inputs=2)
    assert rc == ERR_ARG and "spectral_op" in msg, (rc, msg)
    assert init(spectral_op=1, spectral_inputs=8)[0] == 0
