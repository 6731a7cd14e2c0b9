"""execSpectralOp on mixed-radix x lengths (option "spectral_op" = 2, include/dfft_c.h): the fused forward-multiply-inverse x pass runs the
kernels of csrc/spectral_mixed_<p>.hip out of libdfft_amd_any.so; the chain around it is the one tests/test_gpu_spectral_op.py holds to numpy
for the powers of two.

Reference: numpy in float64 on inputs rounded to the plan's precision.  Metric and bound: those of tests/test_gpu_spectral_op.py,
rms_rel(got, want) <= 2 * forward_bound(prec, n) per rank block, recorded through parity_metric.record (check() there).  Inputs are zero-mean,
outputs start NaN-filled and the input is compared bit for bit after the call (run_op() there).  The table forms run through EVERY supported
mixed-radix length; the array form, the factor forms and the plan variants through one length per structural class (SUBSET) plus every
length that runs a configuration of its own."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import distributedfft_amd as dfft  # noqa: E402

from parity_metric import forward_bound, rms, rms_rel, worst_entry  # noqa: E402
from test_gpu_parity import CDT, NPR  # noqa: E402
from test_gpu_spectral_factors import SCALE, assert_reference_has_something_to_check, factor_args, factor_reference  # noqa: E402
from test_gpu_spectral_op import check, device_multiplier, in_block, make_plans, reference, run_op  # noqa: E402

S = dfft.SPECTRAL_OP
PRECISIONS = ["double", "float"]
TWO = {"spectral_op": 2}
MIXED = {prec: [n for n in range(2, 2049) if n & (n - 1) and dfft.spectral_op_supported(n, prec, 2)] for prec in PRECISIONS}
# one length per structural class: 12 one pass, no LDS, G = 32 | 60 two passes, G > 1 | 250 radix 5.5 | 384, 768, 1536 the de-aliasing sizes |
# 720 four passes, E = 30 | 1000 | 1792 radix 7 | 2000 the largest LDS (fp64) -- and the lengths with a configuration for the fused kernel alone
# (csrc/spectral_mixed.inc: F64_S2000; F32_S384, F32_S480, F32_S1200, F32_S1600)
DEDICATED = {"double": [2000], "float": [384, 480, 1200, 1600]}
SUBSET = {prec: sorted(n for n in set([12, 60, 250, 384, 768, 1536, 720, 1000, 1792, 2000] + DEDICATED[prec]) if n in MIXED[prec]) for prec in PRECISIONS}


def plans_2(shape, P1, P2, prec, c2c, layout, chunks=None, cls=dfft.MPIcuFFT_Pencil_Opt1, options=None, arena=None):
    return make_plans(shape, P1, P2, prec, c2c, layout, chunks=chunks, cls=cls, options=dict(TWO, **(options or {})), arena=arena)


def rows(prec_lengths, *more):
    return [pytest.param(n, prec, *m, id="-".join(map(str, (n, prec) + tuple(m)))) for prec in PRECISIONS for n in prec_lengths[prec] for m in (more or [()])]


def test_the_sweeps_have_their_lengths():
    assert len(MIXED["double"]) == 45 and len(MIXED["float"]) == 47
    assert all(set(DEDICATED[p]) <= set(SUBSET[p]) and len(SUBSET[p]) >= 10 for p in PRECISIONS)


# ---- 1. table forms (kinds 1 and 2): every supported mixed-radix length ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_table_reference(shape, prec, c2c):
    """test_gpu_spectral_op.table_reference() with the seed 20261103 + Nx: integer tables from -3 .. 3, folded for R2C; numpy's answers for
    kind 1 (m = sum / 9) and kind 2 (m = 1 / sum, 0 at a zero sum); the share of zero sums and rho = rms(m U) / rms(U) per kind.  (With that
    function's own seed (2000, 12, 10) R2C has rho = 0.287 and would trip the "something to check" condition below.)"""
    Nx, Ny, Nz = shape
    u = reference(shape, prec, c2c)[0]
    rng = np.random.default_rng(20261103 + Nx)
    ax, ay, az = (rng.integers(-3, 4, n).astype(np.float64) for n in (Nx, Ny, Nz))
    if not c2c:
        fold = lambda t: t[np.minimum(np.arange(t.size), (t.size - np.arange(t.size)) % t.size)]      # noqa: E731
        ax, ay, az = fold(ax), fold(ay), az[:Nz // 2 + 1]
    s = ax[:, None, None] + ay[None, :, None] + az[None, None, :]
    n = float(np.prod(shape))
    U = np.fft.fftn(u) if c2c else np.fft.rfftn(u)
    back = (lambda X: np.fft.ifftn(X) * n) if c2c else (lambda X: np.fft.irfftn(X, s=shape, axes=(0, 1, 2)) * n)
    ms = (s / 9.0, np.where(s != 0, 1.0 / np.where(s != 0, s, 1.0), 0.0))
    wants = tuple(back(U * m) for m in ms)
    for a in (ax, ay, az) + wants:
        a.setflags(write=False)
    return u, (ax, ay, az), wants, float(np.mean(s == 0)), tuple(rms(m * U) / rms(U) for m in ms)


@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("Nx,prec", rows(MIXED))
def test_table_multiplier_every_mixed_length(Nx, prec, c2c):
    """(Nx, 12, 10) over 2 x 2 at pipeline depth 3, kinds 1 and 2, both layouts: tx read at another index than t2 + NT * sigma(c) of the
    length's configuration, a register left out of the multiplier loop (E / CH chunks must cover E), ay without the chunk's first ky row"""
    shape = (Nx, 12, 10)
    u, tables, wants, zero_fraction, rhos = mixed_table_reference(shape, prec, c2c)
    assert zero_fraction >= 0.04, f"only {zero_fraction:.3f} of the spectrum has a zero table sum"
    assert min(rhos) >= 0.3, f"rms(m U) / rms(U) = {rhos}: the multiplier leaves too little of the spectrum"
    for layout in (0, 1):
        plans = plans_2(shape, 2, 2, prec, c2c, layout, chunks=3)
        assert all(pl.getPipelineChunks() == 3 and pl.debugChain(S)[2]["group"] == "xx" and pl.debugChain(S)[2]["launches"] == 3 for pl in plans)
        for kind in (1, 2):
            want = wants[kind - 1]
            assert all(np.any(in_block(pl, want) != 0) for pl in plans), "a rank's expected block is all zeros"
            outs = run_op(plans, prec, c2c, u, tables=tables, reciprocal=kind == 2, scale=1.0 / 9.0 if kind == 1 else 1.0)
            check(plans, outs, want, prec, f"kind {kind} layout {layout}")


# ---- 2. array form (kind 0) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("Nx,prec,P1,P2", rows(SUBSET, (1, 1), (2, 1), (1, 2), (2, 2)))
def test_array_multiplier_against_numpy(Nx, prec, P1, P2, c2c):
    shape = (Nx, 8, 16)
    u, m, want = reference(shape, prec, c2c)
    for layout in (0, 1):
        plans = plans_2(shape, P1, P2, prec, c2c, layout)
        check(plans, run_op(plans, prec, c2c, u, m=m), want, prec, f"layout {layout}")


# ---- 3. factor forms (kinds 3, 4, 5) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("Nx,prec,P1,P2,chunks", rows(SUBSET, (1, 1, 1), (2, 2, 3)))
def test_factor_tables_against_numpy(Nx, prec, P1, P2, chunks, c2c):
    """test_gpu_spectral_factors.factor_reference() as it is (seed 20261019 + Nx): its conditions hold for every length of SUBSET at
    (Nx, 12, 10), C2C and R2C, and are asserted here before anything runs"""
    shape = (Nx, 12, 10)
    u, factors, tables, wants, stats = factor_reference(shape, prec, c2c)
    assert_reference_has_something_to_check(stats)
    for layout in (0, 1):
        plans = plans_2(shape, P1, P2, prec, c2c, layout, chunks=chunks)
        assert all(pl.getPipelineChunks() == chunks and pl.debugChain(S)[2]["launches"] == chunks for pl in plans)
        for kind in (3, 4, 5):
            want = wants[kind - 3]
            assert all(np.any(in_block(pl, want) != 0) for pl in plans), "a rank's expected block is all zeros"
            args = factor_args(plans, prec, factors, tables if kind > 3 else None, reciprocal=kind == 5, scale=SCALE)
            check(plans, run_op(plans, prec, c2c, u, args=args), want, prec, f"kind {kind} layout {layout} depth {chunks}")


# ---- 4. ragged tiles, 5. slab ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("layout", [0, 1])
def test_ragged_tiles(layout, prec):
    """R2C on (60, 24, 38) over 2 x 3: Nzc = 20 -> 7 + 7 + 6 lines per ky row, no tile is full"""
    shape = (60, 24, 38)
    u, m, want = reference(shape, prec, False)
    plans = plans_2(shape, 2, 3, prec, False, layout)
    check(plans, run_op(plans, prec, False, u, m=m), want, prec, "2 x 3")


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
def test_slab_opt1_against_numpy(c2c, prec):
    """MPIcuFFT_Slab_Opt1 with P = 3: the 60 x rows and the 12 ky rows split 20 + 20 + 20 and 4 + 4 + 4; array and table forms, both layouts"""
    shape = (60, 12, 10)
    u, m, want = reference(shape, prec, c2c)
    _, tables, table_wants, _, _ = mixed_table_reference(shape, prec, c2c)
    for layout in (0, 1):
        plans = plans_2(shape, 3, 1, prec, c2c, layout, cls=dfft.MPIcuFFT_Slab_Opt1)
        assert sorted(pl.getInStart()[0] for pl in plans)[1] > 0 and all(pl.getInSize()[1:] == shape[1:] for pl in plans)
        check(plans, run_op(plans, prec, c2c, u, m=m), want, prec, f"slab layout {layout} array")
        check(plans, run_op(plans, prec, c2c, u, tables=tables, scale=1.0 / 9.0), table_wants[0], prec, f"slab layout {layout} tables")
        check(plans, run_op(plans, prec, c2c, u, tables=tables, reciprocal=True), table_wants[1], prec, f"slab layout {layout} reciprocal")


# ---- 6. fused against unfused ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("shape,P1,P2", [((768, 8, 8), 1, 1), ((1000, 8, 16), 1, 2)])
def test_agrees_with_the_unfused_path(shape, P1, P2, prec):
    """same plans, input and multiplier: execR2C -> multiply on spectrumView -> execC2R against the fused call, with the bound of
    test_gpu_spectral_op.test_agrees_with_the_unfused_path"""
    u, m, want = reference(shape, prec, False)
    plans = plans_2(shape, P1, P2, prec, False, 0)
    fused = run_op(plans, prec, False, u, m=m)
    P, esz = len(plans), 16 if prec == "double" else 8
    ins = [torch.from_numpy(in_block(pl, u).astype(NPR[prec])).cuda() for pl in plans]
    specs = [torch.zeros(pl.getDomainSize() // esz, dtype=CDT[prec], device="cuda") for pl in plans]
    backs = [torch.zeros_like(t) for t in ins]
    mults = [device_multiplier(pl, prec, m) for pl in plans]
    torch.cuda.synchronize()
    with ThreadPoolExecutor(P) as ex:
        list(ex.map(lambda r: plans[r].execR2C(specs[r], ins[r]), range(P)))
    for r, pl in enumerate(plans):
        pl.spectrumView(specs[r]).mul_(pl.spectrumView(mults[r]))
    torch.cuda.synchronize()
    with ThreadPoolExecutor(P) as ex:
        list(ex.map(lambda r: plans[r].execC2R(backs[r], specs[r]), range(P)))
    torch.cuda.synchronize()
    n = int(np.prod(shape))
    want_rms, bound = rms(want), 2 * forward_bound(prec, n)
    for r in range(P):
        unfused = backs[r].cpu().numpy().astype(np.float64)
        v = rms_rel(fused[r], unfused, want_rms)
        assert v <= bound, f"rank {r}: fused and unfused differ by {v:.3e} > {bound:.1e}; " + worst_entry(fused[r], unfused, want_rms)


# ---- 7. streams and graph, 8. powers of two under value 2 -----------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 2)])
def test_compute_streams_and_graph_change_no_bit(P1, P2, c2c, prec):
    shape = (60, 24, 20)
    u, m, want = reference(shape, prec, c2c)
    results = {}
    cases = [("cs1", {"compute_streams": 1, "trace": 1}), ("cs2", {"compute_streams": 2, "trace": 1})]
    if P1 * P2 == 1:
        cases += [("graph0", {"graph": 0}), ("graph1", {"graph": 1})]
    for name, options in cases:
        plans = plans_2(shape, P1, P2, prec, c2c, 0, chunks=3, options=options)
        assert plans[0].getPipelineChunks() == 3
        results[name] = run_op(plans, prec, c2c, u, m=m)
        if name == "graph1":      # (a second call is where a plan would replay what it captured in the first)
            again = run_op(plans, prec, c2c, u, m=m)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(again, results[name]))
        if "trace" in options:
            for pl in plans:
                issued = pl.debugTrace(S, 0)
                assert issued and issued == pl.debugTrace(S, 3)
                assert any(o["stream"] == 1 for o in issued) == (name == "cs2")
        if name == "cs1":
            check(plans, results[name], want, prec, "compute_streams 1")
    for name in results:
        for r, (a, b) in enumerate(zip(results[name], results["cs1"])):
            assert a.tobytes() == b.tobytes(), f"{name} rank {r}: differs from the compute_streams = 1 run"


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
def test_a_power_of_two_gives_the_same_bits_under_1_and_2(c2c, prec):
    shape = (64, 24, 20)
    u, m, want = reference(shape, prec, c2c)
    one = make_plans(shape, 2, 2, prec, c2c, 0, chunks=3)
    two = plans_2(shape, 2, 2, prec, c2c, 0, chunks=3)
    assert all(pl.getOption("spectral_op") == v for v, plans in ((1, one), (2, two)) for pl in plans)
    a, b = run_op(one, prec, c2c, u, m=m), run_op(two, prec, c2c, u, m=m)
    check(two, b, want, prec, "value 2")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
