"""Where the kernels read and write: every exec entry point and every kernel family on guarded buffers (tests/guarded.py).

The other GPU tests compare what the kernels compute with the oracle, on exact-size zero-filled tensors from torch's caching
allocator: a store one tile past the end of `out`, `back` or the work area lands in a neighbouring cached block, a load past the end of
`in` reads zeros, a result that depends on what a buffer held before finds zeros there.  Here one case per family -- the shapes and the
family assertions of tests/test_gpu_entry_parity.py, at the smallest shape that reaches the form -- runs through the same runners with
`arena=`: `in`, `out`, `back` and a caller-owned work area of getWorkSizeDevice() bytes (initFFT with allocate=False) each sit between
two guards of max(2 MiB, getDomainSize()) bytes of 0xFF, and every case runs twice on the same plans, once with the payloads of `out`,
`back` and the work area filled with 0xFF (NaN) and once with 0x00.  Asserted on every rank:

  guards   after the forward and again after the inverse exec every guard byte still is 0xFF (in the runners: Arena.check_guards);
  inputs   the input of execR2C, execC2C(FORWARD), the slab sequences, the forward partial transforms and `in` of execSpectralOp is
           bit-identical afterwards (Arena.check_inputs), as include/dfft_c.h promises; the spectrum handed to an inverse is
           documented as destroyed, so only its guards are checked;
  outputs  no NaN in the spectrum block or in the block that comes back (the NaN guards around `in` turn a read outside it that feeds a
           result into a NaN); both blocks bit-identical between the 0xFF and the 0x00 run; the forward block within
           parity_metric's per-entry bound and the round trip within TOL_RT, as in test_gpu_entry_parity.py.  No new tolerance.

What the library leaves in the slack of `out` behind the spectrum block is its own business.  tests/test_cpu_guarded.py shows on CPU
tensors that the arena reports what it is for; profiles/footprint_table.txt has the run times, the guard and work-area sizes
(DFFT_FOOTPRINT_TABLE=<file>) and the findings."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import distributedfft_amd as dfft  # noqa: E402
from oracle import oracle as orc  # noqa: E402

import guarded  # noqa: E402
from parity_metric import check_forward, check_forward_blocks, rms  # noqa: E402
from test_gpu_entry_parity import (PRECS, assert_subtile_axis, centred_input, is_pow2, kind, oracle_spectrum,  # noqa: E402
                                   round_trip_per_entry, subtile_axis_spectrum, SUBTILE_AXIS)
from test_gpu_parity import mixed_lengths, run_distributed, run_distributed_real, run_partial, run_single  # noqa: E402
from test_gpu_round3 import rmixed_lengths, run_single_order  # noqa: E402
import test_gpu_slab_sequences as slabs  # noqa: E402
import test_gpu_spectral_mixed as spectral_mixed  # noqa: E402
import test_gpu_spectral_op as spectral_op  # noqa: E402
import test_gpu_two_level as two_level  # noqa: E402
import test_gpu_variants as variants  # noqa: E402


def both_fills(run, offset256=False):
    """run(arena) with the payload fill 0xFF and then 0x00 on one arena -- the runners keep their plans and buffers in it"""
    arena = guarded.Arena("cuda", offset256=offset256)
    results = []
    for fill in (0xFF, 0x00):
        arena.fill = fill
        results.append(run(arena))
    return results


def written_and_same(nan_run, zero_run, what):
    """per rank: no NaN, and not one bit of difference between the run on NaN-filled and the run on zero-filled buffers"""
    assert len(nan_run) == len(zero_run)
    for r, (a, b) in enumerate(zip(nan_run, zero_run)):
        guarded.assert_written(a, f"{what}, rank {r}, buffers filled with 0xFF")
        guarded.assert_written(b, f"{what}, rank {r}, buffers filled with 0x00")
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), \
            f"{what}, rank {r}: the result depends on what out, back or the work area held before ({int(np.sum(a != b))} of {a.size} entries differ)"


def pencil_case(family, shape, P1, P2, prec, real, options=None, chunks=None, offset256=False):
    n3 = int(np.prod(shape))
    g = centred_input(shape, real, 13 if real else 7)

    def run(arena):
        if real:
            return run_distributed_real(shape, P1, P2, prec, field=g, options=options, chunks=chunks, arena=arena)
        return run_distributed(shape, P1, P2, prec, options=options, chunks=chunks, center=True, arena=arena)

    (plans, ins, spec, backs), (_, _, spec0, backs0) = both_fills(run, offset256)
    what = f"{family}: {shape} {P1}x{P2} {'R2C' if real else 'C2C'} {prec} {options or ''} chunks={chunks}"
    written_and_same(spec, spec0, what + " spectrum")
    written_and_same(backs, backs0, what + " round trip")
    check_forward_blocks(plans, spec, oracle_spectrum(g, prec, real), prec, n3)
    x_rms = rms(g)
    for r in range(P1 * P2):
        round_trip_per_entry(backs[r], ins[r], n3, prec, (what, r), x_rms)
    return plans


def single_case(runner, what, real, spectrum=oracle_spectrum, **kw):
    """the single-rank runners, runner(arena=arena, **kw): (input, spectrum, round trip); spectrum(g, prec, real): the oracle's"""
    prec = kw["prec"]
    (g, got, back), (_, got0, back0) = both_fills(lambda arena: runner(arena=arena, **kw))
    written_and_same([got], [got0], what + " spectrum")
    written_and_same([back], [back0], what + " round trip")
    check_forward(got, spectrum(g, prec, real), prec, g.size)
    round_trip_per_entry(back, g, g.size, prec, what)


# ------------------------------------------------------------------------------------------
# powers of two: one rank; pencil and slab with uneven splits at pipeline depths 1 and 4 and on two compute streams; R2C
# ------------------------------------------------------------------------------------------
DEPTHS = [pytest.param(1, None, id="depth1"), pytest.param(4, None, id="depth4"), pytest.param(4, {"compute_streams": 2}, id="two-streams")]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", [(32, 16, 64), (2, 4, 8)])
def test_power_of_two_c2c_one_rank(shape, prec):
    single_case(run_single, f"one rank {shape} {prec}", False, shape=shape, prec=prec, center=True)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("chunks,options", DEPTHS)
@pytest.mark.parametrize("shape,P1,P2,offset256", [((16, 16, 16), 3, 2, False), ((32, 32, 32), 2, 4, False), ((32, 32, 32), 2, 4, True),
                                                   ((32, 64, 32), 8, 1, False)])
def test_power_of_two_c2c_pencil_and_slab(shape, P1, P2, offset256, chunks, options, prec):
    plans = pencil_case("power of two", shape, P1, P2, prec, False, options=options, chunks=chunks, offset256=offset256)
    assert 1 <= plans[0].getPipelineChunks() <= chunks
    if options:
        assert all(pl.getOption("compute_streams") == 2 for pl in plans)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("chunks,options", DEPTHS)
def test_power_of_two_r2c(chunks, options, prec):
    pencil_case("power of two", (16, 8, 512), 1, 2, prec, True, options=options, chunks=chunks)


# ------------------------------------------------------------------------------------------
# every role variant: 17-wide spectrum rows of odd pitch (R2C 512 x 64 x 32), natural lines on the z passes (C2C 16 x 24 x 512)
# ------------------------------------------------------------------------------------------
def variant_case(shape, P1, P2, prec, real, offset256):
    assert 512 in shape and all(kind(n, prec) == "native" for n in shape)
    n3 = int(np.prod(shape))
    x_rms = rms(centred_input(shape, real, 13 if real else 7))
    for v in variants.VARIANTS[prec]:
        spectra = []

        def run(arena):
            plans, ins, backs, _ = variants.check(shape, P1, P2, prec, v, real, center=True, arena=arena, spectra=spectra)
            return plans, ins, backs, list(spectra)

        (plans, ins, backs, spec), (_, _, backs0, spec0) = both_fills(run, offset256)
        assert all(pl.getOption("variant_" + k) == v for pl in plans for k in variants.PASSES)
        what = f"role variant {v}: {shape} {P1}x{P2} {'R2C' if real else 'C2C'} {prec}"
        written_and_same(spec, spec0, what + " spectrum")
        written_and_same(backs, backs0, what + " round trip")
        for r in range(P1 * P2):
            round_trip_per_entry(backs[r], ins[r], n3, prec, (what, r), x_rms)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("offset256", [False, True], ids=["aligned", "offset256"])
@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 2)])
def test_every_role_variant_on_odd_pitch_rows(P1, P2, offset256, prec):
    variant_case((512, 64, 32), P1, P2, prec, True, offset256)


@pytest.mark.parametrize("prec", PRECS)
def test_every_role_variant_on_the_z_passes(prec):
    variant_case((16, 24, 512), 1, 1, prec, False, False)


# ------------------------------------------------------------------------------------------
# the kernels of the other lengths: mixed radix, packed real mixed z, Bluestein, two levels, long lines, long Bluestein
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_native_mixed_radix_c2c(prec):
    shape = (12, 20, 24)
    if prec == "float" and not all(n in mixed_lengths("float") for n in shape):
        pytest.skip("length without fp32 configuration")
    for n in shape:
        assert not is_pow2(n) and n in mixed_lengths(prec) and kind(n, prec) == "native" and dfft.kernel_info(n, prec) is not None, n
    pencil_case("native mixed radix", shape, 2, 2, prec, False)


@pytest.mark.parametrize("prec", PRECS)
def test_packed_real_mixed_z_pass(prec):
    shape = (6, 10, 200)
    M = shape[2] // 2
    if prec == "float" and M not in rmixed_lengths("F32"):
        pytest.skip("length without fp32 configuration")
    assert not is_pow2(M) and M in rmixed_lengths("F64" if prec == "double" else "F32") and kind(M, prec) == "native", M
    pencil_case("packed real mixed z", shape, 1, 2, prec, True)


@pytest.mark.parametrize("prec", PRECS)
def test_bluestein_axes_c2c(prec):
    for n in (9, 7):
        assert kind(n, prec) == "bluestein", (n, kind(n, prec))
    pencil_case("Bluestein", (9, 7, 10), 3, 2, prec, False)


@pytest.mark.parametrize("prec", PRECS)
def test_bluestein_real_z(prec):
    assert kind(13, prec) == "bluestein"
    pencil_case("Bluestein real z", (10, 9, 13), 3, 1, prec, True)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("real", [False, True], ids=["c2c", "r2c"])
def test_forced_two_level_distributed(real, prec):
    shape = (12, 10, 14)
    for n in shape:
        assert kind(n, prec, 1) == "two_level", n
    pencil_case("forced two-level", shape, 2, 4, prec, real, options={"two_level": 1})


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("real", [False, True], ids=["c2c", "r2c"])
def test_forced_two_level_single_rank(real, prec):
    shape = (16, 256, 10)
    for n in shape:
        assert kind(n, prec, 1) == "two_level", n
    single_case(two_level.single, f"forced two-level: {shape} one rank {'R2C' if real else 'C2C'} {prec}", real,
                shape=shape, prec=prec, c2c=not real, options={"two_level": 1}, center=True)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape,real,axis", [((8200, 8, 6), False, 8200), ((4, 6, 10000), True, 10000)])
def test_long_lines(shape, real, axis, prec):
    assert kind(axis, prec) == "two_level", kind(axis, prec)
    pencil_case("long line", shape, 2, 2, prec, real)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("real", [False, True], ids=["c2c", "r2c"])
def test_long_bluestein_lines(real, prec):
    assert kind(4099, prec) == "long_bluestein"
    pencil_case("long Bluestein", (6, 8, 4099), 2, 3, prec, real)


@pytest.mark.parametrize("prec", PRECS)
def test_long_line_with_a_sub_tile_level_single_rank(prec):
    """(2101248, 2, 3): the scratch between the levels of a 2e6-point line (Bluestein 513 x plain 4096, sub-tile workgroups) within a
    caller-owned work area of exactly getWorkSizeDevice() bytes"""
    shape = (SUBTILE_AXIS, 2, 3)
    assert_subtile_axis(prec)
    single_case(two_level.single, f"long line, sub-tile level: {shape} one rank C2C {prec}", False,
                spectrum=lambda g, p, real: subtile_axis_spectrum(g, shape, p, real), shape=shape, prec=prec, c2c=True, center=True)


# ------------------------------------------------------------------------------------------
# option single_order = 1 (the padded private layout in the work area), option spectral_layout = 1
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape,family", [((32, 64, 24), "native"), ((12, 20, 24), "native"), ((17, 33, 9), "bluestein")])
def test_forced_zxy_order(shape, family, prec):
    assert all(kind(n, "double") == family for n in shape)
    for n in shape:      # a mixed-radix length without fp32 configuration runs Bluestein at fp32
        assert kind(n, prec) == ("native" if family == "native" and (is_pow2(n) or n in mixed_lengths(prec)) else "bluestein"), n
    single_case(run_single_order, f"forced z,x,y order: {shape} {prec}", False,
                shape=shape, prec=prec, options={"single_order": 1}, center=True)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape,P1,P2,real", [((66, 50, 38), 2, 3, False), ((24, 40, 50), 2, 2, True)])
def test_x_contiguous_spectrum(shape, P1, P2, real, prec):
    plans = pencil_case("x-contiguous spectrum", shape, P1, P2, prec, real, options={"spectral_layout": 1})
    for pl in plans:
        s = pl.getOutSize()
        assert pl.getOption("spectral_layout") == 1 and pl.getOutStrides() == (1, s[2] * s[0], s[0])


# ------------------------------------------------------------------------------------------
# slab sequences Z_Then_YX (forward and inverse) and Y_Then_ZX (forward only)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
def test_slab_sequences(c2c, prec):
    shape, P = (33, 20, 18), 4
    n3 = int(np.prod(shape))
    assert {kind(n, prec) for n in shape} <= {"native", "bluestein"} and kind(33, prec) == "bluestein"
    what = f"slab Z_Then_YX: {shape} P={P} {'C2C' if c2c else 'R2C'} {prec}"
    (plans, ins, spec, backs), (_, _, spec0, backs0) = both_fills(
        lambda arena: slabs.run(dfft.MPIcuFFT_Slab_Z_Then_YX, shape, P, prec, c2c, center=True, arena=arena))
    written_and_same(spec, spec0, what + " spectrum")
    written_and_same(backs, backs0, what + " round trip")
    g = slabs.global_input(shape, c2c, prec, center=True)
    check_forward_blocks(plans, spec, orc.fft3d_c2c(g, -1) if c2c else orc.fft3d_r2c(g), prec, n3)
    for r in range(P):
        round_trip_per_entry(backs[r], ins[r], n3, prec, (what, r), rms(g))
    (plans, spec), (_, spec0) = both_fills(lambda arena: slabs.run_yzx(shape, P, prec, c2c, center=True, arena=arena))
    written_and_same(spec, spec0, what.replace("Z_Then_YX", "Y_Then_ZX") + " spectrum")
    g = slabs.global_input(shape, c2c, prec, seed=33, center=True)
    want = orc.fft3d_c2c(np.ascontiguousarray(g.astype(np.complex128)), -1)[:, :(shape[1] if c2c else shape[1] // 2 + 1), :]
    check_forward_blocks(plans, spec, want, prec, n3)


# ------------------------------------------------------------------------------------------
# partial transforms: d = 1 (lines along z), d = 2 ((y, z) planes); the forward ones only read `in` (include/dfft_c.h)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("d", [1, 2])
def test_partial_transforms(d, c2c, prec):
    shape, P1, P2 = (16, 32, 64), 3, 2
    (plans, blocks, ref, ins, backs), (_, blocks0, _, _, backs0) = both_fills(
        lambda arena: run_partial(shape, P1, P2, d, c2c, prec=prec, center=True, arena=arena))
    what = f"partial transform d={d}: {shape} {P1}x{P2} {'C2C' if c2c else 'R2C'} {prec}"
    written_and_same([b[0] for b in blocks], [b[0] for b in blocks0], what + " stage")
    written_and_same(backs, backs0, what + " round trip")
    points = shape[2] if d == 1 else shape[1] * shape[2]
    ref_rms = rms(ref)
    x_rms = rms(np.concatenate([x.ravel() for x in ins]))
    for r, (got, want) in enumerate(blocks):
        check_forward(got, want, prec, points, want_rms=ref_rms)
        round_trip_per_entry(backs[r], ins[r], points, prec, (what, r), x_rms)


# ------------------------------------------------------------------------------------------
# execSpectralOp: `in`, the multiplier array and the tables are only read; `out` is a block of the input layout
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 2)])
@pytest.mark.parametrize("form", ["array", "tables", "mixed-tables"])
def test_exec_spectral_op(form, P1, P2, c2c, prec):
    """a power-of-two x length in the array form (kind 0) and in the table form (kind 1), and the smallest x length that is no power of
    two and has a fused kernel (option spectral_op = 2) in the table form"""
    if form == "mixed-tables":
        Nx = spectral_mixed.MIXED[prec][0]
        assert not is_pow2(Nx) and dfft.spectral_op_supported(Nx, prec, 2) and not any(
            dfft.spectral_op_supported(n, prec, 2) for n in range(2, Nx) if not is_pow2(n))
        shape = (Nx, 12, 10)
        u, tables, wants, _, _ = spectral_mixed.mixed_table_reference(shape, prec, c2c)
        make, op, want = spectral_mixed.plans_2, dict(tables=tables, scale=1.0 / 9.0), wants[0]
    elif form == "tables":
        shape = (64, 12, 10)
        u, tables, wants, _, _ = spectral_op.table_reference(shape, prec, c2c)
        make, op, want = spectral_op.make_plans, dict(tables=tables, scale=1.0 / 9.0), wants[0]
    else:
        shape = (64, 12, 10)
        u, m, want = spectral_op.reference(shape, prec, c2c)
        make, op = spectral_op.make_plans, dict(m=m)

    def run(arena):
        plans = arena.once("plans", lambda: make(shape, P1, P2, prec, c2c, 0, arena=arena))
        return plans, spectral_op.run_op(plans, prec, c2c, u, arena=arena, **op)

    (plans, outs), (_, outs0) = both_fills(run)
    what = f"execSpectralOp {form}: {shape} {P1}x{P2} {'C2C' if c2c else 'R2C'} {prec}"
    assert all(pl.debugChain(dfft.SPECTRAL_OP)[2]["group"] == "xx" for pl in plans)
    written_and_same(outs, outs0, what)
    spectral_op.check(plans, outs, want, prec, what)
