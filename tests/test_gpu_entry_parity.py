"""Every kernel family of libdfft_amd_any.so and every option-forced form, per entry, on ZERO-MEAN input, fp64 and fp32.

The per-entry forward bound of parity_metric.py,  max_k |err[k]| / max(|want[k]|, rms(want)) <= RMS_TOL[prec] * log2(points),  is
asserted at fp32 on zero-mean input only (module docstring there), and the 3-D tests of the families below -- mixed radix, packed
real mixed, Bluestein, two-level, long lines, long Bluestein, the forced z, x, y order, the x-contiguous spectrum, the slab sequences,
partial transforms, every role variant -- feed the reference's non-negative distribution.  Here each family runs once more on the
same input centred (uniform - 127.5), at the smallest shape that still reaches the form, through the runners of the existing files:
forward per entry against the oracle on every rank (factor 1: the bound is parity_metric.forward_bound itself), the old bound scaled
by max|X| beside it, and the round trip per entry, max|back / n - x| / rms(x), against the round-trip tolerance of test_gpu_parity.py.
Each case first asserts through axis_plan_info / kernel_info that the axis it names runs the family it is listed for.

profiles/entry_parity_table.txt holds the measured values (DFFT_PARITY_TABLE), profiles/entry_parity_mutation.txt the proof that
these assertions fail when the fp64 tables (twiddles, Bluestein chirp and bhat) are rounded through fp32."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import distributedfft_amd as dfft  # noqa: E402
from oracle import oracle as orc  # noqa: E402

from parity_metric import CENTER, check_forward, check_forward_blocks, rms  # noqa: E402
from test_gpu_parity import (NPDT, NPR, TOL_FWD, TOL_RT, mixed_lengths, rel, run_distributed, run_distributed_real,  # noqa: E402
                             run_partial)
from test_gpu_round3 import rmixed_lengths, run_single_order  # noqa: E402
import test_gpu_slab_sequences as slabs  # noqa: E402
import test_gpu_two_level as two_level  # noqa: E402
import test_gpu_variants as variants  # noqa: E402

PRECS = ["double", "float"]


def kind(N, prec, forced=0):
    info = dfft.axis_plan_info(N, prec, forced)
    assert info is not None, N
    return info["kind"]


def is_pow2(n):
    return n & (n - 1) == 0


@functools.lru_cache(maxsize=2)
def centred_input(shape, real, seed):
    """the global input of run_distributed (seed 7) / run_distributed_real (seed 13) with center / the centred field, in fp64"""
    return orc.fill_block(shape, (0, 0, 0), shape, 1 if real else 2, seed=seed) - (CENTER if real else CENTER * (1 + 1j))


def oracle_spectrum(g, prec, real):
    """the oracle's transform of the input as the device holds it (rounded to the plan's precision)"""
    if real:
        return orc.fft3d_r2c(g.astype(NPR[prec]).astype(np.float64))
    return orc.fft3d_c2c(g.astype(NPDT[prec]).astype(np.complex128), -1)


def round_trip_per_entry(back, x, n, prec, what, x_rms=None):
    """max|back / n - x| / rms(x): every entry of the round trip against the typical input entry (the centred input has no large one);
    x_rms: the rms of the whole input when x is one rank's block"""
    v = float(np.max(np.abs(back / float(n) - x))) / (x_rms if x_rms is not None else rms(x))
    assert v < TOL_RT[prec], (what, v)


def pencil_case(family, shape, P1, P2, prec, real, options=None):
    """one centred pencil / slab-as-pencil run: forward per entry on every rank, the old bound, the round trip per entry"""
    n3 = int(np.prod(shape))
    g = centred_input(shape, real, 13 if real else 7)
    if real:
        plans, ins, spec, backs = run_distributed_real(shape, P1, P2, prec, field=g, options=options)
    else:
        plans, ins, spec, backs = run_distributed(shape, P1, P2, prec, options=options, center=True)
    want = oracle_spectrum(g, prec, real)
    check_forward_blocks(plans, spec, want, prec, n3, label=f"{family}: {shape} {P1}x{P2} {'R2C' if real else 'C2C'} {options or ''} centred")
    x_rms = rms(g)
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert np.max(np.abs(spec[r] - want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]])) / np.max(np.abs(want)) < TOL_FWD[prec]
        round_trip_per_entry(backs[r], ins[r], n3, prec, (shape, P1, P2, r), x_rms)
    return plans


# ------------------------------------------------------------------------------------------
# native mixed-radix chain, C2C
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape,P1,P2", [((12, 20, 24), 2, 2), ((48, 36, 40), 2, 3)])
def test_native_mixed_radix_c2c(shape, P1, P2, prec):
    if prec == "float" and not all(n in mixed_lengths("float") for n in shape):
        pytest.skip("length without fp32 configuration")
    for n in shape:
        assert not is_pow2(n) and n in mixed_lengths(prec) and kind(n, prec) == "native" and dfft.kernel_info(n, prec) is not None, n
    pencil_case("native mixed radix", shape, P1, P2, prec, False)


# ------------------------------------------------------------------------------------------
# packed real z pass of the mixed-radix lengths (Nz / 2 points + Hermitian split / merge: table tw_zr)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape,P1,P2", [((6, 10, 200), 1, 2), ((6, 12, 1536), 1, 1)])
def test_packed_real_mixed_z_pass(shape, P1, P2, prec):
    M = shape[2] // 2
    if prec == "float" and M not in rmixed_lengths("F32"):
        pytest.skip("length without fp32 configuration")
    assert not is_pow2(M) and M in rmixed_lengths("F64" if prec == "double" else "F32") and kind(M, prec) == "native", M
    pencil_case("packed real mixed z", shape, P1, P2, prec, True)


# ------------------------------------------------------------------------------------------
# Bluestein axes (chirp and bhat tables), C2C; real z lines of odd and even length through the Bluestein kernel's real modes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape,P1,P2,blue", [((9, 7, 10), 3, 2, (9, 7)), ((17, 33, 9), 1, 1, (17, 33, 9))])
def test_bluestein_axes_c2c(shape, P1, P2, blue, prec):
    for n in blue:
        assert kind(n, prec) == "bluestein", (n, kind(n, prec))
    pencil_case("Bluestein", shape, P1, P2, prec, False)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape,P1,P2", [((10, 9, 13), 3, 1), ((12, 10, 14), 2, 4)])
def test_bluestein_real_z(shape, P1, P2, prec):
    Nz = shape[2]
    assert kind(Nz, prec) == "bluestein" and (Nz % 2 or Nz // 2 not in rmixed_lengths("F64" if prec == "double" else "F32")), Nz
    pencil_case("Bluestein real z", shape, P1, P2, prec, True)


# ------------------------------------------------------------------------------------------
# option two_level = 1: two launches of the generic kernel with the inter-level twiddles twN
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("real", [False, True])
def test_forced_two_level_distributed(real, prec):
    shape, P1, P2 = (12, 10, 14), 2, 4
    for n in shape:
        assert kind(n, prec, 1) == "two_level", n
    pencil_case("forced two-level", shape, P1, P2, prec, real, options={"two_level": 1})


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("real", [False, True])
def test_forced_two_level_single_rank(real, prec):
    shape = (16, 256, 10)
    for n in shape:
        assert kind(n, prec, 1) == "two_level", n
    g, got, back = two_level.single(shape, prec, not real, {"two_level": 1}, center=True)
    want = oracle_spectrum(g, prec, real)
    check_forward(got, want, prec, g.size, label=f"forced two-level: {shape} one rank {'R2C' if real else 'C2C'} centred")
    assert rel(got, want) < TOL_FWD[prec]
    round_trip_per_entry(back, g, g.size, prec, shape)


# ------------------------------------------------------------------------------------------
# long lines (two levels by themselves) and long Bluestein lines (four launches)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape,real,axis", [((8200, 8, 6), False, 8200), ((4, 6, 10000), True, 10000)])
def test_long_lines(shape, real, axis, prec):
    assert kind(axis, prec) == "two_level", kind(axis, prec)
    pencil_case("long line", shape, 2, 2, prec, real)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("real", [False, True])
def test_long_bluestein_lines(real, prec):
    assert kind(4099, prec) == "long_bluestein"
    pencil_case("long Bluestein", (6, 8, 4099), 2, 3, prec, real)


# ------------------------------------------------------------------------------------------
# a 2101248-point axis = Bluestein 513 x plain 4096: the shortest line with a plain sub-tile level (the workgroups of the 4096- and
# 8192-point transforms take part of a tile's lines each), which every power of two from 2^23 on needs.  As the x axis of a C2C plan
# (the pass's own strided address forms on the outer sides of the levels), as the real z axis (real_mode 1 and 2 of the two levels
# with N / 2 + 1 spectral points) and under a 2 x 2 partition (segmented, chunked address forms on the outer sides).  The kernel-level
# cases of the same form: test_gpu_two_level.py LONG_FORMS; on guarded buffers: test_gpu_footprint.py.
# ------------------------------------------------------------------------------------------
SUBTILE_AXIS = 2101248
SUBTILE_LEVELS = [(513, 2048, True), (4096, 4096, False)]
SUBTILE_SPECTRA = {}


def subtile_axis_spectrum(g, shape, prec, real):
    """the oracle's spectrum of two_level.single's centred input g (seed 5); the C2C ones are kept for test_gpu_footprint.py, which
    runs the same shape (4 s of oracle each)"""
    key = (tuple(shape), prec, real)
    if key in SUBTILE_SPECTRA:
        return SUBTILE_SPECTRA[key]
    want = oracle_spectrum(g, prec, real)
    if not real:
        SUBTILE_SPECTRA[key] = want
    return want


def assert_subtile_axis(prec):
    info = dfft.axis_plan_info(SUBTILE_AXIS, prec)
    assert info is not None and info["kind"] == "two_level" and info["levels"] == SUBTILE_LEVELS, info


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape,real", [((SUBTILE_AXIS, 2, 3), False), ((2, 3, SUBTILE_AXIS), True)])
def test_sub_tile_level_axis_single_rank(shape, real, prec):
    assert_subtile_axis(prec)
    g, got, back = two_level.single(shape, prec, not real, center=True)
    want = subtile_axis_spectrum(g, shape, prec, real)
    check_forward(got, want, prec, g.size, label=f"long line, sub-tile level: {shape} one rank {'R2C' if real else 'C2C'} centred")
    assert rel(got, want) < TOL_FWD[prec]
    round_trip_per_entry(back, g, g.size, prec, shape)


@pytest.mark.parametrize("prec", PRECS)
def test_sub_tile_level_axis_distributed(prec):
    assert_subtile_axis(prec)
    pencil_case("long line, sub-tile level", (SUBTILE_AXIS, 2, 4), 2, 2, prec, False)


# ------------------------------------------------------------------------------------------
# option single_order = 1: the single-rank pass order z, x, y
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape,family", [((32, 64, 24), "native"), ((12, 20, 24), "native"), ((17, 33, 9), "bluestein")])
def test_forced_zxy_order(shape, family, prec):
    """ragged power-of-two tiles, mixed-radix axes, Bluestein axes (ZXY_FAMILY_SHAPES of conftest.py)"""
    assert all(kind(n, "double") == family for n in shape)
    for n in shape:      # a mixed-radix length without fp32 configuration runs Bluestein at fp32, as in the existing test
        assert kind(n, prec) == ("native" if family == "native" and (is_pow2(n) or n in mixed_lengths(prec)) else "bluestein"), n
    g, got, back = run_single_order(shape, prec, {"single_order": 1}, center=True)
    want = oracle_spectrum(g, prec, False)
    check_forward(got, want, prec, g.size, label=f"forced z,x,y order: {shape} one rank C2C centred")
    assert rel(got, want) < 2 * TOL_FWD[prec]
    round_trip_per_entry(back, g, g.size, prec, shape)


# ------------------------------------------------------------------------------------------
# option spectral_layout = 1: the x-contiguous spectrum block
# ------------------------------------------------------------------------------------------
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
@pytest.mark.parametrize("c2c", [True, False])
def test_slab_sequences(c2c, prec):
    shape, P = (33, 20, 18), 4
    n3 = int(np.prod(shape))
    assert {kind(n, prec) for n in shape} <= {"native", "bluestein"} and kind(33, prec) == "bluestein"
    plans, ins, spec, backs = slabs.run(dfft.MPIcuFFT_Slab_Z_Then_YX, shape, P, prec, c2c, center=True)
    g = slabs.global_input(shape, c2c, prec, center=True)
    want = orc.fft3d_c2c(g, -1) if c2c else orc.fft3d_r2c(g)
    check_forward_blocks(plans, spec, want, prec, n3, label=f"slab Z_Then_YX: {shape} P={P} {'C2C' if c2c else 'R2C'} centred")
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert np.max(np.abs(spec[r] - want[:, :, o[2]:o[2] + s[2]])) / np.max(np.abs(want)) < TOL_FWD[prec]
        round_trip_per_entry(backs[r], ins[r], n3, prec, r, rms(g))
    plans, spec = slabs.run_yzx(shape, P, prec, c2c, center=True)
    g = slabs.global_input(shape, c2c, prec, seed=33, center=True)
    want = orc.fft3d_c2c(np.ascontiguousarray(g.astype(np.complex128)), -1)[:, :(shape[1] if c2c else shape[1] // 2 + 1), :]
    check_forward_blocks(plans, spec, want, prec, n3, label=f"slab Y_Then_ZX: {shape} P={P} {'C2C' if c2c else 'R2C'} centred")
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert np.max(np.abs(spec[r] - want[:, o[1]:o[1] + s[1], :])) / np.max(np.abs(want)) < TOL_FWD[prec]


# ------------------------------------------------------------------------------------------
# partial transforms: d = 1 (lines along z), d = 2 ((y, z) planes)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("c2c", [True, False])
@pytest.mark.parametrize("d", [1, 2])
def test_partial_transforms(d, c2c, prec):
    shape, P1, P2 = (16, 32, 64), 3, 2
    plans, blocks, ref, ins, backs = run_partial(shape, P1, P2, d, c2c, prec=prec, center=True)
    points = shape[2] if d == 1 else shape[1] * shape[2]
    ref_rms, scale = rms(ref), np.max(np.abs(ref))
    x_rms = rms(np.concatenate([x.ravel() for x in ins]))
    for r, (got, want) in enumerate(blocks):
        check_forward(got, want, prec, points, want_rms=ref_rms,
                      label=f"partial transform d={d}: {shape} {P1}x{P2} {'C2C' if c2c else 'R2C'} centred" if r == 0 else None)
        assert np.max(np.abs(got - want)) / scale < TOL_FWD[prec]
        round_trip_per_entry(backs[r], ins[r], points, prec, r, x_rms)


# ------------------------------------------------------------------------------------------
# every role variant on every pass (test_gpu_variants.py), 1 x 1 and 2 x 2
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape,real", [((512, 512, 16), False), ((16, 24, 512), False), ((512, 64, 32), True)])
def test_every_role_variant(shape, real, prec):
    """(512, 512, 16): tiled / transposed-tile / point-major forms on the y and x passes; (16, 24, 512): natural lines on the z passes;
    R2C (512, 64, 32): 17-wide spectrum rows of odd pitch"""
    assert 512 in shape and all(kind(n, prec) == "native" for n in shape)      # the variants are configurations of the native 512-point pass
    n3 = int(np.prod(shape))
    x_rms = rms(centred_input(shape, real, 13 if real else 7))
    for v in variants.VARIANTS[prec]:
        for P1, P2 in ((1, 1), (2, 2)):
            last = v == variants.VARIANTS[prec][-1]
            plans, ins, backs, _ = variants.check(shape, P1, P2, prec, v, real, center=True,
                                                  label=f"role variant {v}: {shape} {P1}x{P2} {'R2C' if real else 'C2C'} centred" if last or v == 1 else None)
            assert all(pl.getOption("variant_" + k) == v for pl in plans for k in variants.PASSES)
            for r in range(P1 * P2):
                round_trip_per_entry(backs[r], ins[r], n3, prec, (v, P1, P2, r), x_rms)
