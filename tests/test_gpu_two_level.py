"""Two-level lines (N = N1*N2 over two launches of the generic kernel: csrc/fft_pass.hip.h "Two-level lines", dfft.hip
axis_plan_two_level): the lengths that have no kernel of their own -- beyond 8192, beyond 4096 when not a power of two --
which the reference takes through cuFFT (mpicufft_pencil_opt1.cpp:165-197: cufftMakePlanMany64 accepts any size).

* kernel level: natural lines, both directions, both precisions, forced on short lengths (variant -2: every pairing of
  plain and Bluestein levels) and by itself on long ones; at the end of the file the forms of a level that only lines beyond
  131072 points have (plain levels of 1024 ... 8192 points, long Bluestein over 2^20 ... 2^24 padded points) up to the top of
  the documented range, 2^24 points, against numpy in long double;
* plans: long axes in every position, C2C and R2C (the real modes of the two levels), on one rank and distributed;
* option two_level = 1 forces the two-level form on small grids for every pipeline (pencil, slab, the two slab
  sequences, chunked exchanges, partial transforms), compared with the oracle and with the one-launch kernels.

Tolerances as in test_gpu_parity.py (fp64 1e-11 forward / 1e-10 round trip, fp32 1e-4 / 5e-5), relaxed by sqrt-ish growth on
the lines of 10^4 .. 10^5 points where stated."""
import functools
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import distributedfft_amd as dfft  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from parity_metric import CENTER, check_forward, check_forward_blocks  # noqa: E402
from test_gpu_parity import NPDT, rel, run_distributed, run_distributed_real  # noqa: E402
import test_gpu_slab_sequences as slabs  # noqa: E402

FORCED = [4, 6, 8, 9, 15, 16, 21, 64, 100, 121, 256, 1000, 1024, 1155, 2048, 3000, 4096, 6 * 1024, 8192]
LONG = [4098, 5000, 6000, 9999, 10000, 12288, 16384, 20000, 65536, 3 * 4093, 100000, 131072]


def fft1d_case(N, prec, variant, batch, big_prime=False, label=None):
    """the reference's distribution and the same centred (zero mean), both directions: the old bound scaled by max|X|, and per entry
    (parity_metric.py; at fp32 asserted on the centred input).  `label`: rows of the parity table for this length"""
    rng = np.random.default_rng(N)
    x0 = rng.uniform(0, 255, (batch, N)) + 1j * rng.uniform(0, 255, (batch, N))
    grow = max(1.0, np.log2(N) / 12.0)
    for centred, x in ((False, x0.astype(NPDT[prec])), (True, (x0 - CENTER * (1 + 1j)).astype(NPDT[prec]))):
        d_in = torch.from_numpy(x).cuda()
        d_out = torch.zeros_like(d_in)
        for direction in (dfft.FORWARD, dfft.INVERSE):
            torch.cuda.synchronize()
            dfft.fft1d_batched(d_out, d_in, N, batch, direction, prec, variant=variant)
            torch.cuda.synchronize()
            ref = np.fft.fft(x.astype(np.complex128), axis=-1) if direction == dfft.FORWARD else np.fft.ifft(x.astype(np.complex128), axis=-1) * N
            if big_prime:      # the oracle transforms a prime length as an O(N^2) sum (65537 points: 25 s per case): pocketfft alone here
                want = ref
            else:
                want = orc.fft1d(x.astype(np.complex128), direction)
                assert rel(want, ref) < 1e-12      # independent cross-check of the oracle itself on these lengths
            check_forward(d_out.cpu().numpy(), want, prec, N, zero_mean=centred,
                          label=f"{label} fft1d N={N} dir={direction} centred={centred}" if label else None)
            assert rel(d_out.cpu().numpy(), want) < (2e-11 if prec == "double" else 2e-4) * grow
        assert np.array_equal(d_in.cpu().numpy(), x), "the pass must not modify its input"


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("N", FORCED)
def test_fft1d_two_level_forced_vs_oracle(N, prec):
    """variant -2: two levels wherever the length splits -- plain x plain (64, 1024), plain x Bluestein (6, 3000),
    Bluestein x Bluestein (15, 121, 1155).  No sub-tile level here: the cost model avoids 8192 = 4096 x 2, and 6144 runs
    48 x 128; the sub-tile workgroups of a 4096- or 8192-point level are held by the lengths of LONG_FORMS below"""
    fft1d_case(N, prec, -2, 45 if N < 4096 else 19, label="forced two-level" if N == FORCED[-1] else None)


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("N", LONG)
def test_fft1d_long_lines_vs_oracle(N, prec):
    """lengths without a kernel of their own take the two-level form by themselves (ragged batch: not a multiple of the tile)"""
    fft1d_case(N, prec, 0, 11 if N < 50000 else 5, label="long line" if N == LONG[-1] else None)


LONG_BLUESTEIN = [4099, 8198, 5003, 10007, 12289, 2 * 3 * 4099, 65537]


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("N", LONG_BLUESTEIN)
def test_fft1d_long_bluestein_lines_vs_oracle(N, prec):
    """lengths that neither fit one launch nor split into two factors within its reach -- a prime above 4096 (4099, 5003, 10007,
    12289, 65537), a small multiple of one (8198, 24594) -- run Bluestein's algorithm with M-point transforms that are two-level
    lines themselves (four launches of the generic kernel, dfft.hip launch_long_bluestein).  The reference takes such sizes through
    cuFFT like any other (mpicufft_pencil_opt1.cpp:165-197)."""
    assert dfft.axis_plan_info(N, prec)["kind"] == "long_bluestein"
    fft1d_case(N, prec, 0, 7 if N < 20000 else 3, big_prime=N > 20000, label="long Bluestein" if N == LONG_BLUESTEIN[-1] else None)


def test_every_length_has_a_plan_and_absurd_ones_fail_loudly():
    """every length from 2 to 2^23 has a plan now; beyond the 32-bit point indices of the kernel (2^24) there is none"""
    for N in (2, 3, 4099, 8191 * 3, 99991, 1000003, (1 << 23) - 15):
        assert dfft.axis_plan_info(N, "double") is not None
    plan = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), precision="double")
    with pytest.raises(dfft.DfftError, match="unsupported axis length"):
        plan.initFFT(dfft.GlobalSize((1 << 24) + 1, 4, 4), dfft.Pencil_Partition(1, 1), False, c2c=True)


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False])
@pytest.mark.parametrize("shape", [(4099, 4, 6), (3, 4099, 8), (5, 4, 4099), (6, 5, 8198), (8198, 3, 10)])
def test_single_rank_long_bluestein_axes_vs_oracle(shape, c2c, prec):
    """a long-Bluestein axis in every position; R2C: real input lines of an odd (4099) and an even (8198) prime-ridden length"""
    g, got, back = single(shape, prec, c2c)
    want = orc.fft3d_c2c(g.astype(np.complex128), -1) if c2c else orc.fft3d_r2c(g.astype(np.float64))
    assert rel(got, want) < (4e-11 if prec == "double" else 4e-4)
    check_forward(got, want, prec, g.size, zero_mean=False)
    assert rel(back / g.size, g) < (2e-10 if prec == "double" else 1e-4)


@pytest.mark.parametrize("c2c", [True, False])
@pytest.mark.parametrize("shape,P1,P2,chunks", [((4099, 8, 12), 2, 2, 2), ((8, 4099, 6), 2, 2, 1), ((6, 8, 4099), 2, 3, 2), ((4099, 6, 8), 3, 1, 3)])
def test_distributed_long_bluestein_axes_vs_oracle(shape, P1, P2, chunks, c2c):
    """... distributed: the first and the last launch carry the pass's own (segmented, chunked) address forms"""
    prec = "double"
    if c2c:
        plans, ins, spec, backs = run_distributed(shape, P1, P2, prec, chunks=chunks)
        g = orc.fill_block(shape, (0, 0, 0), shape, 2, seed=7).astype(np.complex128)
        want = orc.fft3d_c2c(g, -1)
    else:
        plans, ins, spec, backs = run_distributed_real(shape, P1, P2, prec)
        g = orc.fill_block(shape, (0, 0, 0), shape, 1, seed=13).astype(np.float64)
        want = orc.fft3d_r2c(g)
    scale = np.max(np.abs(want))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert np.max(np.abs(spec[r] - want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]])) / scale < 4e-11
        assert rel(backs[r] / float(np.prod(shape)), ins[r]) < 2e-10
    check_forward_blocks(plans, spec, want, prec, g.size, zero_mean=False)


def single(shape, prec, c2c, options=None, seed=5, center=False, arena=None):
    """arena: as in test_gpu_parity.run_single"""
    cdt = torch.complex128 if prec == "double" else torch.complex64
    esz = 16 if prec == "double" else 8
    g = orc.fill_block(shape, (0, 0, 0), shape, 2 if c2c else 1, seed=seed)
    if center:
        g = g - (CENTER * (1 + 1j) if c2c else CENTER)
    g = g.astype(NPDT[prec]) if c2c else g.astype(np.float64 if prec == "double" else np.float32)

    def setup():
        plan = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), precision=prec)
        for k, v in (options or {}).items():
            plan.setOption(k, v)
        plan.initFFT(dfft.GlobalSize(*shape), dfft.Pencil_Partition(1, 1), arena is None, c2c=c2c)
        if arena is not None:
            return (plan,) + arena.plan_buffers(plan, g, cdt)
        d_in = torch.from_numpy(g).cuda()
        return plan, d_in, torch.zeros(plan.getDomainSize() // esz, dtype=cdt, device="cuda"), torch.zeros_like(d_in)

    plan, d_in, d_out, d_back = setup() if arena is None else arena.once("two_level.single", setup)
    what = f"two_level.single {shape} {prec} {'C2C' if c2c else 'R2C'} {options or ''}"
    if arena is not None:
        arena.refill()
    torch.cuda.synchronize()
    if c2c:
        plan.execC2C(d_out, d_in, dfft.FORWARD)
    else:
        plan.execR2C(d_out, d_in)
    s = plan.getOutSize()
    got = d_out[:s[0] * s[1] * s[2]].cpu().numpy().reshape(s)
    assert np.array_equal(d_in.cpu().numpy(), g), "forward must not modify its input"
    if arena is not None:
        arena.check_guards(what + " forward")
        arena.check_inputs(what + " forward")
        arena.refill(keep=[d_out])
    torch.cuda.synchronize()
    if c2c:
        plan.execC2C(d_back, d_out, dfft.INVERSE)
    else:
        plan.execC2R(d_back, d_out)
    torch.cuda.synchronize()
    if arena is not None:
        arena.check_guards(what + " inverse")
    return g, got, d_back.cpu().numpy()


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False])
@pytest.mark.parametrize("shape", [(16384, 4, 6), (3, 10000, 8), (5, 4, 16384), (9, 3, 10000), (2, 3, 9999), (12288, 5, 20),
                                   (4100, 2, 5000)])
def test_single_rank_long_axes_vs_oracle(shape, c2c, prec):
    """a long axis in every position; R2C: the real modes of the two levels (even and odd Nz)"""
    g, got, back = single(shape, prec, c2c)
    want = orc.fft3d_c2c(g.astype(np.complex128), -1) if c2c else orc.fft3d_r2c(g.astype(np.float64))
    assert rel(got, want) < (4e-11 if prec == "double" else 4e-4)
    check_forward(got, want, prec, g.size, zero_mean=False)
    assert rel(back / g.size, g) < (2e-10 if prec == "double" else 1e-4)


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False])
@pytest.mark.parametrize("shape", [(8, 8, 8), (12, 10, 14), (64, 64, 64), (30, 16, 50), (9, 15, 21), (128, 4, 36), (16, 256, 10)])
def test_single_rank_forced_two_level_vs_oracle(shape, c2c, prec):
    """option two_level = 1: every axis that splits runs in two levels (primes keep Bluestein), on both pass orders of a
    single rank; equal to the oracle and, to rounding, to the plan without the option"""
    g, got, back = single(shape, prec, c2c, {"two_level": 1})
    want = orc.fft3d_c2c(g.astype(np.complex128), -1) if c2c else orc.fft3d_r2c(g.astype(np.float64))
    assert rel(got, want) < (2e-11 if prec == "double" else 2e-4)
    check_forward(got, want, prec, g.size, zero_mean=False)
    assert rel(back / g.size, g) < (1e-10 if prec == "double" else 5e-5)
    _, plain, _ = single(shape, prec, c2c)
    assert rel(got, plain) < (2e-11 if prec == "double" else 2e-4)
    if c2c:
        g2, got2, back2 = single(shape, prec, c2c, {"two_level": 1, "single_order": 1})
        assert rel(got2, want) < (2e-11 if prec == "double" else 2e-4)
        check_forward(got2, want, prec, g.size, zero_mean=False)
        assert rel(back2 / g.size, g) < (1e-10 if prec == "double" else 5e-5)


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("shape,P1,P2,chunks", [((16, 16, 16), 2, 2, None), ((32, 32, 32), 2, 4, 2), ((12, 10, 14), 2, 4, None),
                                                ((64, 32, 16), 4, 2, 4), ((30, 20, 18), 3, 1, None), ((16, 32, 16), 1, 4, 1),
                                                ((64, 64, 64), 3, 5, None)])
def test_distributed_forced_two_level_vs_oracle(shape, P1, P2, chunks, prec):
    """pencil and slab pipelines with segmented (multi-peer, chunked) loads and stores on two-level axes, C2C and R2C"""
    opts = {"two_level": 1}
    plans, ins, spec, backs = run_distributed(shape, P1, P2, prec, chunks=chunks, options=opts)
    want = orc.fft3d_c2c(orc.fill_block(shape, (0, 0, 0), shape, 2, seed=7).astype(NPDT[prec]).astype(np.complex128), -1)
    n3 = float(np.prod(shape))
    tf, tr = (2e-11, 1e-10) if prec == "double" else (2e-4, 5e-5)
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        ref = want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]]
        assert np.max(np.abs(spec[r] - ref)) / np.max(np.abs(want)) < tf
        assert rel(backs[r] / n3, ins[r]) < tr
    check_forward_blocks(plans, spec, want, prec, int(n3), zero_mean=False)
    plans, ins, spec, backs = run_distributed_real(shape, P1, P2, prec, options=opts)
    rdt = np.float64 if prec == "double" else np.float32
    wantr = orc.fft3d_r2c(orc.fill_block(shape, (0, 0, 0), shape, 1, seed=13).astype(rdt).astype(np.float64))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        ref = wantr[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]]
        assert np.max(np.abs(spec[r] - ref)) / np.max(np.abs(wantr)) < tf
        assert rel(backs[r] / n3, ins[r]) < tr
    check_forward_blocks(plans, spec, wantr, prec, int(n3), zero_mean=False)


@pytest.mark.parametrize("shape,P1,P2", [((8200, 8, 6), 2, 2), ((6, 9000, 10), 2, 2), ((4, 6, 10000), 2, 2), ((16384, 4, 8), 4, 1)])
def test_distributed_long_axes_vs_oracle(shape, P1, P2):
    """long axes under a partition (uneven splits included), C2C and R2C, fp64"""
    plans, ins, spec, backs = run_distributed(shape, P1, P2, "double")
    want = orc.fft3d_c2c(orc.fill_block(shape, (0, 0, 0), shape, 2, seed=7), -1)
    n3 = float(np.prod(shape))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        ref = want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]]
        assert np.max(np.abs(spec[r] - ref)) / np.max(np.abs(want)) < 4e-11
        assert rel(backs[r] / n3, ins[r]) < 2e-10
    check_forward_blocks(plans, spec, want, "double", int(n3), zero_mean=False)
    plans, ins, spec, backs = run_distributed_real(shape, P1, P2, "double")
    wantr = orc.fft3d_r2c(orc.fill_block(shape, (0, 0, 0), shape, 1, seed=13))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        ref = wantr[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]]
        assert np.max(np.abs(spec[r] - ref)) / np.max(np.abs(wantr)) < 4e-11
        assert rel(backs[r] / n3, ins[r]) < 2e-10
    check_forward_blocks(plans, spec, wantr, "double", int(n3), zero_mean=False)


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False])
@pytest.mark.parametrize("shape,P", [((16, 16, 16), 2), ((33, 20, 18), 4), ((24, 10, 20), 4), ((64, 32, 16), 8)])
def test_slab_sequences_forced_two_level(shape, P, c2c, prec):
    """Z_Then_YX (forward and inverse) and Y_Then_ZX (forward; R2C along y: real lines at a stride) on two-level axes"""
    tf, tr = (2e-11, 1e-10) if prec == "double" else (2e-4, 5e-5)
    plans, ins, spec, backs = slabs.run(dfft.MPIcuFFT_Slab_Z_Then_YX, shape, P, prec, c2c, options={"two_level": 1})
    g = slabs.global_input(shape, c2c, prec)
    want = orc.fft3d_c2c(g, -1) if c2c else orc.fft3d_r2c(g)
    n3 = float(np.prod(shape))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert np.max(np.abs(spec[r] - want[:, :, o[2]:o[2] + s[2]])) / np.max(np.abs(want)) < tf
        assert np.max(np.abs(backs[r] / n3 - ins[r])) / 255.0 < tr
    check_forward_blocks(plans, spec, want, prec, int(n3), zero_mean=False)
    plans, spec = slabs.run_yzx(shape, P, prec, c2c, options={"two_level": 1})
    g = slabs.global_input(shape, c2c, prec, seed=33)
    want = orc.fft3d_c2c(np.ascontiguousarray(g.astype(np.complex128)), -1)
    want = want[:, :(shape[1] if c2c else shape[1] // 2 + 1), :]
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert np.max(np.abs(spec[r] - want[:, o[1]:o[1] + s[1], :])) / np.max(np.abs(want)) < tf
    check_forward_blocks(plans, spec, want, prec, int(n3), zero_mean=False)


def test_work_area_holds_the_level_scratch():
    """getWorkSizeDevice grows by the scratch between the levels, and a caller-owned work area of that size is enough"""
    shape = (10000, 6, 8)
    sizes = {}
    for name, shp in (("long", shape), ("short", (1000, 6, 8))):
        plan = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), precision="double")
        plan.initFFT(dfft.GlobalSize(*shp), dfft.Pencil_Partition(1, 1), False, c2c=True)
        sizes[name] = (plan.getWorkSizeDevice(), plan.getDomainSize())
    assert sizes["short"][0] <= sizes["short"][1] + 256
    assert sizes["long"][0] >= 2 * sizes["long"][1]      # one slice + tiles x 8 lines x 10000 points of scratch
    plan = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), precision="double")
    plan.initFFT(dfft.GlobalSize(*shape), dfft.Pencil_Partition(1, 1), False, c2c=True)
    work = torch.zeros(plan.getWorkSizeDevice(), dtype=torch.uint8, device="cuda")
    plan.setWorkArea(work)
    g = orc.fill_block(shape, (0, 0, 0), shape, 2, seed=3)
    d_in = torch.from_numpy(g).cuda()
    d_out = torch.zeros_like(d_in)
    torch.cuda.synchronize()
    plan.execC2C(d_out, d_in, dfft.FORWARD)
    torch.cuda.synchronize()
    want = orc.fft3d_c2c(g, -1)
    assert rel(d_out.cpu().numpy().reshape(shape), want) < 4e-11
    check_forward(d_out.cpu().numpy().reshape(shape), want, "double", g.size, zero_mean=False)


# ------------------------------------------------------------------------------------------
# Lines up to 2^24 points: the documented range (README, DESIGN 3.2, include/dfft_c.h) beyond LONG and LONG_BLUESTEIN above, whose
# largest plain level is 512 points.  One length per form of a level that those never reach -- plain levels of 1024 and 2048 points,
# the sub-tile workgroups of a plain 4096- or 8192-point level (Cfg::kSUB > 1 with PassArgs::plain), long Bluestein over M >= 2^20
# padded points -- each at the smallest length that has it, and the top of the range.  Every case first asserts its plan, so that a
# change of the cost model fails the test and does not move it to another form.
#
# fft1d_case's scheme (both directions, the reference's distribution and the same centred, the per-entry bound with factor 1, the old
# bound beside it, the input bit-identical afterwards) with two differences the sizes ask for: the reference is numpy's transform in
# long double (np.clongdouble: complex256 out), rounded once to complex128 -- 1e-16 of an entry, against bounds of 1e-12 -- and it is computed
# once per input: the unnormalised inverse of x is the forward transform read backwards, ifft(x)[k] * N = fft(x)[(N - k) % N].
# profiles/long_lines_parity_table.txt: the measured values and wall times (DFFT_PARITY_TABLE); profiles/long_lines_mutation.txt: the
# fp64 cases on a library whose tables are rounded through fp32.
# ------------------------------------------------------------------------------------------
TILE_LINES = {"double": 8, "float": 16}      # getTileLines() of any plan (csrc/dfft_internal.hpp)


def two(n1, m1, b1, n2, m2, b2):
    return ("two_level", 0, [(n1, m1, bool(b1)), (n2, m2, bool(b2))])


def longb(n1, n2):
    return ("long_bluestein", n1 * n2, [(n1, n1, False), (n2, n2, False)])


# (length, plan in both precisions); a level (F, M, bluestein): plain when M == F
LONG_FORMS = [
    pytest.param(132096, two(129, 512, 1, 1024, 1024, 0), id="132096-bluestein129xplain1024"),
    pytest.param(524288, two(512, 512, 0, 1024, 1024, 0), id="524288-plain512xplain1024"),
    pytest.param(526336, two(257, 1024, 1, 2048, 2048, 0), id="526336-bluestein257xplain2048"),
    pytest.param(1048576, two(1024, 1024, 0, 1024, 1024, 0), id="1048576-plain1024xplain1024"),
    pytest.param(4194304, two(2048, 2048, 0, 2048, 2048, 0), id="4194304-plain2048xplain2048"),
    pytest.param(2101248, two(513, 2048, 1, 4096, 4096, 0), id="2101248-bluestein513xsubtile4096"),
    pytest.param(4202496, two(513, 2048, 1, 8192, 8192, 0), id="4202496-bluestein513xsubtile8192"),
    pytest.param(8388608, two(2048, 2048, 0, 4096, 4096, 0), id="8388608-plain2048xsubtile4096"),
    pytest.param(262147, longb(1024, 1024), id="262147-long-bluestein-M1048576"),
    pytest.param(1000003, longb(1024, 2048), id="1000003-long-bluestein-M2097152"),
    # 2^21 + 1 = 3 x 699051 does not split: the smallest length above 2^21 that axis_plan_info reports as long Bluestein.  30 s a case,
    # 22 s of it the host's long-double transform of the 2^23 chirp entries at the first call (axis_upload), 7 s the reference: slow
    pytest.param(2097153, longb(2048, 4096), id="2097153-long-bluestein-M8388608", marks=pytest.mark.slow),
]
# the top of the range: the longest line, the longest with one / with two Bluestein levels of 4093 points (the largest prime whose
# padded length fits one launch), the longest long-Bluestein line.  Centred input only.  2^24 takes 7 s a case (4 s of it the host's
# table of 2^24 long-double twiddles) and stays in the default run; the two lengths with a factor of 4093 take 7 ... 12 s with their
# composed reference and 8388593 takes 49 s (47 s of it the host's long-double transform of 2^24 chirp entries): slow
# (profiles/long_lines_parity_table.txt)
LONG_TOP = [
    pytest.param(1 << 24, two(2048, 2048, 0, 8192, 8192, 0), id="16777216-plain2048xsubtile8192"),
    pytest.param(16764928, two(4093, 8192, 1, 4096, 4096, 0), id="16764928-bluestein4093xsubtile4096", marks=pytest.mark.slow),
    pytest.param(16752649, two(4093, 8192, 1, 4093, 8192, 1), id="16752649-bluestein4093xbluestein4093", marks=pytest.mark.slow),
    pytest.param(8388593, longb(2048, 8192), id="8388593-long-bluestein-M16777216", marks=pytest.mark.slow),
]


def table_note(text):
    path = os.environ.get("DFFT_PARITY_TABLE")
    if path:
        with open(path, "a") as f:
            f.write(text + "\n")


def largest_prime_factor(n):
    p, f = 1, 2
    while f * f <= n:
        while n % f == 0:
            p, n = f, n // f
        f += 1
    return max(p, n) if n > 1 else p


@functools.lru_cache(maxsize=1)
def composed_twiddles(n1, n2):
    """exp(-2 pi i k1 m / (n1 n2)) for k1 < n1, m < n2, evaluated in long double"""
    ang = -2 * np.longdouble("3.141592653589793238462643383279502884") / np.longdouble(n1 * n2) \
        * (np.arange(n1, dtype=np.longdouble)[:, None] * np.arange(n2, dtype=np.longdouble)[None, :])
    return (np.cos(ang) + 1j * np.sin(ang)).astype(np.complex128)


def composed_fft(x, n1, n2):
    """the transform of lines of n1 * n2 points composed from pocketfft's transforms of n1 and of n2 points (a prime factor of 4093
    points goes through its Bluestein path there) and long-double twiddles between them: pocketfft takes 16764928 = 4093 x 4096 and
    16752649 = 4093^2 points as a whole with an O(4093 N) pass, 38 s and 77 s a line; per entry the two differ by 8e-15 at both"""
    b = x.shape[0]
    a = np.fft.fft(x.reshape(b, n1, n2), axis=1)      # [k1][m], point n = n1-index * n2 + m
    a *= composed_twiddles(n1, n2)[None]
    a = np.fft.fft(a, axis=2)                         # [k1][k2] is output k1 + n1 * k2
    return np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(b, n1 * n2)


def long_line_case(N, prec, plan, batch, inputs=(False, True), long_double=True, label="long line"):
    """inputs: centred or not, in turn.  long_double=False: complex128 pocketfft as the reference (the top of the range: its own
    per-entry error on the centred input is 1.5e-15 at 2^24 and 2.7e-15 at 8388593 against the long-double transform, a
    thousandth of the fp64 bound), composed from its transforms of the two factors where it is slow as a whole (composed_fft).  The oracle's own transform is cross-checked against the reference where it is fast: up to
    2^20 points without a large prime factor (it takes a prime length as an O(N^2) sum)."""
    info = dfft.axis_plan_info(N, prec)
    assert info is not None and (info["kind"], info["M"], info["levels"]) == plan, (N, prec, info)
    if plan[0] == "long_bluestein":
        assert plan[1] == 1 << (2 * N - 2).bit_length() and plan[1] >= 2 * N - 1
    assert batch % TILE_LINES[prec] != 0, "a ragged number of lines, not a multiple of the tile"
    t_case = time.time()
    rng = np.random.default_rng(N)
    x0 = rng.uniform(0, 255, (batch, N)) + 1j * rng.uniform(0, 255, (batch, N))
    grow = max(1.0, np.log2(N) / 12.0)
    with_oracle = N <= 1 << 20 and largest_prime_factor(N) <= 257
    t_ref = t_first = t_gpu = 0.0
    d_in = d_out = None
    try:
        for centred in inputs:
            x = (x0 - CENTER * (1 + 1j) if centred else x0).astype(NPDT[prec])
            t0 = time.time()
            if long_double:
                forward = np.fft.fft(x.astype(np.clongdouble), axis=-1)
                assert forward.dtype == np.clongdouble
                forward = forward.astype(np.complex128)
            elif N > 1 << 20 and 2048 < largest_prime_factor(N) < N:
                forward = composed_fft(x.astype(np.complex128), plan[2][0][0], plan[2][1][0])
            else:
                forward = np.fft.fft(x.astype(np.complex128), axis=-1)
            t_ref += time.time() - t0
            if with_oracle:
                assert rel(orc.fft1d(x.astype(np.complex128), dfft.FORWARD), forward) < 1e-12
            d_in = torch.from_numpy(x).cuda()
            d_out = torch.zeros_like(d_in)
            for direction in (dfft.FORWARD, dfft.INVERSE):
                torch.cuda.synchronize()
                t0 = time.time()
                dfft.fft1d_batched(d_out, d_in, N, batch, direction, prec)
                torch.cuda.synchronize()
                if t_first == 0.0:
                    t_first = time.time() - t0      # with the host's long-double table build (axis_upload)
                else:
                    t_gpu += time.time() - t0
                got = d_out.cpu().numpy()
                want = forward if direction == dfft.FORWARD else np.roll(forward[:, ::-1], 1, axis=-1)
                check_forward(got, want, prec, N, zero_mean=centred, label=f"{label} fft1d N={N} x{batch} dir={direction} centred={centred}")
                assert rel(got, want) < (2e-11 if prec == "double" else 2e-4) * grow
                del got, want
            assert np.array_equal(d_in.cpu().numpy(), x), "the pass must not modify its input"
    finally:
        del d_in, d_out
        torch.cuda.empty_cache()
    table_note(f"{label} fft1d N={N} x{batch} {prec}: wall {time.time() - t_case:.1f} s (reference {t_ref:.1f} s, first call with the table "
               f"build {t_first:.2f} s, the other {2 * len(inputs) - 1} calls {t_gpu:.3f} s)")


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("N,plan", LONG_FORMS)
def test_fft1d_long_line_forms_vs_long_double(N, plan, prec):
    """every form of a level between the suite's 131072 points and the top of the range, 3 lines (2 above 5e6 points)"""
    long_line_case(N, prec, plan, 3 if N < 5000000 else 2)


@pytest.mark.parametrize("prec", ["double", "float"])
def test_fft1d_long_line_on_more_than_one_tile(prec):
    """TL + 1 lines of 524288 points: a second tile of lines (their own N points each in the scratch); centred input"""
    long_line_case(524288, prec, two(512, 512, 0, 1024, 1024, 0), TILE_LINES[prec] + 1, inputs=(True,), label="long line, two tiles")


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("N,plan", LONG_TOP)
def test_fft1d_top_of_the_range_vs_pocketfft(N, plan, prec):
    """2 lines each of the longest lengths with a plan: tables of 2^24 entries, 32-bit point indices at their limit"""
    long_line_case(N, prec, plan, 2, inputs=(True,), long_double=False, label="top of the range")


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("N", [(1 << 24) + 1, 8388609])
def test_fft1d_beyond_the_range_is_refused(N, prec):
    """2^24 + 1 is beyond the kernel's point indices, 8388609 = 3 x 2796203 neither splits nor pads within 2^24: ERR_UNSUPPORTED
    before anything is launched (the buffers are whole lines all the same)"""
    assert dfft.axis_plan_info(N, prec) is None
    d_in = torch.zeros(N, dtype=torch.complex128 if prec == "double" else torch.complex64, device="cuda")
    d_out = torch.full_like(d_in, 7.0)
    try:
        for direction in (dfft.FORWARD, dfft.INVERSE):
            with pytest.raises(dfft.DfftError, match="error 4.*unsupported line length"):
                dfft.fft1d_batched(d_out, d_in, N, 1, direction, prec)
        torch.cuda.synchronize()
        assert bool((d_out == 7.0).all()) and not bool(d_in.any()), "a refused call must not touch its buffers"
    finally:
        del d_in, d_out
        torch.cuda.empty_cache()
