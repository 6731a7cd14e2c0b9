"""Parity tests proper: HIP path (through the C ABI) vs the CPU oracle on the same seeded
inputs.  Tolerances: fp64 forward rel L-inf (scaled by max|X|) <= 1e-11, round
trip <= 1e-10; fp32 forward <= 1e-4 (vs the fp64 oracle), round trip <= 5e-5."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import distributedfft_amd as dfft  # noqa: E402
from oracle import oracle as orc  # noqa: E402

from parity_metric import CENTER, check_forward, check_forward_blocks, rms  # noqa: E402

TOL_FWD = {"double": 1e-11, "float": 1e-4}
TOL_RT = {"double": 1e-10, "float": 5e-5}
CDT = {"double": torch.complex128, "float": torch.complex64}
NPDT = {"double": np.complex128, "float": np.complex64}
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("N", [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192])
def test_fft1d_batched_vs_oracle(N, prec):
    """kernel-level: batched axis pass on natural lines, ragged batch (not a multiple of the
    lines-per-workgroup), both directions"""
    batch = 37 if N >= 256 else 531
    rng = np.random.default_rng(N)
    x0 = rng.uniform(0, 255, (batch, N)) + 1j * rng.uniform(0, 255, (batch, N))
    for x in (x0, x0 - CENTER * (1 + 1j)):        # the reference's distribution, and the same centred (zero mean)
        d_in = torch.from_numpy(x.astype(NPDT[prec])).cuda()
        d_out = torch.zeros_like(d_in)
        for direction in (dfft.FORWARD, dfft.INVERSE):
            torch.cuda.synchronize()
            dfft.fft1d_batched(d_out, d_in, N, batch, direction, prec)
            torch.cuda.synchronize()
            want = orc.fft1d(x.astype(NPDT[prec]), direction)
            assert rel(d_out.cpu().numpy(), want) < TOL_FWD[prec]
            check_forward(d_out.cpu().numpy(), want, prec, N, zero_mean=x is not x0,
                          label=f"fft1d N={N} dir={direction} mean={x.real.mean():.0f}" if N in (8, 1024, 8192) else None)


def run_single(shape, prec, seed=5, center=False, arena=None):
    """arena (tests/guarded.py): every buffer and a caller-owned work area come from it, refilled before either exec, and the guards and
    the input are checked after either exec; a second call with the same arena runs the plan and the buffers of the first"""
    g = orc.fill_block(shape, (0, 0, 0), shape, 2, seed=seed)
    if center:
        g = g - CENTER * (1 + 1j)
    g = g.astype(NPDT[prec])
    esz = 16 if prec == "double" else 8

    def setup():
        plan = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), precision=prec)
        plan.initFFT(dfft.GlobalSize(*shape), dfft.Pencil_Partition(1, 1), arena is None, c2c=True)
        if arena is not None:
            return (plan,) + arena.plan_buffers(plan, g, CDT[prec])
        return plan, torch.from_numpy(g).cuda(), torch.zeros(plan.getDomainSize() // esz, dtype=CDT[prec], device="cuda"), None

    plan, d_in, d_out, d_back = setup() if arena is None else arena.once("run_single", setup)
    if arena is not None:
        arena.refill()
    torch.cuda.synchronize()
    plan.execC2C(d_out, d_in, dfft.FORWARD)
    got = d_out[:g.size].cpu().numpy().reshape(shape)
    assert np.array_equal(d_in.cpu().numpy(), g), "forward must not modify its input"
    if arena is None:
        d_back = torch.zeros_like(d_in)
    else:
        arena.check_guards(f"run_single {shape} {prec} forward")
        arena.check_inputs(f"run_single {shape} {prec} forward")
        arena.refill(keep=[d_out])
    torch.cuda.synchronize()      # the fill runs on torch's stream, the plan on its own
    plan.execC2C(d_back, d_out, dfft.INVERSE)
    if arena is not None:
        arena.check_guards(f"run_single {shape} {prec} inverse")
    return g, got, d_back.cpu().numpy()


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("shape", [(8, 8, 8), (2, 4, 8), (16, 16, 16), (32, 16, 64), (64, 64, 64),
                                   (16, 128, 32), (128, 128, 128), (256, 8, 512), (4, 1024, 16), (2048, 4, 4),
                                   (4096, 4, 6), (3, 8192, 20), (5, 4, 4096), (16, 20, 8192)])
def test_single_rank_3d_vs_oracle(shape, prec):
    """fft3d branch (one rank): three local axis passes == oracle 3-D transform"""
    for center in (False, True):
        g, got, back = run_single(shape, prec, center=center)
        want = orc.fft3d_c2c(g.astype(np.complex128), -1)
        assert rel(got, want) < TOL_FWD[prec]
        check_forward(got, want, prec, g.size, zero_mean=center, label=f"single rank {shape} centred={center}" if shape in ((128, 128, 128), (16, 20, 8192)) else None)
        assert rel(back / g.size, g) < TOL_RT[prec]


def test_golden_fixture_single_rank():
    d = np.load(os.path.join(GOLD, "fft3d_small.npz"))
    shape = (8, 8, 8)
    g, got, _ = run_single(shape, "double", seed=int(d["seed"]))
    assert rel(got, d["c2c_8x8x8"]) < 1e-11


def run_distributed(shape, P1, P2, prec, seed=7, chunks=None, options=None, comm_options=None, center=False, arena=None):
    """P1*P2 virtual ranks on one GPU (one host thread per rank, like MPI ranks sharing a
    device: tests/src/pencil/random_dist_3D.cu:175-177).  arena: as in run_single."""
    P = P1 * P2
    esz = 16 if prec == "double" else 8

    def setup():
        world = dfft.Comm.local(P)
        for k, v in (comm_options or {}).items():
            world.setOption(k, v)
        plans, ins, outs, backs = [], [], [], []
        for r in range(P):
            pl = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), world, precision=prec, rank=r)
            if chunks is not None:
                pl.setPipelineChunks(chunks)
            for k, v in (options or {}).items():
                pl.setOption(k, v)
            pl.initFFT(dfft.GlobalSize(*shape), dfft.Pencil_Partition(P1, P2), arena is None, c2c=True)
            size, start = pl.getInSize(), pl.getInStart()
            blk = orc.fill_block(shape, start, size, 2, seed=seed)
            if center:
                blk = blk - CENTER * (1 + 1j)
            blk = blk.astype(NPDT[prec])
            plans.append(pl)
            if arena is not None:
                for lst, t in zip((ins, outs, backs), arena.plan_buffers(pl, blk, CDT[prec], r)):
                    lst.append(t)
                continue
            ins.append(torch.from_numpy(blk).cuda())
            outs.append(torch.zeros(pl.getDomainSize() // esz, dtype=CDT[prec], device="cuda"))
            backs.append(torch.zeros_like(ins[-1]))
        return plans, ins, outs, backs

    plans, ins, outs, backs = setup() if arena is None else arena.once("run_distributed", setup)
    what = f"run_distributed {shape} {P1}x{P2} {prec} {options or ''}"
    if arena is not None:
        arena.refill()
    torch.cuda.synchronize()
    with ThreadPoolExecutor(P) as ex:
        list(ex.map(lambda r: plans[r].execC2C(outs[r], ins[r], dfft.FORWARD), range(P)))
    if arena is not None:
        arena.check_guards(what + " forward")
        arena.check_inputs(what + " forward")
    spec = []
    for r in range(P):      # (Nx, yo, zs) whatever the plan's spectral layout (option spectral_layout)
        spec.append(plans[r].spectrumView(outs[r]).contiguous().cpu().numpy())
    if arena is not None:
        arena.refill(keep=outs)
    with ThreadPoolExecutor(P) as ex:
        list(ex.map(lambda r: plans[r].execC2C(backs[r], outs[r], dfft.INVERSE), range(P)))
    torch.cuda.synchronize()
    if arena is not None:
        arena.check_guards(what + " inverse")
    return plans, [t.cpu().numpy() for t in ins], spec, [t.cpu().numpy() for t in backs]


DIST = [((4096, 16, 8), 2, 2), ((8, 8192, 48), 3, 2), ((16, 16, 16), 2, 2), ((32, 32, 32), 2, 4), ((64, 32, 16), 4, 2), ((16, 16, 16), 3, 2),
        ((32, 16, 64), 2, 1), ((32, 64, 32), 8, 1), ((16, 32, 16), 1, 4), ((64, 64, 64), 3, 5),
        ((128, 64, 32), 2, 4)]


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("shape,P1,P2", DIST)
def test_distributed_vs_oracle(shape, P1, P2, prec):
    """reference testcase 1 (distributed == single device) and testcase 3 (round trip), with
    even and uneven partitions, pencil and slab (P2 == 1)."""
    opl = orc.PencilPlan(*shape, P1, P2, True)
    n3 = float(np.prod(shape))
    for center in (False, True):
        plans, ins, spec, backs = run_distributed(shape, P1, P2, prec, center=center)
        g = orc.fill_block(shape, (0, 0, 0), shape, 2, seed=7) - (CENTER * (1 + 1j) if center else 0)
        want = orc.fft3d_c2c(g.astype(NPDT[prec]).astype(np.complex128), -1)
        want_rms = rms(want)
        for r, pl in enumerate(plans):
            s, o = pl.getOutSize(), pl.getOutStart()
            assert (s, o) == opl.out_block(r)
            ref = want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]]
            assert rel(spec[r], ref) < TOL_FWD[prec] * (np.max(np.abs(want)) / max(np.max(np.abs(ref)), 1e-300))
            check_forward(spec[r], ref, prec, g.size, want_rms=want_rms, zero_mean=center,
                          label=f"distributed {shape} {P1}x{P2} rank {r} centred={center}" if r == 0 and shape in ((128, 64, 32), (64, 64, 64)) else None)
            assert rel(backs[r] / n3, ins[r]) < TOL_RT[prec]
            for which in (1, 2):   # byte tables == the reference's formulas (via the oracle restatement)
                esz = 16 if prec == "double" else 8
                assert pl.getExchangeTables(which) == [[v * esz for v in t] for t in opl.exchange_tables(r, which)]


# ------------------------------------------------------------------------------------------
# R2C / C2R: the reference's actual API (execR2C / execC2R, Nz_out = Nz/2+1)
# ------------------------------------------------------------------------------------------
RDT = {"double": torch.float64, "float": torch.float32}
NPR = {"double": np.float64, "float": np.float32}


def run_distributed_real(shape, P1, P2, prec, field=None, seed=13, modify=None, options=None, comm_options=None, chunks=None, arena=None):
    """arena: as in run_single"""
    P = P1 * P2
    esz = 16 if prec == "double" else 8

    def setup():
        world = dfft.Comm.local(P) if P > 1 else None
        for k, v in (comm_options or {}).items():
            world.setOption(k, v)
        plans, ins, outs, backs = [], [], [], []
        for r in range(P):
            pl = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), world, precision=prec, rank=r)
            if chunks is not None:
                pl.setPipelineChunks(chunks)
            for k, v in (options or {}).items():
                pl.setOption(k, v)
            pl.initFFT(dfft.GlobalSize(*shape), dfft.Pencil_Partition(P1, P2), arena is None)      # R2C plan
            size, start = pl.getInSize(), pl.getInStart()
            if field is None:
                blk = orc.fill_block(shape, start, size, 1, seed=seed)
            else:
                blk = np.ascontiguousarray(field[start[0]:start[0] + size[0], start[1]:start[1] + size[1], :])
            plans.append(pl)
            if arena is not None:
                for lst, t in zip((ins, outs, backs), arena.plan_buffers(pl, blk.astype(NPR[prec]), CDT[prec], r)):
                    lst.append(t)
                continue
            ins.append(torch.from_numpy(blk.astype(NPR[prec])).cuda())
            outs.append(torch.zeros(pl.getDomainSize() // esz, dtype=CDT[prec], device="cuda"))
            backs.append(torch.zeros_like(ins[-1]))
        return plans, ins, outs, backs

    plans, ins, outs, backs = setup() if arena is None else arena.once("run_distributed_real", setup)
    what = f"run_distributed_real {shape} {P1}x{P2} {prec} {options or ''}"
    if arena is not None:
        arena.refill()
    torch.cuda.synchronize()
    with ThreadPoolExecutor(P) as ex:
        list(ex.map(lambda r: plans[r].execR2C(outs[r], ins[r]), range(P)))
    if arena is not None:
        arena.check_guards(what + " forward")
        arena.check_inputs(what + " forward")
    spec = []
    for r in range(P):      # (Nx, yo, zs) whatever the plan's spectral layout (option spectral_layout)
        spec.append(plans[r].spectrumView(outs[r]).contiguous().cpu().numpy())
    if modify is not None:
        for r in range(P):
            s, o = plans[r].getOutSize(), plans[r].getOutStart()
            blk = np.ascontiguousarray(spec[r].astype(np.complex128))
            modify(blk, s, o)
            plans[r].spectrumView(outs[r]).copy_(torch.from_numpy(blk.astype(NPDT[prec])).cuda())
    if arena is not None:
        arena.refill(keep=outs)
    torch.cuda.synchronize()
    with ThreadPoolExecutor(P) as ex:
        list(ex.map(lambda r: plans[r].execC2R(backs[r], outs[r]), range(P)))
    torch.cuda.synchronize()
    if arena is not None:
        arena.check_guards(what + " inverse")
    return plans, [t.cpu().numpy() for t in ins], spec, [t.cpu().numpy() for t in backs]


REAL = [((8, 8, 8), 1, 1), ((16, 16, 16), 1, 1), ((32, 16, 64), 1, 1), ((128, 128, 128), 1, 1),
        ((4, 4, 2048), 1, 1), ((4, 6, 4096), 1, 1), ((4, 512, 4096), 2, 2), ((16, 8, 2048), 2, 2), ((8, 8, 1024), 1, 1), ((8, 16, 1024), 2, 2), ((16, 8, 512), 1, 2), ((16, 16, 16), 2, 2), ((32, 32, 32), 2, 4), ((64, 32, 16), 4, 2),
        ((16, 16, 16), 3, 2), ((32, 16, 64), 2, 1), ((64, 64, 64), 3, 5), ((128, 64, 32), 2, 4)]


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("shape,P1,P2", REAL)
def test_r2c_c2r_vs_oracle(shape, P1, P2, prec):
    """execR2C output == oracle rfftn block (Hermitian half, uneven Nz/2+1 split) and
    C2R(R2C(x)) == Nx*Ny*Nz*x (reference testcase 3, random_dist_3D.cu:641-666)"""
    n3 = float(np.prod(shape))
    for center in (False, True):
        g0 = orc.fill_block(shape, (0, 0, 0), shape, 1, seed=13) - (CENTER if center else 0.0)
        plans, ins, spec, backs = run_distributed_real(shape, P1, P2, prec, field=g0 if center else None)
        g = g0.astype(NPR[prec]).astype(np.float64)
        want = orc.fft3d_r2c(g)
        scale = np.max(np.abs(want))
        want_rms = rms(want)
        for r, pl in enumerate(plans):
            s, o = pl.getOutSize(), pl.getOutStart()
            ref = want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]]
            assert np.max(np.abs(spec[r] - ref)) / scale < TOL_FWD[prec]
            check_forward(spec[r], ref, prec, g.size, want_rms=want_rms, zero_mean=center,
                          label=f"R2C {shape} {P1}x{P2} rank {r} centred={center}" if r == 0 and shape in ((128, 64, 32), (4, 512, 4096)) else None)
            assert rel(backs[r] / n3, ins[r]) < TOL_RT[prec]


@pytest.mark.parametrize("shape,P1,P2", [((32, 32, 32), 1, 1), ((32, 32, 32), 2, 4), ((64, 32, 16), 2, 2)])
def test_testcase4_laplacian_known_answer(shape, P1, P2):
    """reference testcase 4 (random_dist_3D.cu:685-811): u = sin sin sin, multiply the
    distributed spectrum by -(k1^2+k2^2+k3^2)/sqrt(N^3), inverse, compare with -3 sqrt(N^3) u"""
    Nx, Ny, Nz = shape
    x, y, z = np.meshgrid(np.arange(Nx), np.arange(Ny), np.arange(Nz), indexing="ij")
    u = np.sin(2 * np.pi * x / Nx) * np.sin(2 * np.pi * y / Ny) * np.sin(2 * np.pi * z / Nz)

    def modify(blk, s, o):
        orc.derivative_coefficients(blk, shape, o[2], o[1], half=True)

    plans, ins, spec, backs = run_distributed_real(shape, P1, P2, "double", field=u, modify=modify)
    n3 = float(Nx * Ny * Nz)
    for r in range(len(plans)):
        want = orc.testcase4_expected(shape, ins[r])      # the reference's multiplier divides by sqrtf(N^3): oracle/oracle.py
        assert np.max(np.abs(backs[r] - want)) < 1e-9 * np.sqrt(n3)


@pytest.mark.parametrize("n,P1,P2", [(128, 2, 2), (128, 4, 1), (256, 2, 2), (512, 2, 2)])
def test_testcase4_reproduces_the_references_own_shipped_results(n, P1, P2):
    """THE HIP PATH AGAINST NUMBERS THE REFERENCE ITSELF PRODUCED: testcase 4 (deterministic input, closed-form answer) through
    execR2C -> the reference's derivativeCoefficients arithmetic -> execC2R on 4 virtual ranks, compared with the `Result (avg)` /
    `Result (max)` lines of the run logs the reference ships (tests/golden/ref_testcase4_results.json; see
    tests/test_oracle.py::test_testcase4_reproduces_the_references_own_shipped_results for what the digits are made of)."""
    import json
    ref_all = json.load(open(os.path.join(GOLD, "ref_testcase4_results.json")))
    mode = "slab" if P2 == 1 else "pencil"
    ref = ref_all[f"{mode} {n}x{n}x{n} opt=1 seq=ZY_Then_X ranks=4"] + ref_all[f"{mode} {n}x{n}x{n} opt=0 seq=ZY_Then_X ranks=4"]
    shape = (n, n, n)
    ax = np.sin(2 * np.pi * np.arange(n) / n)
    u = ax[:, None, None] * ax[None, :, None] * ax[None, None, :]

    def modify(blk, s, o):
        orc.derivative_coefficients(blk, shape, o[2], o[1], half=True)

    plans, ins, spec, backs = run_distributed_real(shape, P1, P2, "double", field=u, modify=modify)
    n3 = float(n) ** 3
    diffs = [np.abs(backs[r] - (-3.0 * np.sqrt(n3)) * ins[r]) for r in range(P1 * P2)]
    avg, mx = sum(float(d.sum()) for d in diffs) / n3, max(float(d.max()) for d in diffs)
    lo_a, hi_a = min(e["avg"] for e in ref), max(e["avg"] for e in ref)
    lo_m, hi_m = min(e["max"] for e in ref), max(e["max"] for e in ref)
    if n in (128, 512):      # the single-precision root dominates: six printed digits of the average, the maximum inside the logs' scatter
        assert format(avg, ".6g") in {format(e["avg"], ".6g") for e in ref}, (avg, ref)      # as the reference printed it: six significant digits
        assert lo_m * (1 - 5e-4) <= mx <= hi_m * (1 + 5e-4), (mx, lo_m, hi_m)
    else:                    # 256^3: the float root is exact, what is left is the input's rounding amplified by k^2 -- the same floor as cuFFT's
        assert 0.7 * lo_a <= avg <= 1.3 * hi_a and 0.7 * lo_m <= mx <= 1.3 * hi_m, (avg, mx, ref)


def test_error_behaviour():
    """bad arguments raise instead of exit(EXIT_FAILURE) (mpicufft_pencil_opt1.cpp:22-33, 61-65)"""
    pl = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations())
    with pytest.raises(dfft.DfftError, match="Invalid Input Partition"):
        pl.initFFT(dfft.GlobalSize(16, 16, 16), dfft.Pencil_Partition(2, 2))
    with pytest.raises(dfft.DfftError, match="not initialised"):
        pl.execR2C(1, 1)
    pl.initFFT(dfft.GlobalSize(16, 16, 16), dfft.Pencil_Partition(1, 1))
    with pytest.raises(dfft.DfftError, match="C2C|R2C"):
        pl.execC2C(1, 1)
    with pytest.raises(dfft.DfftError, match="unsupported"):
        pl.initFFT(dfft.GlobalSize((1 << 24) + 1, 16, 16), dfft.Pencil_Partition(1, 1), False)      # more than 2^24 points on a line


@pytest.mark.parametrize("chunks", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("shape,P1,P2", [((32, 32, 32), 2, 4), ((16, 16, 16), 3, 2), ((64, 32, 16), 8, 1), ((16, 32, 16), 1, 4)])
def test_pipelined_exchange_chunks(shape, P1, P2, chunks):
    """the chunked two-stream pipeline (compute of chunk c+1 overlapped with the exchange of chunk c)
    gives the same result for every depth, including depths that do not divide the extents"""
    plans, ins, spec, backs = run_distributed(shape, P1, P2, "double", chunks=chunks)
    assert 1 <= plans[0].getPipelineChunks() <= chunks
    want = orc.fft3d_c2c(orc.fill_block(shape, (0, 0, 0), shape, 2, seed=7), -1)
    n3 = float(np.prod(shape))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        ref = want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]]
        assert np.max(np.abs(spec[r] - ref)) / np.max(np.abs(want)) < 1e-11
        assert rel(backs[r] / n3, ins[r]) < 1e-10
    check_forward_blocks(plans, spec, want, "double", want.size, zero_mean=False)


# ------------------------------------------------------------------------------------------
# partial transforms: MPIcuFFT_Pencil::execR2C/execC2R(out, in, d), d = 1, 2
# (reference tests random_dist_1D.cu:180-451, random_dist_2D.cu:181-455)
# ------------------------------------------------------------------------------------------
def run_partial(shape, P1, P2, d, c2c, two_level=0, prec="double", center=False, seed=31, arena=None):
    """execC2C / execR2C(out, in, d) and back on P1*P2 virtual ranks: (plans, global input, per-rank (got, want) blocks of the partial
    spectrum, the whole partial spectrum, inputs, round trips); the reference is numpy's transform along z (d = 1), then y (d = 2).
    arena: as in run_single (the forward partial transforms only read `in`: include/dfft_c.h)"""
    P = P1 * P2
    Nx, Ny, Nz = shape
    Nzc = Nz if c2c else Nz // 2 + 1
    esz = 16 if prec == "double" else 8
    g = orc.fill_block(shape, (0, 0, 0), shape, 2 if c2c else 1, seed=seed)
    if center:
        g = g - (CENTER * (1 + 1j) if c2c else CENTER)
    g = g.astype(NPDT[prec] if c2c else NPR[prec])
    g64 = g.astype(np.complex128 if c2c else np.float64)
    # d = 1: FFT along z only; d = 2: along z then y (numpy as the independent reference)
    ref = np.fft.fft(g64, axis=2) if c2c else np.fft.rfft(g64, axis=2)
    if d == 2:
        ref = np.fft.fft(ref, axis=1)

    def setup():
        world = dfft.Comm.local(P) if P > 1 else None
        plans, ins, outs, backs = [], [], [], []
        for r in range(P):
            pl = dfft.MPIcuFFT_Pencil(dfft.Configurations(), world, precision=prec, rank=r)
            pl.setOption("two_level", two_level)
            pl.initFFT(dfft.GlobalSize(*shape), dfft.Pencil_Partition(P1, P2), arena is None, c2c=c2c)
            s, o = pl.getInSize(), pl.getInStart()
            blk = np.ascontiguousarray(g[o[0]:o[0] + s[0], o[1]:o[1] + s[1], :])
            plans.append(pl)
            if arena is not None:
                for lst, t in zip((ins, outs, backs), arena.plan_buffers(pl, blk, CDT[prec], r)):
                    lst.append(t)
                continue
            ins.append(torch.from_numpy(blk).cuda())
            outs.append(torch.zeros(pl.getDomainSize() // esz, dtype=CDT[prec], device="cuda"))
            backs.append(torch.zeros_like(ins[-1]))
        return plans, ins, outs, backs

    plans, ins, outs, backs = setup() if arena is None else arena.once("run_partial", setup)
    what = f"run_partial {shape} {P1}x{P2} d={d} {'C2C' if c2c else 'R2C'} {prec}"
    if arena is not None:
        arena.refill()
    torch.cuda.synchronize()

    def fwd(r):
        if c2c:
            plans[r].execC2C(outs[r], ins[r], dfft.FORWARD, d=d)
        else:
            plans[r].execR2C(outs[r], ins[r], d)

    def inv(r):
        if c2c:
            plans[r].execC2C(backs[r], outs[r], dfft.INVERSE, d=d)
        else:
            plans[r].execC2R(backs[r], outs[r], d)

    with ThreadPoolExecutor(P) as ex:
        list(ex.map(fwd, range(P)))
    torch.cuda.synchronize()
    if arena is not None:
        arena.check_guards(what + " forward")
        arena.check_inputs(what + " forward")
    blocks = []
    for r, pl in enumerate(plans):
        isz, ist = pl.getInSize(), pl.getInStart()
        osz, ost = pl.getOutSize(), pl.getOutStart()
        if d == 1:      # [xs][ys][Nzc]
            shp = (isz[0], isz[1], Nzc)
            want = ref[ist[0]:ist[0] + isz[0], ist[1]:ist[1] + isz[1], :]
        else:           # [xs][Ny][zs]
            shp = (isz[0], Ny, osz[2])
            want = ref[ist[0]:ist[0] + isz[0], :, ost[2]:ost[2] + osz[2]]
        blocks.append((outs[r][:int(np.prod(shp))].cpu().numpy().reshape(shp), want))
    if arena is not None:
        arena.refill(keep=outs)
    with ThreadPoolExecutor(P) as ex:
        list(ex.map(inv, range(P)))
    torch.cuda.synchronize()
    if arena is not None:
        arena.check_guards(what + " inverse")
    return plans, blocks, ref, [t.cpu().numpy() for t in ins], [t.cpu().numpy() for t in backs]


@pytest.mark.parametrize("c2c", [False, True])
@pytest.mark.parametrize("shape,P1,P2", [((16, 16, 16), 1, 1), ((32, 32, 32), 2, 4), ((16, 32, 64), 3, 2), ((64, 32, 16), 4, 1)])
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("two_level", [0, 1])
def test_partial_dimension_transforms(shape, P1, P2, d, c2c, two_level):
    """execR2C / execC2R(out, in, d) (src/pencil/mpicufft_pencil.cpp:1644-1839); two_level = 1: the same on two-level lines"""
    Nx, Ny, Nz = shape
    plans, blocks, ref, ins, backs = run_partial(shape, P1, P2, d, c2c, two_level)
    scale = np.max(np.abs(ref))
    points = Nz if d == 1 else Nz * Ny        # the transform applied: lines along z, or (y, z) planes
    ref_rms = rms(ref)
    for got, want in blocks:
        assert np.max(np.abs(got - want)) / scale < 1e-11
        check_forward(got, want, "double", points, want_rms=ref_rms, zero_mean=False)
    norm = float(points)
    for r in range(P1 * P2):
        assert rel(backs[r] / norm, ins[r]) < 1e-10


# ------------------------------------------------------------------------------------------
# arbitrary lengths (the reference accepts any size through cuFFT): Bluestein passes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("N", [3, 5, 6, 7, 9, 10, 12, 15, 17, 30, 100, 127, 243, 250, 384, 500, 1000, 1023, 1025, 1500, 2047,
                               2049, 3000, 4095])
def test_fft1d_any_length_vs_oracle(N, prec):
    """variant -1 = the Bluestein kernel for every length (also those that have a native mixed-radix configuration)"""
    batch = 45
    rng = np.random.default_rng(N)
    x0 = rng.uniform(0, 255, (batch, N)) + 1j * rng.uniform(0, 255, (batch, N))
    for centred, x in ((False, x0.astype(NPDT[prec])), (True, (x0 - CENTER * (1 + 1j)).astype(NPDT[prec]))):      # the reference's distribution, and the same centred
        d_in = torch.from_numpy(x).cuda()
        d_out = torch.zeros_like(d_in)
        for direction in (dfft.FORWARD, dfft.INVERSE):
            torch.cuda.synchronize()
            dfft.fft1d_batched(d_out, d_in, N, batch, direction, prec, variant=-1)
            torch.cuda.synchronize()
            want = orc.fft1d(x.astype(np.complex128), direction)
            # per entry (parity_metric.py): the inverse of a line is a transform like any other
            check_forward(d_out.cpu().numpy(), want, prec, N, zero_mean=centred,
                          label=f"Bluestein fft1d N={N} dir={direction} centred={centred}" if N == 4095 else None)
            assert rel(d_out.cpu().numpy(), want) < (2e-11 if prec == "double" else 2e-4)


def mixed_lengths(prec):
    """the lengths of csrc/kernels_mixed.inc (generated by tools/gen_mixed_configs.py)"""
    import re
    inc = os.path.join(os.path.dirname(dfft.__file__), "csrc", "kernels_mixed.inc")
    tag = "F64" if prec == "double" else "F32"
    return sorted({int(m) for m in re.findall(r"using %s_M(\d+) =" % tag, open(inc).read())})


@pytest.mark.parametrize("prec", ["double", "float"])
def test_fft1d_mixed_radix_lengths_vs_oracle(prec):
    """every natively supported length that is not a power of two (radix 2, 3, 5, 7 butterflies in the Stockham chain;
    the reference takes any length through cufftMakePlanMany64, mpicufft_pencil_opt1.cpp:165-197): ragged batch, both
    directions, against the oracle; and the kernel info confirms the native chain (threads * points == N * lines)"""
    lengths = mixed_lengths(prec)
    assert len(lengths) >= 40
    for N in lengths:
        info = dfft.kernel_info(N, prec)
        assert info is not None and info["threads"] * info["points_per_thread"] == N * info["lines_per_workgroup"], (N, info)
        batch = 19 if N >= 256 else 77
        rng = np.random.default_rng(N)
        x0 = rng.uniform(0, 255, (batch, N)) + 1j * rng.uniform(0, 255, (batch, N))
        for centred, x in ((False, x0.astype(NPDT[prec])), (True, (x0 - CENTER * (1 + 1j)).astype(NPDT[prec]))):      # the reference's distribution, and the same centred
            d_in = torch.from_numpy(x).cuda()
            d_out = torch.zeros_like(d_in)
            for direction in (dfft.FORWARD, dfft.INVERSE):
                torch.cuda.synchronize()
                dfft.fft1d_batched(d_out, d_in, N, batch, direction, prec)
                torch.cuda.synchronize()
                want = orc.fft1d(x.astype(np.complex128), direction)
                check_forward(d_out.cpu().numpy(), want, prec, N, zero_mean=centred,
                              label=f"mixed radix fft1d N={N} dir={direction} centred={centred}" if N == lengths[-1] else None)
                assert rel(d_out.cpu().numpy(), want) < (2e-11 if prec == "double" else 2e-4), (N, direction)


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("shape,P1,P2", [((6, 10, 12), 1, 1), ((12, 20, 24), 2, 2), ((10, 12, 200), 1, 2), ((24, 6, 1000), 2, 1),
                                         ((6, 12, 1536), 1, 1), ((8, 6, 2000), 2, 3), ((20, 36, 1200), 1, 2), ((48, 40, 144), 3, 2)])
def test_mixed_radix_r2c_c2r_vs_oracle_and_bluestein(shape, P1, P2, prec):
    """R2C / C2R with a z axis whose half length runs the native mixed-radix chain (packed real pass: Nz/2-point complex
    transform + Hermitian split / merge): against the oracle, the round trip, and -- where the Bluestein kernel can serve
    the axis (Nz <= 1024) -- against the same plan with native_mixed = 0"""
    plans, ins, spec, backs = run_distributed_real(shape, P1, P2, prec)
    g = orc.fill_block(shape, (0, 0, 0), shape, 1, seed=13).astype(NPR[prec]).astype(np.float64)
    want = orc.fft3d_r2c(g)
    n3 = float(np.prod(shape))
    scale = np.max(np.abs(want))
    tol_f, tol_r = (2e-11, 1e-10) if prec == "double" else (2e-4, 5e-5)
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        ref = want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]]
        assert np.max(np.abs(spec[r] - ref)) / scale < tol_f
        assert rel(backs[r] / n3, ins[r]) < tol_r
    check_forward_blocks(plans, spec, want, prec, g.size, zero_mean=False)
    if max(shape) <= 1024:
        _, _, spec_b, _ = run_distributed_real(shape, P1, P2, prec, options={"native_mixed": 0})
        for r in range(len(plans)):
            assert np.max(np.abs(spec[r] - spec_b[r])) / scale < tol_f


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("shape,P1,P2", [((12, 20, 24), 1, 1), ((48, 36, 40), 2, 3), ((96, 100, 72), 2, 2), ((6, 1536, 10), 1, 2),
                                         ((2000, 6, 12), 2, 1), ((24, 12, 1000), 1, 3), ((160, 144, 120), 4, 2)])
def test_mixed_radix_grids_vs_oracle_and_bluestein(shape, P1, P2, prec):
    """distributed complex transform on grids whose axes run the native mixed-radix chain: against the oracle, and
    against the same plan with option native_mixed=0 (Bluestein on every axis it can serve)"""
    if prec == "float" and not all(n in mixed_lengths("float") for n in shape):
        pytest.skip("length without fp32 configuration")
    plans, ins, spec, backs = run_distributed(shape, P1, P2, prec)
    want = orc.fft3d_c2c(orc.fill_block(shape, (0, 0, 0), shape, 2, seed=7), -1)
    n3 = float(np.prod(shape))
    tol_f, tol_r = (2e-11, 1e-10) if prec == "double" else (2e-4, 5e-5)
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        ref = want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]]
        assert np.max(np.abs(spec[r] - ref)) / np.max(np.abs(want)) < tol_f
        assert rel(backs[r] / n3, ins[r]) < tol_r
    check_forward_blocks(plans, spec, want, prec, want.size, zero_mean=False)
    if max(shape) <= 1024:
        plans_b, _, spec_b, _ = run_distributed(shape, P1, P2, prec, options={"native_mixed": 0})
        for r in range(len(plans)):
            assert np.max(np.abs(spec[r] - spec_b[r])) / np.max(np.abs(want)) < tol_f


@pytest.mark.parametrize("shape", [(12, 10, 14), (9, 7, 10), (30, 16, 50), (100, 3, 24), (5, 384, 6), (1031, 6, 9), (4, 2500, 10),
                                   (3, 5, 4095)])
def test_single_rank_any_size_vs_oracle_and_golden(shape):
    g, got, back = run_single(shape, "double", seed=20260921)
    want = orc.fft3d_c2c(g, -1)
    assert rel(got, want) < 2e-11
    check_forward(got, want, "double", g.size, zero_mean=False)
    assert rel(back / g.size, g) < 1e-10
    if shape == (12, 10, 14):
        d = np.load(os.path.join(GOLD, "fft3d_small.npz"))
        assert rel(got, d["c2c_12x10x14"]) < 2e-11


@pytest.mark.parametrize("shape,P1,P2", [((12, 10, 14), 2, 4), ((9, 7, 10), 3, 2), ((10, 9, 12), 3, 1), ((30, 20, 18), 2, 3),
                                         ((6, 1100, 2310), 2, 2)])
def test_distributed_any_size_c2c_and_r2c(shape, P1, P2):
    """the uneven, non-power-of-two grids the survey replayed, C2C and R2C
    (R2C with odd and even Nz: Hermitian half via the real Bluestein modes)"""
    plans, ins, spec, backs = run_distributed(shape, P1, P2, "double")
    want = orc.fft3d_c2c(orc.fill_block(shape, (0, 0, 0), shape, 2, seed=7), -1)
    n3 = float(np.prod(shape))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        ref = want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]]
        assert np.max(np.abs(spec[r] - ref)) / np.max(np.abs(want)) < 2e-11
        assert rel(backs[r] / n3, ins[r]) < 1e-10
    check_forward_blocks(plans, spec, want, "double", want.size, zero_mean=False)
    for shp in (shape, (shape[0], shape[1], shape[2] + 1)):
        plans, ins, spec, backs = run_distributed_real(shp, P1, P2, "double")
        wantr = orc.fft3d_r2c(orc.fill_block(shp, (0, 0, 0), shp, 1, seed=13))
        n3 = float(np.prod(shp))
        for r, pl in enumerate(plans):
            s, o = pl.getOutSize(), pl.getOutStart()
            ref = wantr[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]]
            assert np.max(np.abs(spec[r] - ref)) / np.max(np.abs(wantr)) < 2e-11
            assert rel(backs[r] / n3, ins[r]) < 1e-10
        check_forward_blocks(plans, spec, wantr, "double", int(n3), zero_mean=False)


@pytest.mark.parametrize("c2c", [True, False])
def test_graph_replay_of_repeated_execs(c2c):
    """with option "graph" a single-rank plan captures the launches of an exec into a hipGraph at the second call with the
    same buffers and replays it afterwards: every call -- plain, captured, replayed -- must transform the CURRENT contents
    of the buffers; changing an option or re-initialising drops the graphs"""
    shape = (24, 32, 40)
    plan = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations())
    assert plan.getOption("graph") == 0       # off by default: plain launches measured faster (profiles/r2_graph_latency.txt)
    plan.setOption("graph", 1)
    plan.initFFT(dfft.GlobalSize(*shape), dfft.Pencil_Partition(1, 1), True, c2c=c2c)
    rng = np.random.default_rng(3)
    if c2c:
        d_in = torch.zeros(shape, dtype=torch.complex128, device="cuda")
    else:
        d_in = torch.zeros(shape, dtype=torch.float64, device="cuda")
    d_out = torch.zeros(plan.getDomainSize() // 16, dtype=torch.complex128, device="cuda")
    d_back = torch.zeros_like(d_in)
    n3 = float(np.prod(shape))
    for it in range(6):
        if it == 4:
            plan.setOption("graph", 0)          # plain launches again (and the cached graphs are gone)
        x = rng.uniform(0, 255, shape) + (1j * rng.uniform(0, 255, shape) if c2c else 0)
        d_in.copy_(torch.from_numpy(x if c2c else x.real.copy()).cuda())
        torch.cuda.synchronize()
        if c2c:
            plan.execC2C(d_out, d_in, dfft.FORWARD)
            want = orc.fft3d_c2c(x, -1)
        else:
            plan.execR2C(d_out, d_in)
            want = orc.fft3d_r2c(x.real)
        got = d_out[:want.size].cpu().numpy().reshape(want.shape)
        assert rel(got, want) < 1e-11, it
        if c2c:
            plan.execC2C(d_back, d_out, dfft.INVERSE)
        else:
            plan.execC2R(d_back, d_out)
        assert rel(d_back.cpu().numpy() / n3, x if c2c else x.real) < 1e-10, it
    plan.setOption("graph", 1)
    plan.initFFT(dfft.GlobalSize(16, 16, 16), dfft.Pencil_Partition(1, 1), True, c2c=True)     # re-plan: other kernels, other sizes
    y = rng.uniform(0, 1, (16, 16, 16)) + 1j * rng.uniform(0, 1, (16, 16, 16))
    d2 = torch.from_numpy(y).cuda()
    o2 = torch.zeros(plan.getDomainSize() // 16, dtype=torch.complex128, device="cuda")
    for _ in range(3):
        plan.execC2C(o2, d2, dfft.FORWARD)
        assert rel(o2[:y.size].cpu().numpy().reshape(y.shape), orc.fft3d_c2c(y, -1)) < 1e-11


def test_plan_can_be_reinitialised():
    """initFFT twice on one object (the reference allows it: plans are rebuilt in initFFT)"""
    plan = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), precision="double")
    for shape, c2c in [((32, 32, 32), True), ((16, 64, 8), False), ((12, 10, 14), True), ((64, 16, 32), True)]:
        plan.initFFT(dfft.GlobalSize(*shape), dfft.Pencil_Partition(1, 1), True, c2c=c2c)
        g = orc.fill_block(shape, (0, 0, 0), shape, 2 if c2c else 1, seed=3)
        d_in = torch.from_numpy(g).cuda()
        d_out = torch.zeros(plan.getDomainSize() // 16, dtype=torch.complex128, device="cuda")
        torch.cuda.synchronize()
        if c2c:
            plan.execC2C(d_out, d_in, dfft.FORWARD)
            want = orc.fft3d_c2c(g, -1)
        else:
            plan.execR2C(d_out, d_in)
            want = orc.fft3d_r2c(g)
        got = d_out[:want.size].cpu().numpy().reshape(want.shape)
        assert rel(got, want) < 2e-11


def test_randomised_sweep_of_shapes_partitions_and_depths():
    """60 random (grid, P1 x P2, pipeline depth, R2C|C2C) combinations against the oracle: tiny and
    odd extents, partitions as large as the extents allow, depths that do not divide anything"""
    rng = np.random.default_rng(20260921)
    sizes = [2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 15, 16, 18, 20, 24, 27, 30, 32, 33, 40, 48, 64]
    done = 0
    while done < 60:
        shape = tuple(int(rng.choice(sizes)) for _ in range(3))
        c2c = bool(rng.integers(0, 2))
        Nzc = shape[2] if c2c else shape[2] // 2 + 1
        P1 = int(rng.integers(1, 5))
        P2 = int(rng.integers(1, 5))
        if P1 > min(shape[0], shape[1]) or P2 > min(shape[1], Nzc):
            continue
        chunks = int(rng.integers(1, 6))
        if c2c:
            plans, ins, spec, backs = run_distributed(shape, P1, P2, "double", seed=done, chunks=chunks)
            g = orc.fill_block(shape, (0, 0, 0), shape, 2, seed=done)
            want = orc.fft3d_c2c(g, -1)
        else:
            P = P1 * P2
            world = dfft.Comm.local(P) if P > 1 else None
            plans, ins, outs, backs = [], [], [], []
            for r in range(P):
                pl = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), world, precision="double", rank=r)
                pl.setPipelineChunks(chunks)
                pl.initFFT(dfft.GlobalSize(*shape), dfft.Pencil_Partition(P1, P2), True)
                s, o = pl.getInSize(), pl.getInStart()
                plans.append(pl)
                ins.append(torch.from_numpy(orc.fill_block(shape, o, s, 1, seed=done)).cuda())
                outs.append(torch.zeros(pl.getDomainSize() // 16, dtype=torch.complex128, device="cuda"))
                backs.append(torch.zeros_like(ins[-1]))
            torch.cuda.synchronize()
            with ThreadPoolExecutor(P) as ex:
                list(ex.map(lambda r: plans[r].execR2C(outs[r], ins[r]), range(P)))
            spec = []
            for r in range(P):
                s = plans[r].getOutSize()
                spec.append(outs[r][:s[0] * s[1] * s[2]].cpu().numpy().reshape(s))
            with ThreadPoolExecutor(P) as ex:
                list(ex.map(lambda r: plans[r].execC2R(backs[r], outs[r]), range(P)))
            torch.cuda.synchronize()
            ins = [t.cpu().numpy() for t in ins]
            backs = [t.cpu().numpy() for t in backs]
            want = orc.fft3d_r2c(orc.fill_block(shape, (0, 0, 0), shape, 1, seed=done))
        n3 = float(np.prod(shape))
        scale = np.max(np.abs(want))
        for r, pl in enumerate(plans):
            s, o = pl.getOutSize(), pl.getOutStart()
            ref = want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]]
            assert np.max(np.abs(spec[r] - ref)) / scale < 2e-11, (shape, P1, P2, chunks, c2c, r)
            assert rel(backs[r] / n3, ins[r]) < 1e-10, (shape, P1, P2, chunks, c2c, r)
        check_forward_blocks(plans, spec, want, "double", int(n3), zero_mean=False)
        done += 1


@pytest.mark.parametrize("shape,P1,P2", [((64, 64, 64), 4, 4), ((64, 32, 16), 16, 1), ((16, 64, 64), 1, 16), ((48, 48, 20), 6, 3)])
def test_sixteen_and_eighteen_ranks(shape, P1, P2):
    """two-node sized grids (the reference ran 4x4 on 16 GPUs, results_16.csv) as virtual ranks"""
    plans, ins, spec, backs = run_distributed(shape, P1, P2, "double")
    want = orc.fft3d_c2c(orc.fill_block(shape, (0, 0, 0), shape, 2, seed=7), -1)
    n3 = float(np.prod(shape))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        ref = want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]]
        assert np.max(np.abs(spec[r] - ref)) / np.max(np.abs(want)) < 2e-11
        assert rel(backs[r] / n3, ins[r]) < 1e-10
    check_forward_blocks(plans, spec, want, "double", want.size, zero_mean=False)


@pytest.mark.parametrize("mode", ["0", "2"])
def test_address_table_modes_agree(mode, monkeypatch):
    """DFFT_TABLES: 0 = segment search per point, 2 = per-point tables on every tiled side (the
    default uses tables only for sides with more than one segment).  All three must give the same
    spectrum; covers C2C and R2C, pencil and slab, chunked."""
    monkeypatch.setenv("DFFT_TABLES", mode)
    for shape, P1, P2 in (((32, 32, 32), 2, 4), ((64, 32, 16), 8, 1), ((16, 16, 16), 1, 1)):
        plans, ins, spec, backs = run_distributed(shape, P1, P2, "double", chunks=3)
        want = orc.fft3d_c2c(orc.fill_block(shape, (0, 0, 0), shape, 2, seed=7), -1)
        n3 = float(np.prod(shape))
        for r, pl in enumerate(plans):
            s, o = pl.getOutSize(), pl.getOutStart()
            assert np.max(np.abs(spec[r] - want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]])) / np.max(np.abs(want)) < 1e-11
            assert rel(backs[r] / n3, ins[r]) < 1e-10
        check_forward_blocks(plans, spec, want, "double", want.size, zero_mean=False)
    plans, ins, spec, backs = run_distributed_real((32, 16, 64), 2, 2, "float")
    wantr = orc.fft3d_r2c(orc.fill_block((32, 16, 64), (0, 0, 0), (32, 16, 64), 1, seed=13).astype(np.float32).astype(np.float64))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert np.max(np.abs(spec[r] - wantr[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]])) / np.max(np.abs(wantr)) < 1e-4
    check_forward_blocks(plans, spec, wantr, "float", 32 * 16 * 64, zero_mean=False)      # fp32, non-negative input: recorded only


# ------------------------------------------------------------------------------------------
# option compute_streams = 2: the pipeline chunks of a pass alternate over two compute streams
# ------------------------------------------------------------------------------------------
def used_stream_1(plans):
    """from what the last forward and inverse exec of every rank issued (option trace): did any of them use the second compute stream"""
    issued = [pl.debugTrace(d, 0) for pl in plans for d in (dfft.FORWARD, dfft.INVERSE)]
    assert all(issued)
    return any(o["stream"] == 1 for t in issued for o in t)


# small grids at every depth, and one pencil and one slab grid large enough that a chunk's kernels are not launch-bound (256 x 256 x 128
# fp64: 0.27 GB per buffer over all virtual ranks), so that the two streams really overlap
TWO_STREAM_SMALL = [((32, 32, 32), 2, 4), ((16, 16, 16), 3, 2), ((64, 32, 16), 8, 1), ((16, 32, 16), 1, 4), ((128, 64, 32), 2, 4)]
TWO_STREAM_LARGE = [((256, 256, 128), 2, 4, 4), ((256, 256, 128), 8, 1, 4)]
TWO_STREAM_CASES = [pytest.param(s, P1, P2, c, id=f"shape{i}-{P1}-{P2}-{c}") for c in (2, 3, 4, 8) for i, (s, P1, P2) in enumerate(TWO_STREAM_SMALL)] + \
                   [pytest.param(s, P1, P2, c, id=f"shape{len(TWO_STREAM_SMALL) + i}-{P1}-{P2}-{c}") for i, (s, P1, P2, c) in enumerate(TWO_STREAM_LARGE)]


@pytest.mark.parametrize("shape,P1,P2,chunks", TWO_STREAM_CASES)
def test_two_compute_streams_are_bit_identical_to_one(shape, P1, P2, chunks):
    """the same kernels on the same data in another stream assignment: spectrum and round trip must not change by one bit
    (a missing dependency between the two compute streams shows up as a difference or as a wrong result against the oracle);
    the trace of what was issued says that the two-stream runs used the second stream and the one-stream run did not"""
    ref = run_distributed(shape, P1, P2, "double", chunks=chunks, options={"compute_streams": 1, "trace": 1})
    assert not used_stream_1(ref[0])
    want = orc.fft3d_c2c(orc.fill_block(shape, (0, 0, 0), shape, 2, seed=7), -1)
    for _ in range(3):          # scheduling varies from run to run
        two = run_distributed(shape, P1, P2, "double", chunks=chunks, options={"compute_streams": 2, "trace": 1})
        assert two[0][0].getOption("compute_streams") == 2
        assert used_stream_1(two[0])
        for r in range(P1 * P2):
            assert np.array_equal(two[2][r], ref[2][r]) and np.array_equal(two[3][r], ref[3][r])
    for r, pl in enumerate(ref[0]):
        s, o = pl.getOutSize(), pl.getOutStart()
        check_forward(ref[2][r], want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]], "double", want.size, want_rms=rms(want), zero_mean=False)


@pytest.mark.parametrize("shape,P1,P2", [((32, 32, 32), 2, 4), ((64, 32, 16), 4, 1), ((16, 32, 64), 1, 4), ((256, 256, 128), 2, 4), ((256, 256, 128), 8, 1)])
def test_two_compute_streams_r2c_bit_identical(shape, P1, P2):
    ref = run_distributed_real(shape, P1, P2, "double", options={"compute_streams": 1, "trace": 1})
    assert not used_stream_1(ref[0])
    for _ in range(3):
        two = run_distributed_real(shape, P1, P2, "double", options={"compute_streams": 2, "trace": 1})
        assert used_stream_1(two[0])
        for r in range(P1 * P2):
            assert np.array_equal(two[2][r], ref[2][r]) and np.array_equal(two[3][r], ref[3][r])
