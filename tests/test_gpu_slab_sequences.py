"""Alternative slab sequence Z_Then_YX (reference: src/slab/z_then_yx/, include/mpicufft_slab_z_then_yx.hpp):
input split along x, ONE all-to-all over all ranks after the z pass, output [Nx][Ny][Nzc/P] split
along z.  Checked like the reference's slab testcases: distributed == single-device transform
(testcase 1), round trip (testcase 3), analytic Laplacian (testcase 4).  Tolerances as in
test_gpu_parity.py."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import distributedfft_amd as dfft  # noqa: E402
from oracle import oracle as orc  # noqa: E402

from parity_metric import CENTER, check_forward_blocks  # noqa: E402

TOL_FWD = {"double": 1e-11, "float": 1e-4}
TOL_RT = {"double": 1e-10, "float": 5e-5}
CDT = {"double": torch.complex128, "float": torch.complex64}
NPC = {"double": np.complex128, "float": np.complex64}
NPR = {"double": np.float64, "float": np.float32}


def run(cls, shape, P, prec, c2c, chunks=None, field=None, modify=None, seed=21, options=None, center=False, arena=None):
    """arena (tests/guarded.py): every buffer and a caller-owned work area come from it, refilled before either exec, and the guards and
    the inputs are checked after either exec; a second call with the same arena runs the plans and the buffers of the first"""
    esz = 16 if prec == "double" else 8

    def setup():
        world = dfft.Comm.local(P) if P > 1 else None
        plans, ins, outs, backs, host_ins = [], [], [], [], []
        for r in range(P):
            pl = cls(dfft.Configurations(), world, precision=prec, rank=r)
            if chunks is not None:
                pl.setPipelineChunks(chunks)
            for k, v in (options or {}).items():
                pl.setOption(k, v)
            pl.initFFT(dfft.GlobalSize(*shape), dfft.Slab_Partition(P), arena is None, c2c=c2c)
            size, start = pl.getInSize(), pl.getInStart()
            assert tuple(size[1:]) == tuple(shape[1:]) and tuple(start[1:]) == (0, 0)
            if field is not None:
                blk = np.ascontiguousarray(field[start[0]:start[0] + size[0]]).astype(NPR[prec])
            elif c2c:
                blk = (orc.fill_block(shape, start, size, 2, seed=seed) - (CENTER * (1 + 1j) if center else 0.0)).astype(NPC[prec])
            else:
                blk = (orc.fill_block(shape, start, size, 1, seed=seed) - (CENTER if center else 0.0)).astype(NPR[prec])
            plans.append(pl)
            host_ins.append(blk.copy())
            if arena is not None:
                for lst, t in zip((ins, outs, backs), arena.plan_buffers(pl, blk, CDT[prec], r)):
                    lst.append(t)
                continue
            ins.append(torch.from_numpy(blk).cuda())
            outs.append(torch.zeros(pl.getDomainSize() // esz, dtype=CDT[prec], device="cuda"))
            backs.append(torch.zeros_like(ins[-1]))
        return plans, ins, outs, backs, host_ins

    plans, ins, outs, backs, host_ins = setup() if arena is None else arena.once("slabs.run", setup)
    what = f"slabs.run {cls.__name__} {shape} P={P} {'C2C' if c2c else 'R2C'} {prec}"
    if arena is not None:
        arena.refill()
    torch.cuda.synchronize()
    fwd = (lambda r: plans[r].execC2C(outs[r], ins[r], dfft.FORWARD)) if c2c else (lambda r: plans[r].execR2C(outs[r], ins[r]))
    inv = (lambda r: plans[r].execC2C(backs[r], outs[r], dfft.INVERSE)) if c2c else (lambda r: plans[r].execC2R(backs[r], outs[r]))
    with ThreadPoolExecutor(P) as ex:
        list(ex.map(fwd, range(P)))
    torch.cuda.synchronize()
    if arena is not None:
        arena.check_guards(what + " forward")
        arena.check_inputs(what + " forward")
    spec = []
    for r in range(P):
        s = plans[r].getOutSize()
        spec.append(outs[r][:s[0] * s[1] * s[2]].cpu().numpy().reshape(s))
    if modify is not None:
        for r in range(P):
            s, o = plans[r].getOutSize(), plans[r].getOutStart()
            blk = np.ascontiguousarray(spec[r].astype(np.complex128))
            modify(blk, s, o)
            outs[r][:blk.size] = torch.from_numpy(blk.astype(NPC[prec]).ravel()).cuda()
    torch.cuda.synchronize()
    for r in range(P):
        assert np.array_equal(ins[r].cpu().numpy(), host_ins[r]), "forward must not modify its input"
    if arena is not None:
        arena.refill(keep=outs)
    with ThreadPoolExecutor(P) as ex:
        list(ex.map(inv, range(P)))
    torch.cuda.synchronize()
    if arena is not None:
        arena.check_guards(what + " inverse")
    return plans, [t.cpu().numpy() for t in ins], spec, [t.cpu().numpy() for t in backs]


def global_input(shape, c2c, prec, seed=21, center=False):
    g = orc.fill_block(shape, (0, 0, 0), shape, 2 if c2c else 1, seed=seed)
    if center:      # what run / run_yzx subtract with center=True
        g = g - (CENTER * (1 + 1j) if c2c else CENTER)
    return g.astype(NPC[prec]).astype(np.complex128) if c2c else g.astype(NPR[prec]).astype(np.float64)


CASES = [((16, 16, 16), 2), ((32, 16, 64), 3), ((64, 32, 16), 8), ((8, 4, 16), 2), ((33, 20, 18), 4),
         ((24, 10, 20), 4), ((128, 64, 32), 5)]


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False])
@pytest.mark.parametrize("shape,P", CASES)
def test_z_then_yx_vs_oracle(shape, P, c2c, prec):
    cls = dfft.MPIcuFFT_Slab_Z_Then_YX
    plans, ins, spec, backs = run(cls, shape, P, prec, c2c)
    g = global_input(shape, c2c, prec)
    want = orc.fft3d_c2c(g, -1) if c2c else orc.fft3d_r2c(g)
    Nzc = want.shape[2]
    n3 = float(np.prod(shape))
    scale = np.max(np.abs(want))
    cover = np.zeros(Nzc, dtype=int)
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert tuple(s[:2]) == tuple(shape[:2]) and tuple(o[:2]) == (0, 0)
        cover[o[2]:o[2] + s[2]] += 1
        ref = want[:, :, o[2]:o[2] + s[2]]
        assert np.max(np.abs(spec[r] - ref)) / scale < TOL_FWD[prec]
        assert np.max(np.abs(backs[r] / n3 - ins[r])) / 255.0 < TOL_RT[prec]
    assert np.all(cover == 1)
    check_forward_blocks(plans, spec, want, prec, int(n3), zero_mean=False)


@pytest.mark.parametrize("chunks", [1, 2, 3, 8])
@pytest.mark.parametrize("shape,P", [((32, 16, 64), 3), ((64, 32, 16), 4)])
def test_z_then_yx_pipeline_depths_and_opt1_class(shape, P, chunks):
    plans, ins, spec, backs = run(dfft.MPIcuFFT_Slab_Z_Then_YX_Opt1, shape, P, "double", False, chunks=chunks)
    assert 1 <= plans[0].getPipelineChunks() <= chunks
    want = orc.fft3d_r2c(global_input(shape, False, "double"))
    n3 = float(np.prod(shape))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert np.max(np.abs(spec[r] - want[:, :, o[2]:o[2] + s[2]])) / np.max(np.abs(want)) < 1e-11
        assert np.max(np.abs(backs[r] / n3 - ins[r])) / 255.0 < 1e-10


def test_z_then_yx_laplacian_known_answer():
    """reference testcase 4 on the z-split output (tests/src/slab/random_dist_z_then_yx.cu)"""
    shape, P = (32, 32, 32), 4
    Nx, Ny, Nz = shape
    x, y, z = np.meshgrid(np.arange(Nx), np.arange(Ny), np.arange(Nz), indexing="ij")
    u = np.sin(2 * np.pi * x / Nx) * np.sin(2 * np.pi * y / Ny) * np.sin(2 * np.pi * z / Nz)

    def modify(blk, s, o):
        orc.derivative_coefficients(blk, shape, o[2], o[1], half=True)

    plans, ins, spec, backs = run(dfft.MPIcuFFT_Slab_Z_Then_YX, shape, P, "double", False, field=u, modify=modify)
    n3 = float(Nx * Ny * Nz)
    for r in range(P):
        assert np.max(np.abs(backs[r] - orc.testcase4_expected(shape, ins[r]))) < 1e-9 * np.sqrt(n3)


def test_z_then_yx_256_cube_four_ranks_every_point():
    shape, P = (256, 256, 256), 4
    plans, ins, spec, backs = run(dfft.MPIcuFFT_Slab_Z_Then_YX, shape, P, "double", True)
    want = orc.fft3d_c2c(global_input(shape, True, "double"), -1)
    scale = np.max(np.abs(want))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert np.max(np.abs(spec[r] - want[:, :, o[2]:o[2] + s[2]])) / scale < 1e-11
        assert np.max(np.abs(backs[r] / float(np.prod(shape)) - ins[r])) / 255.0 < 1e-10


def test_z_then_yx_errors_and_single_rank():
    world = dfft.Comm.local(4)
    pl = dfft.MPIcuFFT_Slab_Z_Then_YX(dfft.Configurations(), world, rank=0)
    with pytest.raises(dfft.DfftError, match="partition larger"):
        pl.initFFT(dfft.GlobalSize(16, 16, 4), dfft.Slab_Partition(4), True)     # Nz/2+1 = 3 < 4 ranks
    with pytest.raises(dfft.DfftError, match="P2 == 1"):
        pl.initFFT(dfft.GlobalSize(16, 16, 16), dfft.Pencil_Partition(2, 2), True)
    pl.initFFT(dfft.GlobalSize(16, 16, 16), dfft.Slab_Partition(4), True)
    with pytest.raises(dfft.DfftError, match="Z_Then_YX"):
        pl.execR2C(1, 1, d=1)
    # one rank: the plain local 3-D transform (fft3d branch)
    plans, ins, spec, backs = run(dfft.MPIcuFFT_Slab_Z_Then_YX, (16, 8, 32), 1, "double", False)
    want = orc.fft3d_r2c(global_input((16, 8, 32), False, "double"))
    assert np.max(np.abs(spec[0] - want)) / np.max(np.abs(want)) < 1e-11


# ------------------------------------------------------------------------------------------
# Y_Then_ZX (src/slab/y_then_zx/): R2C along y, output [Nx][(Ny/2+1)/P][Nz], forward only
# ------------------------------------------------------------------------------------------
def run_yzx(shape, P, prec, c2c, chunks=None, seed=33, options=None, center=False, arena=None):
    """arena: as in run (forward only: `in`, `out` and the work area)"""
    esz = 16 if prec == "double" else 8

    def setup():
        world = dfft.Comm.local(P) if P > 1 else None
        plans, ins, outs, host_ins = [], [], [], []
        for r in range(P):
            pl = dfft.MPIcuFFT_Slab_Y_Then_ZX(dfft.Configurations(), world, precision=prec, rank=r)
            if chunks is not None:
                pl.setPipelineChunks(chunks)
            for k, v in (options or {}).items():
                pl.setOption(k, v)
            pl.initFFT(dfft.GlobalSize(*shape), dfft.Slab_Partition(P), arena is None, c2c=c2c)
            size, start = pl.getInSize(), pl.getInStart()
            blk = orc.fill_block(shape, start, size, 2 if c2c else 1, seed=seed)
            if center:
                blk = blk - (CENTER * (1 + 1j) if c2c else CENTER)
            blk = blk.astype(NPC[prec] if c2c else NPR[prec])
            plans.append(pl)
            host_ins.append(blk)
            if arena is not None:
                arena.domain(pl.getDomainSize())
                ins.append(arena.input(blk, f"in[{r}]"))
                outs.append(arena.buffer(pl.getDomainSize(), CDT[prec], name=f"out[{r}]"))
                arena.work_area(pl, r)
                continue
            ins.append(torch.from_numpy(blk).cuda())
            outs.append(torch.zeros(pl.getDomainSize() // esz, dtype=CDT[prec], device="cuda"))
        return plans, ins, outs, host_ins

    plans, ins, outs, host_ins = setup() if arena is None else arena.once("slabs.run_yzx", setup)
    if arena is not None:
        arena.refill()
    torch.cuda.synchronize()
    fwd = (lambda r: plans[r].execC2C(outs[r], ins[r], dfft.FORWARD)) if c2c else (lambda r: plans[r].execR2C(outs[r], ins[r]))
    with ThreadPoolExecutor(P) as ex:
        list(ex.map(fwd, range(P)))
    torch.cuda.synchronize()
    if arena is not None:
        what = f"slabs.run_yzx {shape} P={P} {'C2C' if c2c else 'R2C'} {prec} forward"
        arena.check_guards(what)
        arena.check_inputs(what)
    spec = []
    for r in range(P):
        s = plans[r].getOutSize()
        spec.append(outs[r][:s[0] * s[1] * s[2]].cpu().numpy().reshape(s))
        assert np.array_equal(ins[r].cpu().numpy(), host_ins[r])
    return plans, spec


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [False, True])
@pytest.mark.parametrize("shape,P", [((16, 16, 16), 1), ((16, 16, 16), 2), ((32, 16, 64), 3), ((64, 32, 16), 8),
                                     ((33, 20, 18), 4), ((24, 10, 20), 4), ((128, 64, 32), 5), ((8, 6, 4), 2)])
def test_y_then_zx_vs_oracle(shape, P, c2c, prec):
    plans, spec = run_yzx(shape, P, prec, c2c)
    g = global_input(shape, c2c, prec, seed=33)
    want = orc.fft3d_c2c(np.ascontiguousarray(g.astype(np.complex128)), -1)
    Nyc = shape[1] if c2c else shape[1] // 2 + 1
    want = want[:, :Nyc, :]
    scale = np.max(np.abs(want))
    cover = np.zeros(Nyc, dtype=int)
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert (s[0], s[2]) == (shape[0], shape[2]) and (o[0], o[2]) == (0, 0)
        cover[o[1]:o[1] + s[1]] += 1
        assert np.max(np.abs(spec[r] - want[:, o[1]:o[1] + s[1], :])) / scale < TOL_FWD[prec]
    assert np.all(cover == 1)
    check_forward_blocks(plans, spec, want, prec, int(np.prod(shape)), zero_mean=False)


@pytest.mark.parametrize("chunks", [1, 2, 5])
def test_y_then_zx_pipeline_depths_tables_and_errors(chunks):
    shape, P = (32, 16, 64), 3
    plans, spec = run_yzx(shape, P, "double", False, chunks=chunks)
    Nx, Ny, Nz = shape
    want = orc.fft3d_c2c(np.ascontiguousarray(global_input(shape, False, "double", seed=33).astype(np.complex128)), -1)[:, :Ny // 2 + 1, :]
    xs = [Nx // P + (1 if q < Nx % P else 0) for q in range(P)]
    yo = [(Ny // 2 + 1) // P + (1 if q < (Ny // 2 + 1) % P else 0) for q in range(P)]
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert np.max(np.abs(spec[r] - want[:, o[1]:o[1] + s[1], :])) / np.max(np.abs(want)) < 1e-11
        # byte counts of mpicufft_slab_y_then_zx.cpp:309-319
        sc, sd, rc, rd = pl.getExchangeTables(2)
        assert sc == [16 * Nz * yo[q] * xs[r] for q in range(P)] and rc == [16 * Nz * yo[r] * xs[q] for q in range(P)]
        assert sd == [16 * Nz * sum(yo[:q]) * xs[r] for q in range(P)] and rd == [16 * Nz * yo[r] * sum(xs[:q]) for q in range(P)]
    with pytest.raises(dfft.DfftError, match="forward only"):
        plans[0].execC2R(1, 1)
    one = dfft.MPIcuFFT_Slab_Y_Then_ZX(dfft.Configurations())
    with pytest.raises(dfft.DfftError, match="unsupported axis length"):      # beyond the 32-bit point indices of the generic kernel
        one.initFFT(dfft.GlobalSize(16, (1 << 24) + 1, 16), dfft.Slab_Partition(1), False)


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("shape,P", [((16, 2048, 16), 2), ((24, 1024, 32), 1), ((8, 512, 16), 3), ((16, 256, 8), 2)])
def test_y_then_zx_long_power_of_two_real_lines(shape, P, prec):
    """power-of-two Ny runs the packed Ny/2-point real kernel on strided lines (no Bluestein, no Ny <= 1024 limit)"""
    plans, spec = run_yzx(shape, P, prec, False)
    g = global_input(shape, False, prec, seed=33)
    want = orc.fft3d_c2c(np.ascontiguousarray(g.astype(np.complex128)), -1)[:, :shape[1] // 2 + 1, :]
    scale = np.max(np.abs(want))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        err = np.max(np.abs(spec[r] - want[:, o[1]:o[1] + s[1], :])) / scale
        assert err < (1e-11 if prec == "double" else 1e-4), err


@pytest.mark.parametrize("shape,P", [((16, 1536, 16), 2), ((8, 1100, 24), 1), ((6, 3001, 16), 3)])
def test_y_then_zx_long_real_lines_through_bluestein(shape, P):
    """Ny that is not a power of two: the Bluestein kernel's real mode on strided lines, inner transforms of up to 8192
    points (sub-tile workgroups) for Ny up to 4096"""
    plans, spec = run_yzx(shape, P, "double", False)
    g = global_input(shape, False, "double", seed=33)
    want = orc.fft3d_c2c(np.ascontiguousarray(g.astype(np.complex128)), -1)[:, :shape[1] // 2 + 1, :]
    scale = np.max(np.abs(want))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert np.max(np.abs(spec[r] - want[:, o[1]:o[1] + s[1], :])) / scale < 2e-11


def test_y_then_zx_256_cube_four_ranks_every_point():
    shape, P = (256, 256, 256), 4
    plans, spec = run_yzx(shape, P, "double", False)
    want = orc.fft3d_c2c(np.ascontiguousarray(global_input(shape, False, "double", seed=33).astype(np.complex128)), -1)[:, :129, :]
    scale = np.max(np.abs(want))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert np.max(np.abs(spec[r] - want[:, o[1]:o[1] + s[1], :])) / scale < 1e-11
