"""execSpectralOp (option "spectral_op", include/dfft_c.h: dfft_exec_spectral_op): out = IFFT(m * FFT(in)) as one chain whose forward
and inverse x passes are a single kernel (fft_spectral_kernel) with the multiplier between them -- the loop of the reference's testcase 4
(tests/src/pencil/random_dist_3D.cu:685-811) in one call.

Reference: numpy in float64, irfftn(rfftn(u) * m) * n resp. ifftn(fftn(u) * m) * n, with u and m rounded to the plan's precision first.
Metric: the project's per-entry one (tests/parity_metric.py), rms_rel(got, want) <= 2 * forward_bound(prec, n): two transforms, each held
to the per-entry forward bound; |m| <= 1 so the multiplier adds nothing.  Inputs are zero-mean (uniform - 127.5).  The x lengths run
through every configuration the kernel is instantiated for, 2 .. 2048 (2 and 4 take the E < 8 branch of the multiplier loop), in the
array form and in the table forms (test_table_multiplier_against_numpy: integer tables that are neither smooth nor symmetric)."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import distributedfft_amd as dfft  # noqa: E402
from oracle import oracle as orc  # noqa: E402

from parity_metric import CENTER, forward_bound, record, rms, rms_rel, worst_entry  # noqa: E402
from test_gpu_parity import CDT, NPDT, NPR, RDT, TOL_RT, rel  # noqa: E402

SHAPES = [(16, 8, 16), (64, 24, 20), (512, 8, 16), (1024, 8, 8), (2048, 8, 16),
          (2, 12, 10), (4, 12, 10), (8, 12, 10), (128, 12, 10), (256, 12, 10)]
S = dfft.SPECTRAL_OP
GRIDS = [(1, 1), (2, 1), (1, 2), (2, 2)]


def make_plans(shape, P1, P2, prec, c2c, layout, chunks=None, cls=dfft.MPIcuFFT_Pencil_Opt1, options=None, arena=None):
    """arena (tests/guarded.py): the plans are initialised with allocate=False and get a guarded caller-owned work area each"""
    P = P1 * P2
    world = dfft.Comm.local(P) if P > 1 else None
    plans = []
    for r in range(P):
        pl = cls(dfft.Configurations(), world, precision=prec, rank=r)
        if chunks is not None:
            pl.setPipelineChunks(chunks)
        pl.setOption("spectral_op", 1)
        pl.setOption("spectral_layout", layout)
        for k, v in (options or {}).items():
            pl.setOption(k, v)
        pl.initFFT(dfft.GlobalSize(*shape), dfft.Partition(P1, P2), arena is None, c2c=c2c)
        if arena is not None:
            arena.work_area(pl, r)
        plans.append(pl)
    return plans


def in_block(pl, a):
    (nx, ny, nz), (x0, y0, z0) = pl.getInSize(), pl.getInStart()
    return np.ascontiguousarray(a[x0:x0 + nx, y0:y0 + ny, z0:z0 + nz])


def spectrum_block(pl, a):
    (_, ny, nz), (_, y0, z0) = pl.getOutSize(), pl.getOutStart()
    return np.ascontiguousarray(a[:, y0:y0 + ny, z0:z0 + nz])


def device_multiplier(pl, prec, m):
    """the rank's block of the multiplier as a device array in the plan's spectral layout"""
    esz = 16 if prec == "double" else 8
    t = torch.zeros(pl.getDomainSize() // esz, dtype=CDT[prec], device="cuda")
    pl.spectrumView(t).copy_(torch.from_numpy(spectrum_block(pl, m).astype(NPDT[prec])).cuda())
    return t


def device_tables(pl, prec, tables):
    (_, ny, nz), (_, y0, z0) = pl.getOutSize(), pl.getOutStart()
    ax, ay, az = tables
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v).astype(NPR[prec])).cuda()      # noqa: E731
    return dev(ax), dev(ay[y0:y0 + ny]), dev(az[z0:z0 + nz])


def op_args(plans, prec, m=None, tables=None, reciprocal=False, scale=1.0):
    """per rank: the multiplier arguments of execSpectralOp, the array or the tables in device buffers of their own"""
    if m is not None:
        return [dict(multiplier=device_multiplier(pl, prec, m), scale=scale) for pl in plans]
    return [dict(tables=device_tables(pl, prec, tables), reciprocal=reciprocal, scale=scale) for pl in plans]


def guarded_op_args(arena, plans, prec, m=None, tables=None, reciprocal=False, scale=1.0):
    """op_args with the array or the tables in guarded input buffers of the arena: a table read outside its entries meets a NaN"""
    args = []
    for r, pl in enumerate(plans):
        if m is not None:
            t = torch.zeros(pl.getDomainSize() // (16 if prec == "double" else 8), dtype=CDT[prec])
            pl.spectrumView(t).copy_(torch.from_numpy(spectrum_block(pl, m).astype(NPDT[prec])))
            args.append(dict(multiplier=arena.input(t.numpy(), f"mult[{r}]"), scale=scale))
        else:
            (_, ny, nz), (_, y0, z0) = pl.getOutSize(), pl.getOutStart()
            ax, ay, az = tables
            dev = [arena.input(np.asarray(v).astype(NPR[prec]), f"{n}[{r}]") for n, v in (("ax", ax), ("ay", ay[y0:y0 + ny]), ("az", az[z0:z0 + nz]))]
            args.append(dict(tables=tuple(dev), reciprocal=reciprocal, scale=scale))
    return args


def run_op(plans, prec, c2c, u, m=None, tables=None, reciprocal=False, scale=1.0, args=None, arena=None):
    """execSpectralOp on every rank (one host thread each); returns the ranks' output blocks.  `in` must come back bit for bit.
    `args`: what op_args made earlier (the caller keeps the device buffers).  arena (tests/guarded.py; the plans from make_plans with
    the same arena): `in`, `out` and the multiplier come from it at the first call and are used again at every later one, `out` and
    the work areas are refilled before the exec, the guards and every input are checked after it"""
    P = len(plans)
    dt = NPDT[prec] if c2c else NPR[prec]
    if arena is not None:
        def setup():
            ins = [arena.input(in_block(pl, u).astype(dt), f"in[{r}]") for r, pl in enumerate(plans)]
            outs = [arena.buffer(t.numel() * t.element_size(), t.dtype, name=f"out[{r}]").reshape(t.shape) for r, t in enumerate(ins)]
            return ins, outs, guarded_op_args(arena, plans, prec, m, tables, reciprocal, scale)
        ins, outs, args = arena.once("run_op", setup)
        arena.refill()
    else:
        ins = [torch.from_numpy(in_block(pl, u).astype(dt)).cuda() for pl in plans]
        outs = [torch.full_like(t, float("nan")) for t in ins]
    before = [t.cpu().numpy().tobytes() for t in ins]
    if args is None:
        args = op_args(plans, prec, m, tables, reciprocal, scale)
    torch.cuda.synchronize()
    with ThreadPoolExecutor(P) as ex:
        list(ex.map(lambda r: plans[r].execSpectralOp(outs[r], ins[r], **args[r]), range(P)))
    torch.cuda.synchronize()
    for r in range(P):
        assert ins[r].cpu().numpy().tobytes() == before[r], f"rank {r}: execSpectralOp modified its input"
    if arena is not None:
        arena.check_guards("execSpectralOp")
        arena.check_inputs("execSpectralOp")
    return [t.cpu().numpy() for t in outs]


@functools.lru_cache(maxsize=None)
def reference(shape, prec, c2c):
    """(u, m, want): zero-mean input and a multiplier with |m| <= 1 -- the transform of a seeded random real-space kernel, so Hermitian-
    consistent -- both rounded to the plan's precision, and numpy's float64 answer.  Computed once per (shape, precision, kind)."""
    rng = np.random.default_rng(20261017)
    n = float(np.prod(shape))
    kernel = rng.standard_normal(shape)
    if c2c:
        u = (rng.uniform(0, 255, shape) - CENTER) + 1j * (rng.uniform(0, 255, shape) - CENTER)
        u = u.astype(NPDT[prec]).astype(np.complex128)
        m = np.fft.fftn(kernel)
        m = (m / np.abs(m).max()).astype(NPDT[prec]).astype(np.complex128)
        want = np.fft.ifftn(np.fft.fftn(u) * m) * n
    else:
        u = (rng.uniform(0, 255, shape) - CENTER).astype(NPR[prec]).astype(np.float64)
        m = np.fft.rfftn(kernel)
        m = (m / np.abs(m).max()).astype(NPDT[prec]).astype(np.complex128)
        want = np.fft.irfftn(np.fft.rfftn(u) * m, s=shape, axes=(0, 1, 2)) * n
    for a in (u, m, want):
        a.setflags(write=False)
    return u, m, want


def check(plans, outs, want, prec, what):
    """every rank's block against its block of `want`, each entry held to the rms of the whole result; the worst rank's value goes to
    the table (parity_metric.record, DFFT_PARITY_TABLE=<file>) under the running test's id, before anything is asserted"""
    n = int(np.prod(want.shape))
    want_rms, bound = rms(want), 2 * forward_bound(prec, n)
    refs = [in_block(pl, want) for pl in plans]
    vals = [rms_rel(outs[r], refs[r], want_rms) if np.isfinite(outs[r]).all() else float("inf") for r in range(len(plans))]
    record(os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0].split("::")[-1] + " " + what, prec, n, max(vals), bound)
    for r, v in enumerate(vals):
        assert not np.isnan(outs[r]).any(), f"{what} rank {r}: NaN in the output (a part that was not written, or a product with inf)"
        assert np.isfinite(outs[r]).all(), f"{what} rank {r}: inf in the output"
        assert v <= bound, f"{what} rank {r}: per-entry error {v:.3e} > {bound:.1e}; " + worst_entry(outs[r], refs[r], want_rms)


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("P1,P2", GRIDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_array_multiplier_against_numpy(shape, P1, P2, c2c, prec):
    u, m, want = reference(shape, prec, c2c)
    for layout in (0, 1):
        plans = make_plans(shape, P1, P2, prec, c2c, layout)
        check(plans, run_op(plans, prec, c2c, u, m=m), want, prec, f"layout {layout}")


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("layout", [0, 1])
def test_ragged_tiles(layout, prec):
    """R2C on (64, 24, 38) over 2 x 3: Nzc = 20 -> 7 + 7 + 6 lines per ky row, no tile is full"""
    shape = (64, 24, 38)
    u, m, want = reference(shape, prec, False)
    plans = make_plans(shape, 2, 3, prec, False, layout)
    check(plans, run_op(plans, prec, False, u, m=m), want, prec, "2 x 3")


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("chunks", [1, 3])
def test_pipeline_depths(chunks, prec):
    shape = (64, 24, 20)
    for c2c in (True, False):
        u, m, want = reference(shape, prec, c2c)
        plans = make_plans(shape, 2, 2, prec, c2c, 0, chunks=chunks)
        assert plans[0].getPipelineChunks() == chunks and plans[0].debugChain(dfft.SPECTRAL_OP)[2]["launches"] == chunks
        check(plans, run_op(plans, prec, c2c, u, m=m), want, prec, f"depth {chunks} c2c={c2c}")


def wavenumbers(n, half=False):
    """the reference's derivativeCoefficients (random_dist_3D.cu:98-121): k below n/2, n - k above, 0 at n/2; the Hermitian axis holds
    k = 0 .. n/2 only"""
    k = np.arange(n // 2 + 1 if half else n, dtype=np.float64)
    return np.where(k < n // 2, k, 0.0 if half else np.where(k > n // 2, n - k, 0.0))


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("shape,P1,P2", [((32, 32, 32), 1, 1), ((32, 32, 32), 2, 4), ((64, 32, 16), 2, 2)])
def test_testcase4_in_one_call(shape, P1, P2, layout):
    """the reference's testcase 4 -- u = sin sin sin, spectrum times -(k1^2 + k2^2 + k3^2) / sqrt(n), unnormalised inverse -- as ONE call:
    tables ax = -kx^2, ay = -ky^2, az = -kz^2, held to the bound of test_testcase4_laplacian_through_the_strides against the same closed
    form.  sqrt(n) is the reference's own: sqrtf of the int product (oracle.testcase4_root), which is what testcase4_expected divides by."""
    Nx, Ny, Nz = shape
    x, y, z = np.meshgrid(np.arange(Nx), np.arange(Ny), np.arange(Nz), indexing="ij")
    u = np.sin(2 * np.pi * x / Nx) * np.sin(2 * np.pi * y / Ny) * np.sin(2 * np.pi * z / Nz)
    tables = (-wavenumbers(Nx) ** 2, -wavenumbers(Ny) ** 2, -wavenumbers(Nz, half=True) ** 2)
    plans = make_plans(shape, P1, P2, "double", False, layout)
    outs = run_op(plans, "double", False, u, tables=tables, scale=1.0 / orc.testcase4_root(shape))
    n3 = float(Nx * Ny * Nz)
    for r, pl in enumerate(plans):
        assert np.max(np.abs(outs[r] - orc.testcase4_expected(shape, in_block(pl, u)))) < 1e-9 * np.sqrt(n3)


def laplacian_tables(shape, c2c):
    k = lambda n: np.minimum(np.arange(n), n - np.arange(n)).astype(np.float64)      # noqa: E731  (|k|, n/2 at the Nyquist point)
    Nx, Ny, Nz = shape
    return -k(Nx) ** 2, -k(Ny) ** 2, -(k(Nz) if c2c else np.arange(Nz // 2 + 1, dtype=np.float64)) ** 2


# Shapes: dividing by |k|^2 gives back at low k what the rounding of the Laplacian (eps * its own size, which the highest k set) left
# there, so the round trip is good to eps * rms(|k|^2), whatever code runs it: 6e-8 * ~100 on the small grids (TOL_RT is 5e-5 at fp32),
# 1e-16 * ~1e5 on 1024 points at fp64 (TOL_RT 1e-10).  1024 points at fp32 would be 7e-3 by that arithmetic and is not a case.
POISSON = [((16, 8, 16), 1, 1, "double"), ((16, 8, 16), 1, 1, "float"), ((16, 8, 16), 2, 2, "double"), ((16, 8, 16), 2, 2, "float"),
           ((32, 8, 8), 2, 1, "double"), ((32, 8, 8), 2, 1, "float"), ((1024, 8, 8), 1, 2, "double")]


@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("shape,P1,P2,prec", POISSON)
def test_laplacian_then_poisson_returns_the_field(shape, P1, P2, c2c, prec):
    """table form (-|k|^2, normalised), then its reciprocal on the result: the field comes back, without its mean -- the one entry whose
    table sum is 0 is multiplied by 0, not by 1/0"""
    u, _, _ = reference(shape, prec, c2c)
    n = float(np.prod(shape))
    tables = laplacian_tables(shape, c2c)
    plans = make_plans(shape, P1, P2, prec, c2c, 0)
    lap = run_op(plans, prec, c2c, u, tables=tables, scale=1.0 / n)
    full = np.zeros(shape, dtype=np.complex128 if c2c else np.float64)
    for r, pl in enumerate(plans):
        (nx, ny, nz), (x0, y0, z0) = pl.getInSize(), pl.getInStart()
        full[x0:x0 + nx, y0:y0 + ny, z0:z0 + nz] = lap[r]
    spec = np.fft.fftn(u) if c2c else np.fft.rfftn(u)
    kx, ky, kz = np.meshgrid(*tables, indexing="ij")
    want_lap = np.fft.ifftn(spec * (kx + ky + kz)) if c2c else np.fft.irfftn(spec * (kx + ky + kz), s=shape, axes=(0, 1, 2))
    assert rel(full, want_lap) < TOL_RT[prec]
    back = run_op(plans, prec, c2c, full, tables=tables, reciprocal=True, scale=1.0 / n)
    for r, pl in enumerate(plans):
        assert rel(back[r], in_block(pl, u - u.mean())) < TOL_RT[prec]
    # a constant field has nothing but the entry with the zero sum: every output is exactly 0 (with 1/0 there it would be inf or NaN)
    const = run_op(plans, prec, c2c, np.full(shape, 3.0, dtype=full.dtype), tables=tables, reciprocal=True, scale=1.0 / n)
    for r in range(len(plans)):
        assert np.all(const[r] == 0), f"rank {r}: the entry with a zero table sum was not zeroed"


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("shape,P1,P2,layout", [((64, 24, 20), 2, 2, 0), ((64, 24, 20), 2, 2, 1), ((1024, 8, 8), 1, 1, 0), ((2048, 8, 16), 1, 2, 1)])
def test_agrees_with_the_unfused_path(shape, P1, P2, layout, prec):
    """same plans, input and multiplier: execR2C -> multiply on spectrumView -> execC2R against the fused call (not bit for bit: the fused
    x pass runs the default configuration of its length in both directions)"""
    u, m, want = reference(shape, prec, False)
    plans = make_plans(shape, P1, P2, prec, False, layout)
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


def test_argument_errors():
    pl = make_plans((16, 8, 16), 1, 1, "double", False, 0)[0]
    a = torch.zeros(16 * 8 * 16, dtype=RDT["double"], device="cuda")
    b = torch.zeros_like(a)
    m = torch.zeros(pl.getDomainSize() // 16, dtype=CDT["double"], device="cuda")
    with pytest.raises(dfft.DfftError, match="error 2.*out == in"):      # ERR_ARG: in place is not supported
        pl.execSpectralOp(a, a, multiplier=m)
    with pytest.raises(dfft.DfftError):
        pl.execSpectralOp(b, a)
    off = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), None, precision="double")
    off.initFFT(dfft.GlobalSize(16, 8, 16), dfft.Pencil_Partition(1, 1), True)
    with pytest.raises(dfft.DfftError, match="error 3.*spectral_op"):    # ERR_STATE: the plan was initialised without the option
        off.execSpectralOp(b, a, multiplier=m)


# ---- table forms (kinds 1 and 2) against numpy: every x length the kernel is instantiated for ------------------------------------
TABLE_NX = [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048]
TABLE_ROWS = [((Nx, 12, 10), P1, P2, chunks) for Nx in TABLE_NX for P1, P2 in ((1, 1), (2, 2)) for chunks in (1, 3)]
TABLE_ROWS.append(((64, 12, 38), 2, 3, 3))      # R2C: Nzc = 20 -> 7 + 7 + 6 lines per ky row, no tile is full
TABLE_ROWS = [pytest.param(*row, id=f"{'x'.join(map(str, row[0]))}-{row[1]}x{row[2]}-chunks{row[3]}") for row in TABLE_ROWS]


@functools.lru_cache(maxsize=None)
def table_reference(shape, prec, c2c):
    """(u, tables, wants, zero_fraction, rhos): the zero-mean input of reference(); integer tables drawn from -3 .. 3 -- neighbouring
    entries differ by whole numbers, and nothing makes t[k] = t[n - k]; numpy's float64 answers for kind 1 (m = sum / 9, |m| <= 1) and
    kind 2 (m = 1 / sum, 0 at a zero sum; nonzero sums are integers, so |m| <= 1 and the reciprocal is one rounding); the share of the
    spectrum with a zero sum and rho = rms(m * U) / rms(U) of either kind.
    C2C takes the tables as drawn.  R2C folds ax and ay to t[min(k, n - k)]: only then is m * U the spectrum of a real field and irfftn
    a valid reference -- so catching a table read at the reflected index is the C2C rows' job."""
    Nx, Ny, Nz = shape
    u = reference(shape, prec, c2c)[0]
    rng = np.random.default_rng(20261018 + Nx)
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


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("shape,P1,P2,chunks", TABLE_ROWS)
def test_table_multiplier_against_numpy(shape, P1, P2, chunks, c2c, prec):
    """tables=(ax, ay, az), kind 1 (scale = 1/9) and kind 2 (reciprocal, scale = 1) against table_reference(), both spectral layouts,
    held to the bound of the array form: |m| <= 1 in either kind.  What the tables are there to catch: tx read at another index than
    t2 + NT * sigma(c); ay without the first ky row of the pipeline chunk (Launch::ty_off -- the rows with depth 3; the depth is
    asserted from the chain); ay and az swapped or taken at the global instead of the rank's index; a zero sum that is not lane 0 of
    tile 0 (4.9 % .. 13.5 % of the spectrum).  R2C cannot see a table read at the reflected index (table_reference): C2C does.
    The asserts on the reference keep a case from passing for want of anything to check."""
    u, tables, wants, zero_fraction, rhos = table_reference(shape, prec, c2c)
    assert zero_fraction >= 0.04, f"only {zero_fraction:.3f} of the spectrum has a zero table sum"
    assert min(rhos) >= 0.3, f"rms(m U) / rms(U) = {rhos}: the multiplier leaves too little of the spectrum"
    for layout in (0, 1):
        plans = make_plans(shape, P1, P2, prec, c2c, layout, chunks=chunks)
        depth = plans[0].getPipelineChunks()
        if min(min(pl.getInSize()[0], pl.getOutSize()[1]) for pl in plans) >= chunks:      # every rank has that many x and ky rows
            assert depth == chunks
        assert all(pl.debugChain(S)[2]["group"] == "xx" and pl.debugChain(S)[2]["launches"] == depth for pl in plans)
        for kind in (1, 2):
            want = wants[kind - 1]
            assert all(np.any(in_block(pl, want) != 0) for pl in plans), "a rank's expected block is all zeros"
            outs = run_op(plans, prec, c2c, u, tables=tables, reciprocal=kind == 2, scale=1.0 / 9.0 if kind == 1 else 1.0)
            check(plans, outs, want, prec, f"kind {kind} layout {layout} depth {depth}")


# ---- one plan, several multipliers ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def second_multiplier(shape, prec, c2c):
    """another multiplier than reference()'s with |m| <= 1, and numpy's answer for 0.5 * m"""
    u = reference(shape, prec, c2c)[0]
    kernel = np.random.default_rng(20261019).standard_normal(shape)
    n = float(np.prod(shape))
    if c2c:
        m = np.fft.fftn(kernel)
        m = (m / np.abs(m).max()).astype(NPDT[prec]).astype(np.complex128)
        want = np.fft.ifftn(np.fft.fftn(u) * (0.5 * m)) * n
    else:
        m = np.fft.rfftn(kernel)
        m = (m / np.abs(m).max()).astype(NPDT[prec]).astype(np.complex128)
        want = np.fft.irfftn(np.fft.rfftn(u) * (0.5 * m), s=shape, axes=(0, 1, 2)) * n
    m.setflags(write=False)
    want.setflags(write=False)
    return m, want


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 2)])
def test_two_multipliers_on_one_plan(P1, P2, c2c, prec):
    """the operator is an argument of the call, not of the plan: two arrays in two device buffers that both stay allocated (the second
    with scale = 0.5), then the tables, then the first array again -- every call against its own numpy answer"""
    shape = (64, 12, 10)
    u, m1, want1 = reference(shape, prec, c2c)
    m2, want2 = second_multiplier(shape, prec, c2c)
    _, tables, table_wants, _, _ = table_reference(shape, prec, c2c)
    assert rms(want1 - want2) > 0.1 * rms(want1)      # (an answer to the other call's multiplier is nowhere near the bound)
    plans = make_plans(shape, P1, P2, prec, c2c, 0)
    a1, a2 = op_args(plans, prec, m=m1), op_args(plans, prec, m=m2, scale=0.5)
    assert all(x["multiplier"].data_ptr() != y["multiplier"].data_ptr() for x, y in zip(a1, a2))
    check(plans, run_op(plans, prec, c2c, u, args=a1), want1, prec, "first array")
    check(plans, run_op(plans, prec, c2c, u, args=a2), want2, prec, "second array, scale 0.5")
    check(plans, run_op(plans, prec, c2c, u, tables=tables, scale=1.0 / 9.0), table_wants[0], prec, "tables after the arrays")
    check(plans, run_op(plans, prec, c2c, u, args=a1), want1, prec, "first array again")


# ---- slab plans -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("P", [2, 3])
def test_slab_opt1_against_numpy(P, c2c, prec):
    """MPIcuFFT_Slab_Opt1 (input split along x, spectrum along ky; one exchange): array and table forms, both layouts; P = 3 splits
    the 64 x rows 22 + 21 + 21"""
    shape = (64, 12, 10)
    u, m, want = reference(shape, prec, c2c)
    _, tables, table_wants, _, _ = table_reference(shape, prec, c2c)
    for layout in (0, 1):
        plans = make_plans(shape, P, 1, prec, c2c, layout, cls=dfft.MPIcuFFT_Slab_Opt1)
        assert sorted(pl.getInStart()[0] for pl in plans)[1] > 0 and all(pl.getInSize()[1:] == shape[1:] for pl in plans)
        check(plans, run_op(plans, prec, c2c, u, m=m), want, prec, f"slab P={P} layout {layout} array")
        check(plans, run_op(plans, prec, c2c, u, tables=tables, scale=1.0 / 9.0), table_wants[0], prec, f"slab P={P} layout {layout} tables")
        check(plans, run_op(plans, prec, c2c, u, tables=tables, reciprocal=True), table_wants[1], prec, f"slab P={P} layout {layout} reciprocal")


# ---- options that change the schedule, not the launches ---------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 2)])
def test_compute_streams_and_graph_change_no_bit(P1, P2, c2c, prec):
    """compute_streams = 2 (odd chunks on a second stream: asserted from the trace of what the exec issued) and, on one rank, graph = 1
    run the same launches on the same data as the plain plan: the outputs are identical bit for bit, and the plain one meets the bound"""
    shape = (64, 24, 20)
    u, m, want = reference(shape, prec, c2c)
    results = {}
    rows = [("cs1", {"compute_streams": 1, "trace": 1}), ("cs2", {"compute_streams": 2, "trace": 1})]
    if P1 * P2 == 1:
        rows += [("graph0", {"graph": 0}), ("graph1", {"graph": 1})]
    for name, options in rows:
        plans = make_plans(shape, P1, P2, prec, c2c, 0, chunks=3, options=options)
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
