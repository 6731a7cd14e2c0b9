"""The factor-table forms of execSpectralOp (factors=(cx, cy, cz); kinds 3, 4, 5 of dfft_exec_spectral_op, fft_spectral_kernel<Cfg, 2>):
m = scale * P, scale * P * s, scale * P / s (0 at s = 0) with P = cx[kx] * cy[ky] * cz[kz] from complex tables and s = ax[kx] + ay[ky] + az[kz]
from real ones, all local to the rank's spectrum block.

Reference: numpy in float64, ifftn(fftn(u) * m) * n resp. irfftn(rfftn(u) * m) * n, with u and the tables rounded to the plan's precision
first.  Metric and bound are those of tests/test_gpu_spectral_op.py: rms_rel(got, want) <= 2 * forward_bound(prec, n) per rank block (check()
there: two transforms, each held to the per-entry forward bound; the metric is relative to rms(want), so the size of m does not enter), every
value recorded through parity_metric.record.  The factor values {+-1, +-i, +-1 +-i} and the integer sums are exact in either precision: their
products cost the kernel two roundings per point next to the two chains' log2(n) each.  The host emulation of the kernel's arithmetic is
tests/test_cpu_spectral_factors.py."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import distributedfft_amd as dfft  # noqa: E402
from distributedfft_amd._lib import SpectralOp, check as check_rc, lib  # noqa: E402

from parity_metric import forward_bound, record, rms, rms_rel  # noqa: E402
from test_gpu_parity import CDT, NPDT, NPR  # noqa: E402
from test_gpu_spectral_op import check, device_multiplier, device_tables, in_block, make_plans, reference, run_op  # noqa: E402

S = dfft.SPECTRAL_OP
SCALE = 0.25
EIGHT = np.array([1, -1, 1j, -1j, 1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j])


def device_factors(pl, prec, factors):
    """the rank's slices of (cx, cy, cz) as complex device tables of the plan's precision; None stays None"""
    (_, ny, nz), (_, y0, z0) = pl.getOutSize(), pl.getOutStart()
    cx, cy, cz = factors
    dev = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v).astype(NPDT[prec])).cuda()      # noqa: E731
    return dev(cx), dev(None if cy is None else cy[y0:y0 + ny]), dev(None if cz is None else cz[z0:z0 + nz])


def factor_args(plans, prec, factors, tables=None, reciprocal=False, scale=1.0):
    """per rank: the arguments of execSpectralOp for the factor forms, every table in a device buffer of its own"""
    return [dict(factors=device_factors(pl, prec, factors), scale=scale, **({} if tables is None else
                 dict(tables=device_tables(pl, prec, tables), reciprocal=reciprocal))) for pl in plans]


# ---- 1. every x length, ragged tiles, ky chunks that do not start at row 0 ----------------------------------------------------------
FACTOR_NX = [2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048]
FACTOR_ROWS = [((Nx, 12, 10), P1, P2, chunks) for Nx in FACTOR_NX for P1, P2, chunks in ((1, 1, 1), (2, 2, 3))]
FACTOR_ROWS.append(((64, 12, 38), 2, 3, 3))      # R2C: Nzc = 20 -> 7 + 7 + 6 lines per ky row, no tile is full
FACTOR_ROWS = [pytest.param(*row, id=f"{'x'.join(map(str, row[0]))}-{row[1]}x{row[2]}-chunks{row[3]}") for row in FACTOR_ROWS]


def hermitian(t):
    """t[n - k] = conj(t[k]), the self-conjugate entries (k = 0 and k = n / 2) real: the part of the value that is not zero"""
    t = t.copy()
    n = t.size
    for k in range(n // 2 + 1):
        if (n - k) % n == k:
            t[k] = t[k].real if t[k].real != 0 else t[k].imag
        else:
            t[n - k] = np.conj(t[k])
    return t


@functools.lru_cache(maxsize=None)
def factor_reference(shape, prec, c2c):
    """(u, factors, tables, wants, stats): the zero-mean input of test_gpu_spectral_op.reference(); cx, cy, cz uniform over the eight values
    {+-1, +-i, +-1 +-i} and ax, ay, az integers in -3 .. 3; numpy's float64 answers for kinds 3, 4, 5 at scale 0.25; per kind
    rho = rms(m U) / rms(U) and the share of m with a nonzero imaginary part, and the share of the spectrum with a zero sum.
    C2C takes the tables as drawn: nothing makes t[k] and t[n - k] alike, so a conjugated table or one read at the reflected index gives
    another answer.  R2C makes each complex table Hermitian (cz: the first Nz / 2 + 1 entries of a Hermitian table, i.e. real at kz = 0 and
    at the Nyquist point) and folds the real ones as the table test of test_gpu_spectral_op.py does: only then is m U the spectrum of a real
    field and irfftn a valid reference (asserted: rfftn of the answer is m U)."""
    Nx, Ny, Nz = shape
    u = reference(shape, prec, c2c)[0]
    rng = np.random.default_rng(20261019 + Nx)
    cx, cy, cz = (EIGHT[rng.integers(0, 8, n)] for n in (Nx, Ny, Nz))
    ax, ay, az = (rng.integers(-3, 4, n).astype(np.float64) for n in (Nx, Ny, Nz))
    if not c2c:
        fold = lambda t: t[np.minimum(np.arange(t.size), (t.size - np.arange(t.size)) % t.size)]      # noqa: E731
        cx, cy, cz = hermitian(cx), hermitian(cy), hermitian(cz)[:Nz // 2 + 1]
        ax, ay, az = fold(ax), fold(ay), az[:Nz // 2 + 1]
    P = cx[:, None, None] * cy[None, :, None] * cz[None, None, :]
    s = ax[:, None, None] + ay[None, :, None] + az[None, None, :]
    n = float(np.prod(shape))
    U = np.fft.fftn(u) if c2c else np.fft.rfftn(u)
    back = (lambda X: np.fft.ifftn(X) * n) if c2c else (lambda X: np.fft.irfftn(X, s=shape, axes=(0, 1, 2)) * n)
    ms = (SCALE * P, SCALE * P * s, np.where(s != 0, SCALE * P / np.where(s != 0, s, 1.0), 0.0))
    wants = tuple(back(U * m) for m in ms)
    if not c2c:
        for m, want in zip(ms, wants):
            assert rms(np.fft.rfftn(want) / n - U * m) <= 1e-12 * rms(U * m), "m U is not the spectrum of a real field"
    stats = dict(rho=tuple(rms(m * U) / rms(U) for m in ms), imag=tuple(float(np.mean(m.imag != 0)) for m in ms), zero=float(np.mean(s == 0)))
    for a in (cx, cy, cz, ax, ay, az) + wants:
        a.setflags(write=False)
    return u, (cx, cy, cz), (ax, ay, az), wants, stats


def assert_reference_has_something_to_check(stats):
    """on the reference alone, before anything runs on the GPU"""
    rho, imag, zero = stats["rho"], stats["imag"], stats["zero"]
    assert rho[0] >= 0.25, f"kind 3: rms(m U) / rms(U) = {rho[0]:.3f}"
    assert rho[1] >= 0.1 and rho[2] >= 0.1, f"kinds 4, 5: rms(m U) / rms(U) = {rho[1]:.3f}, {rho[2]:.3f}"
    assert zero >= 0.01, f"only {zero:.4f} of the spectrum has a zero sum"
    assert min(imag) >= 0.5, f"only {imag} of m has a nonzero imaginary part"


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("shape,P1,P2,chunks", FACTOR_ROWS)
def test_factor_tables_against_numpy(shape, P1, P2, chunks, c2c, prec):
    """factors=(cx, cy, cz) alone (kind 3), with tables (kind 4) and with their reciprocal (kind 5), scale 0.25, both spectral layouts, every
    x length the kernel is instantiated for.  What the rows are there to catch: cx read at another index than t2 + NT * sigma(c); cy without
    the first ky row of the pipeline chunk, or moved by real instead of complex elements (Launch::ty_off -- the rows with depth 3; the depth is
    asserted from the chain); cy and cz swapped or taken at the global instead of the rank's index; a table conjugated or read at the
    reflected index (the C2C rows); the sum of kinds 4 and 5 and its zeros."""
    u, factors, tables, wants, stats = factor_reference(shape, prec, c2c)
    assert_reference_has_something_to_check(stats)
    for layout in (0, 1):
        plans = make_plans(shape, P1, P2, prec, c2c, layout, chunks=chunks)
        depth = plans[0].getPipelineChunks()
        if min(min(pl.getInSize()[0], pl.getOutSize()[1]) for pl in plans) >= chunks:      # every rank has that many x and ky rows
            assert depth == chunks
        assert all(pl.debugChain(S)[2]["group"] == "xx" and pl.debugChain(S)[2]["launches"] == depth for pl in plans)
        for kind in (3, 4, 5):
            want = wants[kind - 3]
            assert all(np.any(in_block(pl, want) != 0) for pl in plans), "a rank's expected block is all zeros"
            args = factor_args(plans, prec, factors, tables if kind > 3 else None, reciprocal=kind == 5, scale=SCALE)
            check(plans, run_op(plans, prec, c2c, u, args=args), want, prec, f"kind {kind} layout {layout} depth {depth}")


# ---- 2. null tables, wavenumbers(), and the operator the form is for -----------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 2)])
def test_null_factors_and_gradient_of_a_poisson_solution(P1, P2, c2c, prec):
    """component d of grad(laplace^-1 u): kind 5 with the d-th factor table i * k_d and the other two None, sums -(kx^2 + ky^2 + kz^2), every
    table built from the plan's own wavenumbers(); numpy's answer from np.fft.fftfreq on the global grid.  |m| = |k_d| / |k|^2 <= 1.  R2C:
    i * k at the Nyquist point is not Hermitian-consistent and is zeroed, as every spectral derivative of a real field does."""
    shape = (16, 12, 10)
    n = float(np.prod(shape))
    u = reference(shape, prec, c2c)[0]
    gk = [np.round(np.fft.fftfreq(m) * m) for m in shape]
    if not c2c:
        gk[2] = np.arange(shape[2] // 2 + 1, dtype=np.float64)
    nyquist = [np.abs(k) * 2 == m for k, m in zip(gk, shape)]
    s = -(gk[0][:, None, None] ** 2 + gk[1][None, :, None] ** 2 + gk[2][None, None, :] ** 2)
    U = np.fft.fftn(u) if c2c else np.fft.rfftn(u)
    plans = make_plans(shape, P1, P2, prec, c2c, 0)
    dev = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v).astype(dt)).cuda()      # noqa: E731
    for d in range(3):
        kd = np.where(nyquist[d], 0.0, gk[d]) if not c2c else gk[d]
        m = 1j * kd.reshape([-1 if a == d else 1 for a in range(3)]) * np.where(s != 0, 1.0 / np.where(s != 0, s, 1.0), 0.0)
        want = np.fft.ifftn(U * m) if c2c else np.fft.irfftn(U * m, s=shape, axes=(0, 1, 2))
        args = []
        for pl in plans:
            k = pl.wavenumbers()
            kl = k[d].astype(np.float64)
            if not c2c:
                kl = np.where(np.abs(kl) * 2 == shape[d], 0.0, kl)
            factors = [None, None, None]
            factors[d] = dev(1j * kl, NPDT[prec])
            args.append(dict(factors=tuple(factors), tables=tuple(dev(-(t.astype(np.float64) ** 2), NPR[prec]) for t in k),
                             reciprocal=True, scale=1.0 / n))
        check(plans, run_op(plans, prec, c2c, u, args=args), want, prec, f"d/d{'xyz'[d]} of the Poisson solution")


# ---- 3. the same multiplier as tables and as an array ---------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
def test_kind_3_against_kind_0(c2c, prec):
    """one plan: kind 3 with the tables, kind 0 with the array scale * P assembled from the same tables -- both held to numpy; their difference
    is recorded (not bit for bit: the array form multiplies by one rounded product, the factor form by the factors)"""
    shape = (64, 12, 10)
    u, factors, _, wants, _ = factor_reference(shape, prec, c2c)
    cx, cy, cz = factors
    P = cx[:, None, None] * cy[None, :, None] * cz[None, None, :]
    plans = make_plans(shape, 2, 2, prec, c2c, 0)
    by_tables = run_op(plans, prec, c2c, u, args=factor_args(plans, prec, factors, scale=SCALE))
    check(plans, by_tables, wants[0], prec, "kind 3")
    by_array = run_op(plans, prec, c2c, u, args=[dict(multiplier=device_multiplier(pl, prec, P), scale=SCALE) for pl in plans])
    check(plans, by_array, wants[0], prec, "kind 0")
    n, want_rms = int(np.prod(shape)), rms(wants[0])
    diff = max(rms_rel(a, b, want_rms) for a, b in zip(by_tables, by_array))
    record("test_kind_3_against_kind_0 kind 3 - kind 0", prec, n, diff, 4 * forward_bound(prec, n))
    assert diff <= 4 * forward_bound(prec, n)      # (each is within 2 * forward_bound of numpy)


# ---- 4. a caller compiled against the six-field struct --------------------------------------------------------------------------------
class OldSpectralOp(C.Structure):
    _fields_ = [("kind", C.c_int32), ("scale", C.c_double), ("mult", C.c_void_p), ("ax", C.c_void_p), ("ay", C.c_void_p), ("az", C.c_void_p)]


@pytest.mark.parametrize("prec", ["double", "float"])
def test_old_struct_layout(prec):
    """dfft_exec_spectral_op with kinds 1 and 2 in the struct as it was before cx, cy, cz were appended, followed in memory by bytes that are
    not zero: the library never reads past the six fields for these kinds, and the output is that of the call through the new struct"""
    shape = (16, 12, 10)
    u, _, tables, _, _ = factor_reference(shape, prec, True)
    pl = make_plans(shape, 1, 1, prec, True, 0)[0]
    ax, ay, az = device_tables(pl, prec, tables)
    d_in = torch.from_numpy(u.astype(NPDT[prec])).cuda()
    assert C.sizeof(OldSpectralOp) == 48 and C.sizeof(SpectralOp) == 72
    for kind in (1, 2):
        new = torch.full_like(d_in, float("nan"))
        pl.execSpectralOp(new, d_in, tables=(ax, ay, az), reciprocal=kind == 2, scale=SCALE)
        buf = (C.c_ubyte * 128)(*([0xAB] * 128))
        old = OldSpectralOp.from_buffer(buf)
        old.kind, old.scale, old.mult, old.ax, old.ay, old.az = kind, SCALE, None, ax.data_ptr(), ay.data_ptr(), az.data_ptr()
        assert bytes(buf)[48:] == b"\xab" * 80
        got = torch.full_like(d_in, float("nan"))
        torch.cuda.synchronize()
        rc = lib().dfft_exec_spectral_op(pl._h, C.c_void_p(got.data_ptr()), C.c_void_p(d_in.data_ptr()), C.cast(buf, C.POINTER(SpectralOp)))
        torch.cuda.synchronize()
        assert rc == 0, lib().dfft_last_error().decode()
        assert not torch.isnan(torch.view_as_real(got)).any()
        assert got.cpu().numpy().tobytes() == new.cpu().numpy().tobytes(), f"kind {kind}: the old struct layout gives another result"


# ---- 5. what the C layer refuses ------------------------------------------------------------------------------------------------------
def test_argument_errors_in_the_c_layer():
    shape = (16, 12, 10)
    pl = make_plans(shape, 1, 1, "double", True, 0)[0]
    a = torch.zeros(int(np.prod(shape)), dtype=CDT["double"], device="cuda")
    b = torch.full_like(a, 7.0)
    t = torch.ones(16, dtype=torch.float64, device="cuda")
    c = torch.ones(16, dtype=CDT["double"], device="cuda")
    p = lambda x: None if x is None else x.data_ptr()      # noqa: E731

    def call(kind, tables=(None, None, None), factors=(None, None, None)):
        op = SpectralOp(kind, 1.0, None, *map(p, tables), *map(p, factors))
        check_rc(lib().dfft_exec_spectral_op(pl._h, C.c_void_p(b.data_ptr()), C.c_void_p(a.data_ptr()), C.byref(op)))

    with pytest.raises(dfft.DfftError, match="error 2.*at least one of cx, cy, cz"):      # ERR_ARG
        call(3)
    with pytest.raises(dfft.DfftError, match="error 2.*at least one of cx, cy, cz"):
        call(5, tables=(t, t, t))
    with pytest.raises(dfft.DfftError, match="error 2.*all of ax, ay, az"):
        call(4, tables=(None, t, t), factors=(c, c, c))
    with pytest.raises(dfft.DfftError, match="error 2.*kind must be 0 .*5 "):
        call(6, tables=(t, t, t), factors=(c, c, c))
    with pytest.raises(dfft.DfftError, match="error 2.*kind must be"):
        call(-1)
    torch.cuda.synchronize()
    assert bool((b == 7.0).all()), "a refused call wrote to its output"
