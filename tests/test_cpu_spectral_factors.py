"""The factor-table forms of execSpectralOp (kinds 3, 4, 5 of dfft_exec_spectral_op: m = scale * cx * cy * cz, times or over the sum of the
real tables) without a GPU:
  * tests/cpp/spectral_factor_check.hip drives the kernel's own building blocks on the host, as tests/test_cpu_spectral_kernel.py does for the
    array and the real-table forms, with the hand-off done by spectral_factor_point / spectral_factor_line -- the functions
    fft_spectral_kernel<Cfg, 2> itself calls -- for every configuration, against N * ifft(fft(x) * m) in long double;
  * MPIcuFFT.wavenumbers() against np.fft.fftfreq on plans that allocate nothing;
  * the argument rules of execSpectralOp that Python enforces, and the struct every call that was valid before factors= existed builds;
  * the check of the kernel argument structs between libdfft_amd.so and libdfft_amd_any.so (csrc/any_loader.hip: dfft_any_abi).
A failure of tests/test_gpu_spectral_factors.py with the first test green points at the plan's table offsets (Launch::ty_off in complex
elements, the rank's slices of cy and cz) or at the null-table handling, not at the kernel's arithmetic."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import distributedfft_amd as dfft
from distributedfft_amd import api
from distributedfft_amd._lib import SpectralOp

import host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_factor_forms_emulated_on_the_host(tmp_path):
    for out in host_check.run(tmp_path, "spectral_factor_check.hip", (("f64", []), ("f32", ["-DCHAIN_F32"]))).values():
        assert "33 forms of 11 configurations checked, 0 failed" in out and "ALL OK" in out, out[-2000:]


# ---- wavenumbers() ------------------------------------------------------------------------------------------------------------------
def host_plans(shape, P1, P2, c2c):
    world = dfft.Comm.local(P1 * P2) if P1 * P2 > 1 else None
    plans = []
    for r in range(P1 * P2):
        pl = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), world, precision="double", rank=r)
        pl.initFFT(dfft.GlobalSize(*shape), dfft.Pencil_Partition(P1, P2), allocate=False, c2c=c2c)
        plans.append(pl)
    return plans


@pytest.mark.parametrize("c2c", [True, False], ids=["c2c", "r2c"])
@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 3)])
def test_wavenumbers_are_the_fftfreq_slices_of_the_block(P1, P2, c2c):
    shape = (16, 12, 14)
    Nx, Ny, Nz = shape
    gx, gy = (np.round(np.fft.fftfreq(n) * n).astype(np.int64) for n in (Nx, Ny))
    gz = np.round(np.fft.fftfreq(Nz) * Nz).astype(np.int64) if c2c else np.arange(Nz // 2 + 1, dtype=np.int64)
    plans = host_plans(shape, P1, P2, c2c)
    for pl in plans:
        kx, ky, kz = pl.wavenumbers()
        (nx, ny, nz), (_, y0, z0) = pl.getOutSize(), pl.getOutStart()
        assert all(isinstance(k, np.ndarray) and k.dtype == np.int64 for k in (kx, ky, kz))
        assert (kx.size, ky.size, kz.size) == (nx, ny, nz) and nx == Nx
        assert np.array_equal(kx, gx) and np.array_equal(ky, gy[y0:y0 + ny]) and np.array_equal(kz, gz[z0:z0 + nz])
    # rank = i * P2 + j: the spectrum's ky is split over i, its kz over j; the ranks' pieces in order are the global arrays
    assert np.array_equal(np.concatenate([plans[i * P2].wavenumbers()[1] for i in range(P1)]), gy)
    assert np.array_equal(np.concatenate([plans[j].wavenumbers()[2] for j in range(P2)]), gz)
    if P1 * P2 > 1:
        assert plans[-1].getOutStart()[1] > 0 and plans[-1].getOutStart()[2] > 0      # (a block that starts at neither origin)
        assert (plans[-1].wavenumbers()[1] < 0).all()                                 # (and lies in the wrapped half of ky)


# ---- what Python refuses, and what it builds --------------------------------------------------------------------------------------
class _Recorder:
    """stands in for the library: keeps the dfft_spectral_op the call was made with"""
    def __init__(self):
        self.ops = []

    def dfft_exec_spectral_op(self, handle, out, in_, op):
        self.ops.append(bytes(op._obj))
        return 0


@pytest.fixture
def recorded(monkeypatch):
    pl = host_plans((16, 12, 14), 1, 1, True)[0]
    rec = _Recorder()
    monkeypatch.setattr(api, "lib", lambda: rec)
    return pl, rec


def test_python_argument_errors(recorded):
    pl, rec = recorded
    t = (0x1000, 0x2000, 0x3000)
    with pytest.raises(dfft.DfftError, match="multiplier"):
        pl.execSpectralOp(1, 2, multiplier=0x100, factors=t)
    with pytest.raises(dfft.DfftError, match="multiplier"):
        pl.execSpectralOp(1, 2, multiplier=0x100, tables=t)
    with pytest.raises(dfft.DfftError, match="multiplier"):
        pl.execSpectralOp(1, 2)
    with pytest.raises(dfft.DfftError, match="reciprocal"):
        pl.execSpectralOp(1, 2, factors=t, reciprocal=True)
    with pytest.raises(dfft.DfftError, match="reciprocal"):
        pl.execSpectralOp(1, 2, multiplier=0x100, reciprocal=True)
    with pytest.raises(dfft.DfftError, match="at least one"):
        pl.execSpectralOp(1, 2, factors=(None, None, None))
    assert rec.ops == [], "a refused call reached the library"


def test_the_struct_each_form_builds(recorded):
    """kind and fields per form; the calls that were valid before factors= existed build the struct they built then -- the six old fields
    as before, the appended ones zero"""
    pl, rec = recorded
    a, c = (0x1000, 0x2000, 0x3000), (0x4000, None, 0x6000)

    def op(**kw):
        pl.execSpectralOp(1, 2, **kw)
        return SpectralOp.from_buffer_copy(rec.ops[-1])

    def fields(o):
        return (o.kind, o.scale, o.mult, o.ax, o.ay, o.az, o.cx, o.cy, o.cz)

    assert fields(op(multiplier=0x100, scale=0.5)) == (0, 0.5, 0x100, None, None, None, None, None, None)
    assert fields(op(tables=a)) == (1, 1.0, None, *a, None, None, None)
    assert fields(op(tables=a, reciprocal=True, scale=2.0)) == (2, 2.0, None, *a, None, None, None)
    assert fields(op(factors=c, scale=0.25)) == (3, 0.25, None, None, None, None, *c)
    assert fields(op(factors=c, tables=a)) == (4, 1.0, None, *a, *c)
    assert fields(op(factors=c, tables=a, reciprocal=True)) == (5, 1.0, None, *a, *c)
    # the old layout is a prefix of the new one
    old = [("kind", C.c_int32), ("scale", C.c_double), ("mult", C.c_void_p), ("ax", C.c_void_p), ("ay", C.c_void_p), ("az", C.c_void_p)]
    assert SpectralOp._fields_[:6] == old and [n for n, _ in SpectralOp._fields_[6:]] == ["cx", "cy", "cz"]
    assert C.sizeof(SpectralOp) == 48 + 24 and SpectralOp.cx.offset == 48


# ---- the seam between the two libraries -------------------------------------------------------------------------------------------
ANY_STUB = """
#include <stddef.h>
#define LAUNCH3(n) int n(int a, int b, const void *A, void *s) { return -1; }
#define LAUNCH2(n) int n(int a, const void *A, void *s) { return -1; }
#define INFO3(n) int n(int a, int b, void *pi) { return 0; }
#define INFO1(n) int n(int a) { return 0; }
LAUNCH3(dfft_any_launch_mixed_f64) LAUNCH3(dfft_any_launch_mixed_f32) INFO3(dfft_any_mixed_info_f64) INFO3(dfft_any_mixed_info_f32)
LAUNCH3(dfft_any_launch_rmixed_f64) LAUNCH3(dfft_any_launch_rmixed_f32) INFO1(dfft_any_rmixed_info_f64) INFO1(dfft_any_rmixed_info_f32)
LAUNCH2(dfft_any_launch_bluestein_f64) LAUNCH2(dfft_any_launch_bluestein_f32)
#ifdef WITH_ABI
void dfft_any_abi(size_t out[3]) { out[0] = SIZE_ARGS; out[1] = SIZE_INFO; out[2] = 999999; }
#endif
"""
INIT_12 = (
    "import distributedfft_amd as dfft\n"
    "pl = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations())\n"
    "try:\n"
    "    pl.initFFT(dfft.GlobalSize(12, 16, 16), dfft.Pencil_Partition(1, 1), allocate=False, c2c=True)\n"
    "    print('planned', pl.getDomainSize())\n"
    "except dfft.DfftError as e:\n"
    "    print('refused:', e)\n")


def init_in_a_child(any_library):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("DFFT_ANY_LIBRARY", None)
    if any_library:
        env["DFFT_ANY_LIBRARY"] = any_library
    out = subprocess.run([sys.executable, "-c", INIT_12], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def real_abi():
    lib = C.CDLL(os.path.join(ROOT, "distributedfft_amd", "libdfft_amd_any.so"))
    v = (C.c_size_t * 3)()
    lib.dfft_any_abi.restype = None
    lib.dfft_any_abi(v)
    return tuple(v)


@pytest.mark.parametrize("stub", ["wrong_abi", "no_abi_symbol"])
def test_a_second_library_of_another_struct_version_is_refused(tmp_path, stub):
    """an x length of 12 has no configuration in the core library: dfft_init opens the second one, which exports every launcher the core
    looks up but answers dfft_any_abi with another DFFT_PASS_ABI (the sizes are the real ones) -- or has no dfft_any_abi at all"""
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    args, info, abi = real_abi()
    (tmp_path / "stub.c").write_text(ANY_STUB)
    so = str(tmp_path / "libstub_any.so")
    defs = ["-DWITH_ABI", f"-DSIZE_ARGS={args}", f"-DSIZE_INFO={info}"] if stub == "wrong_abi" else []
    subprocess.check_call([gcc, "-shared", "-fPIC", *defs, str(tmp_path / "stub.c"), "-o", so])
    out = init_in_a_child(so)
    assert out.startswith("refused:") and "libdfft_amd_any.so" in out and so in out, out
    assert "make -C distributedfft_amd/csrc any" in out, out
    if stub == "wrong_abi":
        assert f"sizeof(PassArgs) {args}, sizeof(PassInfo) {info}, DFFT_PASS_ABI 999999" in out, out              # theirs
        assert f"this library: sizeof(PassArgs) {args}, sizeof(PassInfo) {info}, DFFT_PASS_ABI {abi}" in out, out   # ours
    else:
        assert "lacks the symbol dfft_any_abi" in out, out


def test_the_real_second_library_is_accepted():
    out = init_in_a_child(None)
    assert out.startswith("planned"), out
    assert real_abi()[2] >= 2
