"""Option "spectral_op" = 2 (include/dfft_c.h) without a GPU: execSpectralOp on mixed-radix x lengths.  Value 1 keeps its reach -- powers of
two -- and its messages; value 2 adds the mixed-radix lengths with a fused kernel (csrc/spectral_mixed.inc, kernels of libdfft_amd_any.so) and
nothing else: the chain, the xx descriptors, the extra work slice and the schedule are those of tests/test_cpu_spectral_op.py, whose layout
replay and schedule checker run here on x lengths such as 12, 60, 768 and 1000."""
import ctypes
import os
import re

import numpy as np
import pytest

import distributedfft_amd as dfft
import schedule_check as sc
from layout_sim import World
from schedule_check import LAUNCH
from test_cpu_spectral_op import GROUPS, SpectralFootprints, blocks, multiplier, run_spectral

F, I, S = dfft.FORWARD, dfft.INVERSE, dfft.SPECTRAL_OP
PENCIL, SLAB = dfft.MPIcuFFT_Pencil_Opt1, dfft.MPIcuFFT_Slab_Opt1
PRECISIONS = ["double", "float"]
# native mixed-radix lengths (csrc/kernels_mixed.inc) without a fused kernel: every configuration tried compiles with scratch
# (csrc/spectral_mixed.inc, profiles/spectral_mixed_resources.txt)
LEFT_OUT = {"double": set(), "float": {1920, 2000}}


def init(cls, shape, precision="double", P1=1, P2=1, value=2, **options):
    comm = dfft.Comm.local(P1 * P2) if P1 * P2 > 1 else None
    pl = cls(dfft.Configurations(), comm, precision=precision, rank=0)
    for k, v in dict(options, spectral_op=value).items():
        pl.setOption(k, v)
    pl.initFFT(dfft.GlobalSize(*shape), dfft.Partition(P1, P2), allocate=False)
    return pl


def accepted(nx, precision, value):
    try:
        init(PENCIL, (nx, 8, 8), precision, value=value)
        return True
    except dfft.DfftError as e:
        assert "error 4" in str(e) and str(nx) in str(e), e      # ERR_UNSUPPORTED, naming the length
        return False


def native_mixed_lengths(precision):
    inc = os.path.join(os.path.dirname(dfft.__file__), "csrc", "kernels_mixed.inc")
    tag = "F64" if precision == "double" else "F32"
    return sorted({int(n) for n in re.findall(rf"using {tag}_M(\d+) =", open(inc).read())})


@pytest.mark.parametrize("precision", PRECISIONS)
def test_init_accepts_exactly_what_supported_reports(precision):
    for nx in range(2, 2049):
        pow2 = nx & (nx - 1) == 0
        assert dfft.spectral_op_supported(nx, precision, 1) == pow2, nx
        assert accepted(nx, precision, 1) == pow2, nx
        assert accepted(nx, precision, 2) == dfft.spectral_op_supported(nx, precision, 2), nx
        if pow2:
            assert dfft.spectral_op_supported(nx, precision, 2), nx
    assert not dfft.spectral_op_supported(4096, precision, 2) and not dfft.spectral_op_supported(768, precision, 3)
    assert not dfft.spectral_op_supported(768, precision, 0)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_native_mixed_length_but_the_documented_ones(precision):
    native = native_mixed_lengths(precision)
    assert len(native) == (45 if precision == "double" else 49)
    left_out = {n for n in native if not dfft.spectral_op_supported(n, precision, 2)}
    print(f"{precision}: {len(native) - len(left_out)} of {len(native)} native mixed-radix lengths have a fused kernel; left out: {sorted(left_out)}")
    assert left_out == LEFT_OUT[precision]
    supported = {n for n in range(2, 2049) if n & (n - 1) and dfft.spectral_op_supported(n, precision, 2)}
    assert supported == set(native) - left_out      # and nothing that is not a native mixed-radix length


CASES = [pytest.param(cls, P1, P2, shape, c2c, layout, precision,
                      id=f"{cls.__name__[8:]}-{P1}x{P2}-{'x'.join(map(str, shape))}-{'c2c' if c2c else 'r2c'}-layout{layout}-{precision}")
         for shape, precision in (((12, 10, 14), "double"), ((60, 24, 20), "double"), ((60, 24, 20), "float"), ((768, 8, 8), "double"), ((1000, 8, 8), "float"))
         for cls, P1, P2 in ((PENCIL, 1, 1), (PENCIL, 2, 2), (PENCIL, 2, 3), (SLAB, 3, 1))
         for c2c in (True, False) for layout in (0, 1)
         if shape[0] < 100 or (c2c and layout == 0) or (not c2c and layout == 1)]      # the long lines: one kind per layout


@pytest.mark.parametrize("cls,P1,P2,shape,c2c,layout,precision", CASES)
def test_chain_data_flow_and_schedule(cls, P1, P2, shape, c2c, layout, precision):
    """debugPass("xx") exists, the chain has its five steps with xx third, the work area is the value-0 plan's plus one domain slice, the
    replay of the chain on NaN-filled slices gives numpy's answer, and the executor's trace passes the schedule checker"""
    rng = np.random.default_rng(11)
    u = rng.uniform(0, 255, shape) - 127.5
    if c2c:
        u = u + 1j * (rng.uniform(0, 255, shape) - 127.5)
    m = multiplier(shape, c2c)
    options = {"spectral_op": 2, "spectral_layout": layout}
    for C in (1, 3):
        plain = World(cls, shape, P1, P2, c2c, C, precision=precision, options={"spectral_layout": layout})
        w = World(cls, shape, P1, P2, c2c, C, precision=precision, options=options)
        for a, b in zip(plain.plans, w.plans):
            assert a.debugPass("xx") is None and b.debugPass("xx") is not None
            assert b.getWorkSizeDevice() == a.getWorkSizeDevice() + a.getDomainSize()
        steps = w.plans[0].debugChain(S)
        assert [s["group"] for s in steps] == ["fz", "fy", "xx", "iy", "iz"]
        assert [s["tables"] for s in steps] == [F, F, I, I, I]
        assert steps[2]["launches"] == w.C
        ins, ms, wants = blocks(w, u, m)
        outs = run_spectral(w, ins, ms)
        for r in range(w.P):
            got = outs[r].reshape(wants[r].shape)
            assert not np.isnan(got).any(), f"rank {r}, depth {w.C}: NaN from a work slice reached the output"
            err = np.abs(got - wants[r]).max() / np.abs(wants[r]).max()
            assert err <= 1e-9, f"rank {r}, depth {w.C}: {err}"
        for r, pl in enumerate(w.plans):
            fps = SpectralFootprints(pl, shape)
            for cs in (1, 2):
                pl.setOption("compute_streams", cs)
                trace = pl.debugTrace(S)
                what = f"rank {r} depth {w.C} compute_streams {cs}"
                bad = sorted(sc.check(trace, steps, fps.of(S, steps)), key=lambda v: v.rule not in (3, 4))
                assert not bad, f"{what}: {len(bad)} violations\n" + "\n".join(repr(v) for v in bad[:10])
                launches = [o for o in trace if o["kind"] == LAUNCH]
                assert len(launches) == sum(s["launches"] for s in steps) > 0, what
                assert not any(o["scratch"] for o in launches), what


@pytest.mark.parametrize("precision", PRECISIONS)
def test_refusals(precision):
    for nx in (13, 4096):
        with pytest.raises(dfft.DfftError, match=f"error 4.*{nx}"):      # ERR_UNSUPPORTED, naming the length
            init(PENCIL, (nx, 8, 8), precision)
    with pytest.raises(dfft.DfftError, match="error 4.*768"):      # a two-level x axis is not the native chain
        init(PENCIL, (768, 8, 8), precision, two_level=1)
    with pytest.raises(dfft.DfftError, match="error 4.*768"):      # nor is the Bluestein kernel
        init(PENCIL, (768, 8, 8), precision, native_mixed=0)
    for cls in (dfft.MPIcuFFT_Slab_Z_Then_YX, dfft.MPIcuFFT_Slab_Y_Then_ZX):
        with pytest.raises(dfft.DfftError, match="error 4.*spectral_op.*60"):
            init(cls, (60, 8, 8), precision, 2, 1)
    for nx in sorted(LEFT_OUT[precision]):
        with pytest.raises(dfft.DfftError, match=f"error 4.*{nx}"):
            init(PENCIL, (nx, 8, 8), precision)
    with pytest.raises(dfft.DfftError, match="error 2.*spectral_op"):      # ERR_ARG
        init(PENCIL, (768, 8, 8), precision, value=3)
    with pytest.raises(dfft.DfftError, match=r"error 4.*768 points has no fused forward-multiply-inverse kernel \(powers of two from 2 to 2048 on a native chain\)"):
        init(PENCIL, (768, 8, 8), precision, value=1)      # value 1: its own message, unchanged
    for nx in (12, 768, 1000):      # the y and z axes may use any plan the library has
        assert init(PENCIL, (nx, 13, 14), precision).debugPass("xx") is not None


@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 2)])
@pytest.mark.parametrize("c2c", [True, False])
def test_a_power_of_two_gives_the_same_plan_under_1_and_2(P1, P2, c2c):
    shape = (16, 12, 14)
    one = World(PENCIL, shape, P1, P2, c2c, 3, options={"spectral_op": 1})
    two = World(PENCIL, shape, P1, P2, c2c, 3, options={"spectral_op": 2})
    raw = lambda d: None if d is None else ctypes.string_at(ctypes.addressof(d), ctypes.sizeof(d))      # noqa: E731
    for a, b in zip(one.plans, two.plans):
        assert a.getWorkSizeDevice() == b.getWorkSizeDevice() and a.getDomainSize() == b.getDomainSize()
        for d, dims in [(F, 1), (F, 2), (F, 3), (I, 1), (I, 2), (I, 3), (S, 3)]:
            assert a.debugChain(d, dims) == b.debugChain(d, dims) and a.debugTrace(d, dims) == b.debugTrace(d, dims)
        assert a.debugChain(S) and a.debugTrace(S)
        for g in GROUPS + ["xx"]:
            for k in range(4):
                assert raw(a.debugPass(g, k)) == raw(b.debugPass(g, k)), (g, k)
        assert a.debugPass("xx") is not None
