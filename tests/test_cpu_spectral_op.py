"""The chain of execSpectralOp (option "spectral_op", include/dfft_c.h: dfft_exec_spectral_op) without a GPU:
z -> ex1 -> y -> ex2 -> xx -> ex2^-1 -> y^-1 -> ex1^-1 -> z^-1, where xx is the forward x pass, the pointwise multiplier and the
inverse x pass in one launch per ky chunk.

Data flow: the library's own steps (debugChain(SPECTRAL_OP)) replayed with tests/layout_sim.py's pass descriptors on NaN-filled work
slices, the xx launches simulated as ifft(fft(x) * m) * Nx between their load and store addresses, every exchange with the chunked tables
of the direction the step names.  Schedule: the trace the executor's loop produces (debugTrace(SPECTRAL_OP)) against the footprints of
its launches and exchanges (tests/schedule_check.py, rules 1-5)."""
import ctypes

import numpy as np
import pytest

import distributedfft_amd as dfft
import schedule_check as sc
from layout_sim import MODES, Pass, World
from schedule_check import EXCHANGE, LAUNCH

F, I, S = dfft.FORWARD, dfft.INVERSE, dfft.SPECTRAL_OP
PENCIL, SLAB = dfft.MPIcuFFT_Pencil_Opt1, dfft.MPIcuFFT_Slab_Opt1
GRIDS = [(1, 1), (2, 1), (1, 2), (2, 2), (2, 3)]
SHAPES = [(16, 12, 14), (8, 10, 38)]      # R2C on the second: Nzc = 20 -> 7 + 7 + 6 over P2 = 3 (ragged tiles)
DEPTHS = [1, 3]
ROWS = [pytest.param(cls, P1, P2, shape, c2c, spectral,
                     id=f"{cls.__name__[8:]}-{P1}x{P2}-{'x'.join(map(str, shape))}-{'c2c' if c2c else 'r2c'}-layout{spectral}")
        for cls in (PENCIL, SLAB) for P1, P2 in GRIDS if cls is PENCIL or P2 == 1
        for shape in SHAPES for c2c in (True, False) for spectral in (0, 1)]


def world(cls, shape, P1, P2, c2c, chunks, spectral, op=1):
    return World(cls, shape, P1, P2, c2c, chunks, options={"spectral_op": op, "spectral_layout": spectral})


def multiplier(shape, c2c, seed=7):
    """a multiplier over the whole spectrum with |m| <= 1: the transform of a random real-space kernel (Hermitian-consistent for R2C)"""
    rng = np.random.default_rng(seed)
    if c2c:
        m = np.fft.fftn(rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    else:
        m = np.fft.rfftn(rng.standard_normal(shape))
    return m / np.abs(m).max()


def blocks(w, u, m):
    """per rank: the flat input block, the multiplier block (Nx, yo, zs) and the expected output block"""
    n = int(np.prod(w.shape))
    full = np.fft.ifftn(np.fft.fftn(u) * m) * n if w.c2c else np.fft.irfftn(np.fft.rfftn(u) * m, s=w.shape, axes=(0, 1, 2)) * n
    ins, ms, wants = [], [], []
    for pl in w.plans:
        (nx, ny, nz), (x0, y0, z0) = pl.getInSize(), pl.getInStart()
        ins.append(np.ascontiguousarray(u[x0:x0 + nx, y0:y0 + ny, z0:z0 + nz]).ravel().copy())
        wants.append(full[x0:x0 + nx, y0:y0 + ny, z0:z0 + nz])
        (_, ky, kz), (_, k0, z0) = pl.getOutSize(), pl.getOutStart()
        ms.append(m[:, k0:k0 + ky, z0:z0 + kz])
    return ins, ms, wants


def run_spectral(w, ins, ms):
    """one execSpectralOp on every rank, step by step like World.run; ins are only read"""
    steps = w.plans[0].debugChain(S)
    assert all(pl.debugChain(S) == steps for pl in w.plans[1:])
    Nx = w.shape[0]
    length = (w.shape[2], w.shape[1], w.shape[0])
    nin = [int(np.prod(pl.getInSize())) for pl in w.plans]
    outs = [np.full(n, np.nan, dtype=np.complex128 if w.c2c else np.float64) for n in nin]
    keep = [a.copy() for a in ins]
    W = w.buffers(1 + max(b for s in steps for b in (s["src"], s["dst"])))
    buf = lambda b: ins if b == -2 else outs if b == -1 else [W[r][b] for r in range(w.P)]      # noqa: E731
    for i, s in enumerate(steps):
        src, dst, per = buf(s["src"]), buf(s["dst"]), s["per_chunk"]
        assert s["src"] != -1 and (s["dst"] != -1 or i == len(steps) - 1) and s["dst"] != -2      # `in` never written, `out` by z^-1 only
        for c in range(s["launches"] // per):
            for r, pl in enumerate(w.plans):
                for k in range(c * per, (c + 1) * per):
                    p = Pass(pl, s["group"], k)
                    if s["group"] != "xx":
                        p.run(src[r], dst[r], length[s["axis"]], MODES[s["form"]])
                        continue
                    k0 = sum(pl.debugPass("xx", q).na for q in range(k))      # first ky row of the chunk
                    for a in range(p.d.na):
                        for line in range(p.d.LB):
                            x = src[r][p.load_offset(a, line, np.arange(Nx), Nx)]
                            y = np.fft.ifft(np.fft.fft(x) * ms[r][:, k0 + a, line]) * Nx
                            dst[r][p.store_offset(a, line, np.arange(Nx), Nx)] = y
            if s["exchange"]:
                w.exchange(s["tables"], s["exchange"], c, dst, buf(steps[i + 1]["src"]))
    for a, b in zip(ins, keep):
        assert np.array_equal(a, b)
    return outs


@pytest.mark.parametrize("cls,P1,P2,shape,c2c,spectral", ROWS)
def test_data_flow(cls, P1, P2, shape, c2c, spectral):
    rng = np.random.default_rng(11)
    u = rng.uniform(0, 255, shape) - 127.5
    if c2c:
        u = u + 1j * (rng.uniform(0, 255, shape) - 127.5)
    m = multiplier(shape, c2c)
    for C in DEPTHS:
        w = world(cls, shape, P1, P2, c2c, C, spectral)
        steps = w.plans[0].debugChain(S)
        assert [s["group"] for s in steps] == ["fz", "fy", "xx", "iy", "iz"]
        assert [s["tables"] for s in steps] == [F, F, I, I, I]
        assert [s["exchange"] for s in steps] == [int(P2 > 1), 2 * int(P1 > 1), 2 * int(P1 > 1), int(P2 > 1), 0]
        assert steps[2]["launches"] == w.C
        ins, ms, wants = blocks(w, u, m)
        outs = run_spectral(w, ins, ms)
        for r in range(w.P):
            got = outs[r].reshape(wants[r].shape)
            assert not np.isnan(got).any(), f"rank {r}, depth {w.C}: NaN from a work slice reached the output"
            err = np.abs(got - wants[r]).max() / np.abs(wants[r]).max()
            assert err <= 1e-9, f"rank {r}, depth {w.C}: {err}"


def test_xx_descriptors_are_the_sides_of_fx_and_ix():
    """load side: fx's segments, each base moved to the chunk's first ky row; store side and chunking: ix[c]'s"""
    for spectral in (0, 1):
        w = world(PENCIL, (8, 10, 38), 2, 3, False, 3, spectral)
        for pl in w.plans:
            fx, k0 = pl.debugPass("fx"), 0
            for c in range(w.C):
                xx, ix = pl.debugPass("xx", c), pl.debugPass("ix", c)
                assert (xx.na, xx.LB, xx.LA, xx.load_kind, xx.store_kind, xx.swap) == (ix.na, ix.LB, ix.LA, 1, 2, 0)
                assert xx.lnseg == fx.lnseg and list(xx.lstart[:xx.lnseg]) == list(fx.lstart[:fx.lnseg]) and list(xx.llen[:xx.lnseg]) == list(fx.llen[:fx.lnseg])
                assert [xx.lbase[s] for s in range(xx.lnseg)] == [fx.lbase[s] + k0 * fx.llen[s] * fx.LB for s in range(fx.lnseg)]
                assert xx.snseg == ix.snseg and [list(getattr(xx, f)[:xx.snseg]) for f in ("sstart", "slen", "sbase")] == [list(getattr(ix, f)[:ix.snseg]) for f in ("sstart", "slen", "sbase")]
                assert pl.debugPointTable("xx", c, True) == pl.debugPointTable("ix", c, True)
                k0 += xx.na


# ---- schedule ------------------------------------------------------------------------------------------------------------------
class SpectralFootprints(sc.PlanFootprints):
    """an exchange of the spectral-operator chain uses the tables of the direction its step names"""

    def of(self, direction, steps):
        launch = super().of(direction, steps)

        def footprint(i, op):
            if op["kind"] == LAUNCH:
                return launch(i, op)
            ld, st = self.exchange(steps[op["step"]]["tables"], op["which"], op["chunk"])
            rb, ri = self.where(op["src"], ld)
            wb, wi = self.where(op["dst"], st)
            return {rb: ri}, {wb: wi}
        return footprint


@pytest.mark.parametrize("cls,P1,P2,shape,c2c,spectral", ROWS)
def test_schedule(cls, P1, P2, shape, c2c, spectral):
    for C in DEPTHS:
        w = world(cls, shape, P1, P2, c2c, C, spectral)
        for r, pl in enumerate(w.plans):
            fps = SpectralFootprints(pl, shape)
            steps = pl.debugChain(S)
            for cs in (1, 2):
                pl.setOption("compute_streams", cs)
                trace = pl.debugTrace(S)
                what = f"rank {r} depth {w.C} compute_streams {cs}"
                bad = sorted(sc.check(trace, steps, fps.of(S, steps)), key=lambda v: v.rule not in (3, 4))
                assert not bad, f"{what}: {len(bad)} violations\n" + "\n".join(repr(v) for v in bad[:10])
                launches = [o for o in trace if o["kind"] == LAUNCH]
                assert len(launches) == sum(s["launches"] for s in steps) > 0, what
                assert not any(o["scratch"] for o in launches), what
                assert all(o["src"] != -1 and o["dst"] != -2 for o in trace if o["kind"] in (LAUNCH, EXCHANGE)), what
                assert [o["dst"] for o in launches if o["dst"] == -1] == [-1] * steps[-1]["launches"], what
                on1 = [o for o in trace if o["stream"] == 1]
                if cs == 1:
                    assert not on1, what
                elif w.C >= 2:      # the odd chunks really are on stream 1
                    for o in launches:
                        chunks = steps[o["step"]]["launches"] // steps[o["step"]]["per_chunk"]
                        assert o["stream"] == (o["chunk"] & 1 if chunks > 1 else 0), what
                    assert on1, what
                if P1 > 1 and P2 > 1:
                    assert all(o["stream"] == (3 if o["which"] == 2 else 2) for o in trace if o["kind"] == EXCHANGE), what


# ---- option off, error paths ---------------------------------------------------------------------------------------------------
GROUPS = ["fz", "fy", "fx", "ix", "iy", "iz", "pz1", "qz1", "py2", "qy2", "sz", "sx", "sy"]


@pytest.mark.parametrize("P1,P2", [(1, 1), (2, 2)])
@pytest.mark.parametrize("c2c", [True, False])
def test_option_off_changes_nothing(P1, P2, c2c):
    shape = (16, 12, 14)
    plain = World(PENCIL, shape, P1, P2, c2c, 3)      # a plan that never heard of the option
    off = world(PENCIL, shape, P1, P2, c2c, 3, 0, op=0)
    on = world(PENCIL, shape, P1, P2, c2c, 3, 0, op=1)
    raw = lambda d: None if d is None else ctypes.string_at(ctypes.addressof(d), ctypes.sizeof(d))      # noqa: E731
    for a, b, c in zip(plain.plans, off.plans, on.plans):
        assert a.getWorkSizeDevice() == b.getWorkSizeDevice()
        assert c.getWorkSizeDevice() == a.getWorkSizeDevice() + a.getDomainSize()      # one more slice, nothing else
        for other in (b, c):
            for d in (F, I):
                for dims in (1, 2, 3):
                    assert a.debugChain(d, dims) == other.debugChain(d, dims)
                    assert a.debugTrace(d, dims) == other.debugTrace(d, dims)
            for g in GROUPS:
                for k in range(4):
                    assert raw(a.debugPass(g, k)) == raw(other.debugPass(g, k)), (g, k)
        assert b.debugPass("xx") is None and b.debugChain(S) == [] and b.debugTrace(S) == []
        assert c.debugPass("xx") is not None
        with pytest.raises(dfft.DfftError, match="error 3.*spectral_op"):      # ERR_STATE
            b.execSpectralOp(1, 2, multiplier=3)
        with pytest.raises(dfft.DfftError, match="error 3.*spectral_op"):
            a.execSpectralOp(1, 2, tables=(3, 4, 5))


@pytest.mark.parametrize("precision", ["double", "float"])
def test_unsupported_plans_fail_at_init(precision):
    def init(cls, shape, P1=1, P2=1, **options):
        comm = dfft.Comm.local(P1 * P2) if P1 * P2 > 1 else None
        pl = cls(dfft.Configurations(), comm, precision=precision, rank=0)
        for k, v in dict(options, spectral_op=1).items():
            pl.setOption(k, v)
        pl.initFFT(dfft.GlobalSize(*shape), dfft.Partition(P1, P2), allocate=False)
        return pl
    for nx in (12, 4096):
        with pytest.raises(dfft.DfftError, match=f"error 4.*{nx}"):      # ERR_UNSUPPORTED, naming the length
            init(PENCIL, (nx, 8, 8))
    with pytest.raises(dfft.DfftError, match="error 4.*spectral_op"):
        init(dfft.MPIcuFFT_Slab_Z_Then_YX, (16, 8, 8), 2, 1)
    with pytest.raises(dfft.DfftError, match="error 4.*spectral_op"):
        init(dfft.MPIcuFFT_Slab_Y_Then_ZX, (16, 8, 8), 2, 1)
    with pytest.raises(dfft.DfftError, match="error 4.*16"):      # a two-level x axis is not the native chain
        init(PENCIL, (16, 8, 8), two_level=1)
    for nx in (2, 16, 2048):      # the y and z axes may use any plan the library has
        assert init(PENCIL, (nx, 12, 14)).debugPass("xx") is not None
