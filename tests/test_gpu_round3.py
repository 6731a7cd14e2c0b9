"""Round-3 parity additions (VERDICT r2 "next round" 3):

* C4 (1024^3 fp64: pencil 2x4, slab 8, R2C 2x4) compared with the CPU oracle at EVERY point -- the oracle transforms
  1024^3 in a few seconds on the GPU box's host, so the spot checks of test_gpu_fullsize.py are not the limit.
* C5 at full size: 2048^3 fp32 on one GPU (in = back aliased, like bench.py): direct-DFT entries, Parseval, round trip.
* the single-rank pass order z, x, y (build_pipeline_single) forced on small grids: both precisions, both L2 layouts,
  padded and packed rows, ragged tiles, mixed-radix, Bluestein and one 4096-point axis.
* the packed real z passes of EVERY generated mixed-radix length (DFFT_*_LIST_RMIXED* of csrc/kernels_mixed.inc).
* wave-uniform (scalar) table reads against the per-lane table reads on segmented plans (option uniform_tables).
* scalar-base address forms against the per-point 64-bit vector addresses (debug bit 1), bit for bit.
"""
import ctypes as C
import math
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import distributedfft_amd as dfft  # noqa: E402
from oracle import oracle as orc  # noqa: E402

from parity_metric import CENTER, check_forward, check_forward_blocks, entry_rel, forward_bound, record  # noqa: E402
from test_gpu_fullsize import direct_dft_entry, host_rms, make_world, owner_entry, run_all, spectrum_block  # noqa: E402
from test_gpu_parity import (CDT, NPDT, NPR, TOL_FWD, TOL_RT, rel, run_distributed, run_distributed_real,  # noqa: E402
                             run_single)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_free_gib():
    try:
        import psutil
        return psutil.virtual_memory().available / 2 ** 30
    except Exception:  # noqa: BLE001
        return 0.0


def gpu_free_gib():
    free_b, _ = torch.cuda.mem_get_info()
    return free_b / 2 ** 30


# ------------------------------------------------------------------------------------------
# C4 at every point
# ------------------------------------------------------------------------------------------
@pytest.mark.baseline_config
@pytest.mark.parametrize("P1,P2,c2c", [(2, 4, True), (8, 1, True), (2, 4, False)])
def test_c4_1024_fp64_every_point_vs_oracle(P1, P2, c2c):
    """BASELINE C4: 1024^3 fp64 on the pencil 2x4 grid (and slab 8, and the reference's own R2C API on 2x4), every rank a
    virtual rank of this GPU.  The global input is gathered on the host, transformed by the oracle (in place, OpenMP), and
    every rank's spectrum block is compared with the oracle's at every point, on the device."""
    need_host = 20 if c2c else 20
    if host_free_gib() < need_host:
        pytest.skip(f"needs {need_host} GiB of free host memory for the 1024^3 oracle transform, {host_free_gib():.0f} GiB free")
    if gpu_free_gib() < 110:
        pytest.skip(f"needs 110 GiB of free HBM (8 virtual ranks), {gpu_free_gib():.0f} GiB free")
    shape = (1024, 1024, 1024)
    n3 = float(np.prod(shape))
    ranks = make_world(shape, P1, P2, "double", c2c=c2c, center=True)       # zero-mean input: max|X| is no DC term (parity_metric.py)
    g = np.empty(shape, dtype=np.complex128 if c2c else np.float64)
    for rk in ranks:
        s, o = rk["plan"].getInSize(), rk["plan"].getInStart()
        g[o[0]:o[0] + s[0], o[1]:o[1] + s[1], :] = rk["x"].cpu().numpy()
    if c2c:
        run_all(ranks, lambda rk: rk["plan"].execC2C(rk["out"], rk["x"], dfft.FORWARD))
        orc.lib().orc_fft3d_c2c(g.ctypes.data_as(C.c_void_p), *shape, -1)       # in place: g is the spectrum now
        want = g
    else:
        run_all(ranks, lambda rk: rk["plan"].execR2C(rk["out"], rk["x"]))
        want = orc.fft3d_r2c(g)
        del g
    want_rms = host_rms(want)
    scale, worst, per_entry = 0.0, 0.0, 0.0
    for rk in ranks:
        s, o = rk["plan"].getOutSize(), rk["plan"].getOutStart()
        ref = torch.from_numpy(np.ascontiguousarray(want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]])).cuda()
        err = (spectrum_block(rk) - ref).abs()
        mag = ref.abs()
        worst = max(worst, float(err.max()))
        scale = max(scale, float(mag.max()))
        per_entry = max(per_entry, float((err / mag.clamp_(min=want_rms)).max()))
        del ref, err, mag
    assert worst / scale < 1e-11, worst / scale                       # scaled by max|X|
    bound = forward_bound("double", n3)
    record(f"C4 1024^3 fp64 {P1}x{P2} {'C2C' if c2c else 'R2C'}, every point, centred input", "double", int(n3), per_entry, bound, worst / scale)
    assert per_entry <= bound, per_entry          # per entry: max |err| / max(|X[k]|, rms(X)) <= 1e-13 log2(N^3)
    del want
    if c2c:
        run_all(ranks, lambda rk: rk["plan"].execC2C(rk["back"], rk["out"], dfft.INVERSE))
    else:
        run_all(ranks, lambda rk: rk["plan"].execC2R(rk["back"], rk["out"]))
    for rk in ranks:
        assert float((rk["back"] / n3 - rk["x"]).abs().max()) / 255.0 < 1e-10


# ------------------------------------------------------------------------------------------
# C5 at full size on one GPU
# ------------------------------------------------------------------------------------------
@pytest.mark.baseline_config
def test_c5_2048_fp32_full_size_single_gpu():
    """BASELINE C5's grid, 2048^3 fp32 complex (64 GiB per buffer), on one MI355X with the inverse written back over the
    input like bench.py does: spectrum entries against a direct DFT accumulated in fp64 slab by slab, Parseval, and the
    round trip against the regenerated input.  (The 8-GPU decomposition of this grid does not fit one GPU as virtual
    ranks: 8 x (in + out + 3 work slices); its kernels and layouts run in test_c5_fp32_axis_2048_and_1024_cube and, on the
    2 x 4 grid at every point, in test_c5_shaped_2048x2048x1024_fp32_pencil_2x4_every_point.)
    The gate is computed from the plan: in + out (domain size) + the library's work area + 3 GiB of temporaries (the fp64
    slabs of the direct DFT); conftest.py empties torch's cache first and turns a skip on an MI355X into a failure."""
    N = 2048
    n = N ** 3
    plan = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), precision="float")
    plan.initFFT(dfft.GlobalSize(N, N, N), dfft.Pencil_Partition(1, 1), False, c2c=True)      # sizes first, no allocation
    need = (8 * n + plan.getDomainSize() + plan.getWorkSizeDevice()) / 2 ** 30 + 3
    if gpu_free_gib() < need:
        pytest.skip(f"needs {need:.0f} GiB of free HBM (in 64 + out {plan.getDomainSize() / 2 ** 30:.0f} + work area "
                    f"{plan.getWorkSizeDevice() / 2 ** 30:.0f} + 3 GiB), {gpu_free_gib():.0f} GiB free")
    plan.setWorkArea()
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    out = torch.empty(plan.getDomainSize() // 8, dtype=torch.complex64, device="cuda")
    planes = 16                                  # x planes per slab: 16 * 2048^2 points = 512 MiB of complex64
    slab = planes * N * N

    def regenerate(visit):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(2048)
        for i in range(0, N, planes):
            visit(i, torch.view_as_complex(torch.rand((slab, 2), dtype=torch.float32, device="cuda", generator=gen) * 255.0))

    def fill(i, v):
        x[i * N * N:(i + planes) * N * N] = v
    regenerate(fill)
    ks = [(0, 0, 0), (1, 2, 3), (N - 1, N // 2, N // 3), (777, 1500, 2047)]
    idx = torch.arange(N, device="cuda", dtype=torch.float64)

    def phase(k):
        ang = -2.0 * math.pi * ((idx * k) % N) / N
        return torch.complex(torch.cos(ang), torch.sin(ang))
    want = [torch.zeros((), dtype=torch.complex128, device="cuda") for _ in ks]
    energy = torch.zeros((), dtype=torch.float64, device="cuda")
    for i in range(0, N, planes):
        blk = x[i * N * N:(i + planes) * N * N].reshape(planes, N, N).to(torch.complex128)
        energy += (blk.real ** 2 + blk.imag ** 2).sum()
        for j, k in enumerate(ks):
            want[j] += torch.einsum("xyz,z,y,x->", blk, phase(k[2]), phase(k[1]), phase(k[0])[i:i + planes])
        del blk
    torch.cuda.synchronize()
    plan.execC2C(out, x, dfft.FORWARD)
    spec = out[:n].reshape(N, N, N)
    scale = abs(complex(want[0].item()))
    spec_rms = math.sqrt(float(energy))           # Parseval: rms of the spectrum * sqrt(n) ... = sqrt(sum |x|^2) per entry
    for j, k in enumerate(ks):
        got = complex(spec[k].item())
        assert abs(got - complex(want[j].item())) / scale < 1e-4, (k, got, complex(want[j].item()))
        e = entry_rel(got, complex(want[j].item()), spec_rms)
        assert e < forward_bound("float", n), (k, e)
        record(f"C5 2048^3 fp32 one rank entry {k} vs direct DFT", "float", n, e, forward_bound("float", n), abs(got - complex(want[j].item())) / scale)
    eX = torch.zeros((), dtype=torch.float64, device="cuda")
    for i in range(0, N, planes):
        blk = spec[i:i + planes].to(torch.complex128)
        eX += (blk.real ** 2 + blk.imag ** 2).sum()
        del blk
    assert abs(float(eX) / (float(n) * float(energy)) - 1.0) < 1e-5      # Parseval at fp32
    torch.cuda.synchronize()
    plan.execC2C(x, out, dfft.INVERSE)          # in = back aliased: the inverse destroys `out` and overwrites the input
    worst = torch.zeros((), dtype=torch.float32, device="cuda")

    def compare(i, v):
        nonlocal worst
        worst = torch.maximum(worst, (x[i * N * N:(i + planes) * N * N] / float(n) - v).abs().max())
    regenerate(compare)
    assert float(worst) / 255.0 < 5e-5


@pytest.mark.baseline_config
def test_c5_2048_fp32_separable_input_every_point_single_gpu():
    """BASELINE C5's grid at EVERY point without a 128 GiB host transform (round-5 verdict, item 8): the input is separable,
    x[i, j, k] = f[i] g[j] h[k] with random complex integer vectors (components in [-7, 7]: every product is exact in fp32, so the
    device holds exactly the array the oracle is asked about), whose 3-D transform is the outer product F[kx] G[ky] H[kz] of three
    2048-point transforms of the CPU oracle.  The expected spectrum is built slab by slab on the device in fp64 and compared with
    all 2^33 entries the plan wrote: an index or layout error anywhere shows (f, g, h are unrelated random vectors), and the
    arithmetic is held to the per-entry bound of parity_metric.py.  Then the round trip, inverse written over the input."""
    N = 2048
    n = N ** 3
    plan = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), precision="float")
    plan.initFFT(dfft.GlobalSize(N, N, N), dfft.Pencil_Partition(1, 1), False, c2c=True)
    need = (8 * n + plan.getDomainSize() + plan.getWorkSizeDevice()) / 2 ** 30 + 6
    if gpu_free_gib() < need:
        pytest.skip(f"needs {need:.0f} GiB of free HBM, {gpu_free_gib():.0f} GiB free")
    plan.setWorkArea()
    rng = np.random.default_rng(20482048)
    vecs = [(rng.integers(-7, 8, N) + 1j * rng.integers(-7, 8, N)).astype(np.complex128) for _ in range(3)]
    spec1d = [orc.fft1d(v[None, :], -1)[0] for v in vecs]
    f, g, h = (torch.from_numpy(v.astype(np.complex64)).cuda() for v in vecs)
    F, G, H = (torch.from_numpy(v).cuda() for v in spec1d)
    spec_rms = math.sqrt(float(np.prod([np.mean(np.abs(v) ** 2) for v in spec1d])))       # rms of an outer product = product of the rms
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    out = torch.empty(plan.getDomainSize() // 8, dtype=torch.complex64, device="cuda")
    planes = 16

    def input_slab(i):
        return ((f[i:i + planes, None, None] * g[None, :, None]) * h[None, None, :]).reshape(-1)
    for i in range(0, N, planes):
        x[i * N * N:(i + planes) * N * N] = input_slab(i)
    torch.cuda.synchronize()
    plan.execC2C(out, x, dfft.FORWARD)
    spec = out[:n].reshape(N, N, N)
    worst = torch.zeros((), dtype=torch.float64, device="cuda")
    worst_abs = torch.zeros((), dtype=torch.float64, device="cuda")
    for i in range(0, N, planes):
        want = (F[i:i + planes, None, None] * G[None, :, None]) * H[None, None, :]
        err = (spec[i:i + planes].to(torch.complex128) - want).abs()
        worst_abs = torch.maximum(worst_abs, err.max())
        worst = torch.maximum(worst, (err / want.abs().clamp_(min=spec_rms)).max())
        del want, err
    per_entry = float(worst)
    peak = float(np.prod([np.max(np.abs(v)) for v in spec1d]))
    # (an outer product of three spectra has entries 30 x its rms on the lines where one factor peaks, and the passes along those lines
    # round at that scale: 3 x the bound of the unstructured inputs; measured 4.7e-6, profiles/r6_parity_table.txt)
    bound = 3 * forward_bound("float", n)
    record("C5 2048^3 fp32 one rank, separable input, every point", "float", n, per_entry, bound, float(worst_abs) / peak)
    assert float(worst_abs) / peak < 1e-4                    # scaled by max|X|
    assert per_entry <= bound, per_entry
    torch.cuda.synchronize()
    plan.execC2C(x, out, dfft.INVERSE)                       # in = back aliased
    rt = torch.zeros((), dtype=torch.float32, device="cuda")
    for i in range(0, N, planes):
        rt = torch.maximum(rt, (x[i * N * N:(i + planes) * N * N] / float(n) - input_slab(i)).abs().max())
    xmax = float(np.prod([np.max(np.abs(v)) for v in vecs]))
    assert float(rt) / xmax < 5e-5, float(rt) / xmax


@pytest.mark.baseline_config
def test_c5_2048_fp32_pencil_2x4_every_rank_at_real_size_every_point():
    """BASELINE C5 itself -- 2048^3 fp32 complex on the 2 x 4 pencil grid -- at its REAL size on one GPU (round-5 verdict, item 8):
    eight virtual ranks of 40 GiB each do not fit 288 GB at once, so the ranks run ONE AFTER THE OTHER on one shared set of buffers
    (in 8 + out 8 + work area 24 GiB) behind a callback transport that keeps what a rank sends to the rank under test and feeds it
    back when that rank's exchange asks for it.  For the rank under test T = (i, j) and its column partner P = (1 - i, j):
        P's row peers (z pass) -> their exchange-1 messages to P          T's row peers (z pass) -> theirs to T
        P (z, exchange 1 fed, y) -> its exchange-2 message to T           T: both exchanges fed, all three passes
    i.e. all eight ranks run once per rank under test, and EVERY rank is the rank under test in turn.  Every message is produced by
    the sending rank's own plan at its real size (per pipeline chunk, with the plan's own counts and displacements, which are asserted
    to agree at both ends); each rank's spectrum block [2048][1024][512] is compared at EVERY point with the outer product of three
    oracle transforms (the separable input of the single-GPU test above): all 2^33 entries of the C5 spectrum, from the plans that
    an 8-GPU run would execute."""
    N, P1, P2 = 2048, 2, 4
    n = N ** 3
    if gpu_free_gib() < 70:
        pytest.skip(f"needs 70 GiB of free HBM, {gpu_free_gib():.0f} GiB free")
    rng = np.random.default_rng(40962048)
    vecs = [(rng.integers(-7, 8, N) + 1j * rng.integers(-7, 8, N)).astype(np.complex128) for _ in range(3)]
    spec1d = [orc.fft1d(v[None, :], -1)[0] for v in vecs]
    f, g, h = (torch.from_numpy(v.astype(np.complex64)).cuda() for v in vecs)
    F, G, H = (torch.from_numpy(v).cuda() for v in spec1d)
    spec_rms = math.sqrt(float(np.prod([np.mean(np.abs(v) ** 2) for v in spec1d])))
    side = torch.cuda.Stream()
    held = {}          # (sender, receiver, exchange, chunk) -> bytes on the device
    calls = {}         # (rank, exchange) -> callbacks so far = the pipeline chunk
    feeding = set()    # (rank, exchange) pairs that are fed from `held`
    state = {"keep": None}     # the rank whose incoming messages are being collected

    def view(ptr, nbytes):
        return torch.as_tensor(dfft.DeviceBuffer(ptr, nbytes, owned=False), device="cuda")

    def make_callback(rank):
        def cb(send, sc, sd, recv, rc, rd, group, me, stream):
            exch = 1 if group[1] - group[0] == 1 else 2          # row group: neighbouring ranks; column group: P2 apart
            c = calls[(rank, exch)] = calls.get((rank, exch), -1) + 1
            with torch.cuda.stream(torch.cuda.ExternalStream(stream)):
                for q, peer in enumerate(group):
                    if q != me and sc[q] and peer == state["keep"]:
                        held[(rank, peer, exch, c)] = view(send + sd[q], sc[q]).clone()
                if (rank, exch) in feeding:
                    for q, peer in enumerate(group):
                        if not rc[q]:
                            continue
                        src = view(send + sd[q], sc[q]) if q == me else held.pop((peer, rank, exch, c))
                        assert src.numel() == rc[q], f"rank {rank} exchange {exch} chunk {c}: {peer} sent {src.numel()} B, {rc[q]} B expected"
                        view(recv + rd[q], rc[q]).copy_(src)
        return cb

    plans, comms = {}, {}
    for r in range(P1 * P2):
        comms[r] = dfft.Comm.callback(P1 * P2, r, make_callback(r))
        pl = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), comms[r], precision="float", rank=r)
        pl.initFFT(dfft.GlobalSize(N, N, N), dfft.Pencil_Partition(P1, P2), False, c2c=True)
        pl.setStream(side.cuda_stream)
        plans[r] = pl
    isz = plans[0].getInSize()
    assert isz == (1024, 512, 2048) and plans[0].getOutSize() == (2048, 1024, 512)
    d_in = torch.empty(isz[0] * isz[1] * isz[2], dtype=torch.complex64, device="cuda")
    d_out = torch.empty(max(pl.getDomainSize() for pl in plans.values()) // 8, dtype=torch.complex64, device="cuda")
    work = torch.empty(max(pl.getWorkSizeDevice() for pl in plans.values()), dtype=torch.uint8, device="cuda")

    def run(r, keep_for):
        """rank r's forward transform on the shared buffers; of what it sends only the messages to `keep_for` stay"""
        pl = plans[r]
        size, start = pl.getInSize(), pl.getInStart()
        x = d_in.reshape(size)
        planes = 32
        for i in range(0, size[0], planes):
            x[i:i + planes] = (f[start[0] + i:start[0] + i + planes, None, None] * g[None, start[1]:start[1] + size[1], None]) * h[None, None, :]
        pl.setWorkArea(work)
        state["keep"] = keep_for
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            pl.execC2C(d_out, d_in, dfft.FORWARD)
        torch.cuda.synchronize()

    peak = float(np.prod([np.max(np.abs(v)) for v in spec1d]))
    bound = 3 * forward_bound("float", n)           # separable input: see the single-GPU test above
    chunks = plans[0].getPipelineChunks()
    for target in range(P1 * P2):
        # the rank under test, its column partner (the source of its exchange-2 message) and the row peers of both
        ti, tj = target // P2, target % P2
        partner = (1 - ti) * P2 + tj
        held.clear(); calls.clear(); feeding.clear()
        for r in range(P1 * P2):
            if r // P2 == partner // P2 and r != partner:
                run(r, partner)                       # z pass -> exchange-1 message to the partner
        for r in range(P1 * P2):
            if r // P2 == ti and r != target:
                run(r, target)                        # z pass -> exchange-1 message to the rank under test
        feeding.add((partner, 1))     # (the partner's exchange 2 receives from the rank under test, which has not run: its x pass works on whatever is there)
        run(partner, target)                          # z, exchange 1 fed, y -> exchange-2 message to the rank under test
        assert not [k for k in held if k[1] == partner], f"rank {partner} did not consume every message it was sent"
        feeding.update({(target, 1), (target, 2)})
        run(target, -1)
        assert not held, f"messages left over: {sorted(held)[:4]}"
        assert calls[(target, 1)] == calls[(target, 2)] == chunks - 1
        osz, ost = plans[target].getOutSize(), plans[target].getOutStart()
        assert osz == (2048, 1024, 512) and ost == (0, 1024 * ti, 512 * tj)
        spec = d_out[:osz[0] * osz[1] * osz[2]].reshape(osz)
        Gb, Hb = G[ost[1]:ost[1] + osz[1]], H[ost[2]:ost[2] + osz[2]]
        worst = torch.zeros((), dtype=torch.float64, device="cuda")
        worst_abs = torch.zeros((), dtype=torch.float64, device="cuda")
        step = 64
        for i in range(0, N, step):
            want = (F[i:i + step, None, None] * Gb[None, :, None]) * Hb[None, None, :]
            err = (spec[i:i + step].to(torch.complex128) - want).abs()
            worst_abs = torch.maximum(worst_abs, err.max())
            worst = torch.maximum(worst, (err / want.abs().clamp_(min=spec_rms)).max())
            del want, err
        record(f"C5 2048^3 fp32 pencil 2x4, rank {target} at real size (peers' messages from their own plans), every point", "float", n,
               float(worst), bound, float(worst_abs) / peak)
        assert float(worst_abs) / peak < 1e-4, (target, float(worst_abs) / peak)
        assert float(worst) <= bound, (target, float(worst))
    for r in plans:
        plans[r] = None
    for c in comms.values():
        c.destroy()


@pytest.mark.baseline_config
def test_c5_shaped_2048x2048x1024_fp32_pencil_2x4_every_point():
    """The largest C5-SHAPED decomposed case one GPU holds as virtual ranks: 2048 x 2048 x 1024 fp32 complex on the pencil
    2 x 4 grid (BASELINE C5's partition, precision and its 2048-point tiled y / x passes with their 8-peer segment tables;
    8 x (in 4 + out 4 + work 12 GiB) = 160 GiB), compared with the CPU oracle at EVERY point (reference testcase 1:
    distributed == single transform of the same global array, tests/src/pencil/random_dist_3D.cu:386-403), then the
    round trip with the inverse written over the input (testcase 3, :641-666)."""
    shape = (2048, 2048, 1024)
    P1, P2 = 2, 4
    n3 = float(np.prod(shape))
    need_host = 16 * n3 / 2 ** 30 + 12
    if host_free_gib() < need_host:
        pytest.skip(f"needs {need_host:.0f} GiB of free host memory for the oracle transform, {host_free_gib():.0f} GiB free")
    if gpu_free_gib() < 180:
        pytest.skip(f"needs 180 GiB of free HBM (8 virtual ranks x 20 GiB + comparison slabs), {gpu_free_gib():.0f} GiB free")
    world = dfft.Comm.local(P1 * P2)
    ranks = []

    def block(r, size):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(4096 + r)
        # zero-mean: the per-entry bound applies (fp32 with the reference's mean of 127.5 carries the DC mass's rounding: parity_metric.py)
        return torch.view_as_complex(torch.rand((size[0] * size[1] * size[2], 2), dtype=torch.float32, device="cuda", generator=gen) * 255 - CENTER).reshape(size)
    for r in range(P1 * P2):
        pl = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), world, precision="float", rank=r)
        pl.initFFT(dfft.GlobalSize(*shape), dfft.Pencil_Partition(P1, P2), True, c2c=True)
        ranks.append(dict(plan=pl, x=block(r, pl.getInSize()), out=torch.zeros(pl.getDomainSize() // 8, dtype=torch.complex64, device="cuda")))
    g = np.empty(shape, dtype=np.complex128)
    for rk in ranks:
        s, o = rk["plan"].getInSize(), rk["plan"].getInStart()
        g[o[0]:o[0] + s[0], o[1]:o[1] + s[1], :] = rk["x"].cpu().numpy()
    torch.cuda.synchronize()
    run_all(ranks, lambda rk: rk["plan"].execC2C(rk["out"], rk["x"], dfft.FORWARD))
    orc.lib().orc_fft3d_c2c(g.ctypes.data_as(C.c_void_p), *shape, -1)       # in place: g is the spectrum now
    scale = max(float(np.abs(g[i:i + 64]).max()) for i in range(0, shape[0], 64))      # max|X| in slabs (no 32 GiB temporary)
    want_rms = host_rms(g)
    worst, per_entry = 0.0, 0.0
    step = 256
    for rk in ranks:
        s, o = rk["plan"].getOutSize(), rk["plan"].getOutStart()
        assert s[0] == shape[0]
        got = spectrum_block(rk)
        for k0 in range(0, s[0], step):
            ref = torch.from_numpy(np.ascontiguousarray(g[k0:k0 + step, o[1]:o[1] + s[1], o[2]:o[2] + s[2]])).cuda()
            err = (got[k0:k0 + step].to(torch.complex128) - ref).abs()
            worst = max(worst, float(err.max()) / scale)
            per_entry = max(per_entry, float((err / ref.abs().clamp_(min=want_rms)).max()))
            del ref, err
    assert worst < 1e-4, worst       # fp32 forward tolerance
    record("C5-shaped 2048x2048x1024 fp32 2x4, every point, centred input", "float", int(n3), per_entry, forward_bound("float", n3), worst)
    assert per_entry <= forward_bound("float", n3), per_entry     # per entry (parity_metric.py)
    del g
    run_all(ranks, lambda rk: rk["plan"].execC2C(rk["x"], rk["out"], dfft.INVERSE))       # in = back aliased
    for r, rk in enumerate(ranks):
        want = block(r, rk["plan"].getInSize())
        assert float((rk["x"] / n3 - want).abs().max()) / 255.0 < 5e-5
        del want


# ------------------------------------------------------------------------------------------
# single-rank pass order z, x, y, forced
# ------------------------------------------------------------------------------------------
def run_single_order(shape, prec, options, seed=5, center=False, arena=None):
    """arena: as in test_gpu_parity.run_single"""
    g = orc.fill_block(shape, (0, 0, 0), shape, 2, seed=seed)
    if center:
        g = g - CENTER * (1 + 1j)
    g = g.astype(NPDT[prec])
    esz = 16 if prec == "double" else 8

    def setup():
        plan = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), precision=prec)
        for k, v in options.items():
            plan.setOption(k, v)
        plan.initFFT(dfft.GlobalSize(*shape), dfft.Pencil_Partition(1, 1), arena is None, c2c=True)
        if arena is not None:
            return (plan,) + arena.plan_buffers(plan, g, CDT[prec])
        return plan, torch.from_numpy(g).cuda(), torch.zeros(plan.getDomainSize() // esz, dtype=CDT[prec], device="cuda"), None

    plan, d_in, d_out, d_back = setup() if arena is None else arena.once("run_single_order", setup)
    what = f"run_single_order {shape} {prec} {options}"
    if arena is not None:
        arena.refill()
    torch.cuda.synchronize()
    plan.execC2C(d_out, d_in, dfft.FORWARD)
    got = d_out[:g.size].cpu().numpy().reshape(shape)
    if arena is None:
        d_back = torch.zeros_like(d_in)
    else:
        arena.check_guards(what + " forward")
        arena.check_inputs(what + " forward")
        arena.refill(keep=[d_out])
    torch.cuda.synchronize()
    plan.execC2C(d_back, d_out, dfft.INVERSE)
    if arena is not None:
        arena.check_guards(what + " inverse")
    return g, got, d_back.cpu().numpy()


SINGLE_ORDER_SHAPES = [
    (16, 16, 16), (32, 64, 24), (64, 32, 20),          # Nz not a multiple of the tile (8 / 16 lines)
    (128, 256, 40), (8, 8, 2048), (2048, 16, 16), (16, 2048, 24),
    (12, 20, 24), (96, 100, 36), (1000, 6, 10),        # mixed-radix axes (native chain)
    (17, 33, 9), (6, 1500, 10), (1025, 4, 4),          # Bluestein axes
    (4096, 4, 16), (8, 4096, 8), (4, 8, 4096),         # sub-tile workgroups (kSUB > 1)
]


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("layout,pad", [(1, 128), (0, 128), (1, 0), (0, 384), (1, 384)])
@pytest.mark.parametrize("shape", SINGLE_ORDER_SHAPES)
def test_single_order_zxy_forced_vs_oracle(shape, layout, pad, prec):
    """option single_order = 1 (the z, x, y pass order that fp32 plans with 2048-point x and y lines pick by themselves):
    strided natural-line z pass, padded private L2 rows, y pass storing into the API layout"""
    g, got, back = run_single_order(shape, prec, {"single_order": 1, "single_layout": layout, "single_pad": pad})
    want = orc.fft3d_c2c(g.astype(np.complex128), -1)
    assert rel(got, want) < 2 * TOL_FWD[prec]
    check_forward(got, want, prec, g.size, zero_mean=False)
    assert rel(back / g.size, g) < TOL_RT[prec]


@pytest.mark.parametrize("prec", ["double", "float"])
def test_single_order_matches_default_order(prec):
    """the two single-rank pass orders give the same spectrum (different summation order: equal within tolerance)"""
    shape = (64, 128, 48)
    _, a, _ = run_single_order(shape, prec, {"single_order": 1})
    _, b, _ = run_single_order(shape, prec, {"single_order": 0})
    assert rel(a, b) < 2 * TOL_FWD[prec]


# ------------------------------------------------------------------------------------------
# every generated packed real z pass
# ------------------------------------------------------------------------------------------
def rmixed_lengths(tag):
    txt = open(os.path.join(ROOT, "distributedfft_amd", "csrc", "kernels_mixed.inc")).read()
    out = []
    for m in re.finditer(r"#define DFFT_%s_LIST_RMIXED\d\(Y\)(.*)" % tag, txt):
        out += [int(v) for v in re.findall(r"Y\((\d+),", m.group(1))]
    return sorted(set(out))


@pytest.mark.parametrize("prec", ["double", "float"])
def test_every_mixed_real_z_pass_vs_oracle(prec):
    """R2C / C2R with Nz = 2M for EVERY M that has a generated packed real configuration (each carries its own
    ONEPLANE choice and LDS size); small Nx, Ny, ragged tiles; two virtual ranks split the Hermitian half unevenly"""
    lengths = rmixed_lengths("F64" if prec == "double" else "F32")
    assert len(lengths) >= 30, lengths
    tol_f, tol_r = (2e-11, 1e-10) if prec == "double" else (2e-4, 5e-5)
    for M in lengths:
        shape = (6, 10, 2 * M)
        plans, ins, spec, backs = run_distributed_real(shape, 1, 2, prec)
        g = orc.fill_block(shape, (0, 0, 0), shape, 1, seed=13).astype(NPR[prec]).astype(np.float64)
        want = orc.fft3d_r2c(g)
        scale = np.max(np.abs(want))
        for r, pl in enumerate(plans):
            s, o = pl.getOutSize(), pl.getOutStart()
            assert np.max(np.abs(spec[r] - want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]])) / scale < tol_f, M
            assert rel(backs[r] / float(np.prod(shape)), ins[r]) < tol_r, M
        check_forward_blocks(plans, spec, want, prec, g.size, zero_mean=False)


# ------------------------------------------------------------------------------------------
# wave-uniform table reads
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("shape,P1,P2,chunks", [((64, 64, 64), 2, 2, 2), ((128, 64, 32), 2, 4, 1), ((256, 128, 32), 4, 1, 4),
                                                ((32, 2048, 16), 1, 2, 1), ((2048, 32, 16), 2, 1, 4), ((64, 4096, 8), 2, 2, 1),
                                                ((16, 8192, 8), 1, 2, 1), ((512, 256, 32), 8, 1, 2), ((1024, 16, 48), 2, 3, 8)])
def test_uniform_table_reads_match_per_lane_reads(shape, P1, P2, chunks, prec):
    """segmented sides whose segments start at multiples of 16 points read their address tables with scalar loads
    (PassArgs::luni / suni); the result must be bit-identical to the per-lane table reads (uniform_tables = 0) and match
    the oracle.  Covers 8 / 16-line tiles, sub-tile workgroups (2048 ... 8192 points) and pipelined chunks."""
    _, ins, spec_u, backs_u = run_distributed(shape, P1, P2, prec, chunks=chunks, options={"uniform_tables": 1})
    plans, _, spec_v, backs_v = run_distributed(shape, P1, P2, prec, chunks=chunks, options={"uniform_tables": 0})
    g = orc.fill_block(shape, (0, 0, 0), shape, 2, seed=7).astype(NPDT[prec]).astype(np.complex128)
    want = orc.fft3d_c2c(g, -1)
    scale = np.max(np.abs(want))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert np.array_equal(spec_u[r], spec_v[r])
        assert np.array_equal(backs_u[r], backs_v[r])
        assert np.max(np.abs(spec_u[r] - want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]])) / scale < TOL_FWD[prec]
        assert rel(backs_u[r] / float(np.prod(shape)), ins[r]) < TOL_RT[prec]
    check_forward_blocks(plans, spec_u, want, prec, g.size, zero_mean=False)


# ------------------------------------------------------------------------------------------
# scalar-base address forms
# ------------------------------------------------------------------------------------------
SCALAR_BASE_SINGLE = [((512, 512, 16), {}), ((16, 512, 512), {}), ((1024, 8, 1024), {}), ((512, 24, 1024), {}), ((2048, 16, 512), {}),
                      ((1024, 16, 512), {"mirror_inverse": 1, "pipeline_chunks": 4}), ((1000, 12, 600), {})]


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("shape,options", SCALAR_BASE_SINGLE)
def test_scalar_base_addresses_match_vector_addresses_single_rank(shape, options, prec):
    """the closed-form address sides of one-tile workgroups (lines of 512 points and more) take a scalar 64-bit base per point
    and one 32-bit lane offset; debug bit 1 (option debug_skip = 2) restores the per-point 64-bit vector
    addresses, which are also what dfft_tune_variants may give a pass back.  Same arithmetic, so bit-identical results:
    natural -> transposed tiles (z), tiled -> same tiles (y), tiled -> API layout (x), and the strided read of the mirrored inverse."""
    g, got_s, back_s = run_single_order(shape, prec, dict(options))
    _, got_v, back_v = run_single_order(shape, prec, dict(options, debug_skip=2))
    assert np.array_equal(got_s, got_v)
    assert np.array_equal(back_s, back_v)
    want = orc.fft3d_c2c(g.astype(np.complex128), -1)
    assert rel(got_s, want) < 2 * TOL_FWD[prec]
    check_forward(got_s, want, prec, g.size, zero_mean=False)
    assert rel(back_s / g.size, g) < TOL_RT[prec]


@pytest.mark.parametrize("prec", ["double", "float"])
@pytest.mark.parametrize("shape,P1,P2,chunks", [((512, 512, 32), 2, 2, 2), ((1024, 512, 16), 2, 1, 4), ((512, 1024, 16), 1, 2, 1)])
def test_scalar_base_addresses_match_vector_addresses_distributed(shape, P1, P2, chunks, prec):
    """the same on multi-rank plans: the point-major API layout on both sides of the x passes (load of the inverse, store of the
    forward transform) next to the table paths, which keep their vector arithmetic"""
    _, ins, spec_s, backs_s = run_distributed(shape, P1, P2, prec, chunks=chunks)
    plans, _, spec_v, backs_v = run_distributed(shape, P1, P2, prec, chunks=chunks, options={"debug_skip": 2})
    g = orc.fill_block(shape, (0, 0, 0), shape, 2, seed=7).astype(NPDT[prec]).astype(np.complex128)
    want = orc.fft3d_c2c(g, -1)
    scale = np.max(np.abs(want))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert np.array_equal(spec_s[r], spec_v[r])
        assert np.array_equal(backs_s[r], backs_v[r])
        assert np.max(np.abs(spec_s[r] - want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]])) / scale < TOL_FWD[prec]
        assert rel(backs_s[r] / float(np.prod(shape)), ins[r]) < TOL_RT[prec]
    check_forward_blocks(plans, spec_s, want, prec, g.size, zero_mean=False)


def test_variant_options_outside_the_key_range_are_rejected():
    """kernel configurations are keyed by (length, variant) with four bits for the variant: a variant of 16 or more would
    alias another length's configuration"""
    plan = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), precision="double")
    for key in ("variant_fz", "variant_ix"):
        with pytest.raises(dfft.DfftError, match="variant"):
            plan.setOption(key, 32)
        with pytest.raises(dfft.DfftError, match="variant"):
            plan.setOption(key, -2)
        plan.setOption(key, 15)
        plan.setOption(key, -1)
    x = torch.zeros((4, 6), dtype=torch.complex128, device="cuda")
    with pytest.raises(dfft.DfftError, match="variant"):
        dfft.fft1d_batched(torch.zeros_like(x), x, 6, 4, dfft.FORWARD, "double", variant=32)


# ------------------------------------------------------------------------------------------
# bench.py lines
# ------------------------------------------------------------------------------------------
def _bench(args, nproc=1, port=29671, self_launch=False):
    """self_launch: `python bench.py --gpus N` exactly as the driver's command line has it -- bench.py starts its own ranks"""
    import json
    import subprocess
    import sys
    if nproc > 1 and not self_launch:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.join(ROOT, "bench.py")] + args
    else:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("nproc,want,alt", [(8, "pencil 2x4", "slab P=8"), pytest.param(4, "pencil 2x2", "slab P=4", marks=pytest.mark.slow),
                                            (2, "slab P=2", None)])
def test_bench_multi_rank_line_is_self_documenting(nproc, want, alt):
    """`bench.py --gpus N --backend gloo` with the N ranks sharing this GPU: the headline decomposition is the one
    BASELINE.json names, slab over all ranks is config.alt, and the line carries the xGMI model (bytes per link / 153 GB/s
    next to the measured exchange spans) and overlap.hidden_frac"""
    # (pencil grids: the relayed run is made the headline whatever its time, to exercise that branch: on ranks that share one GPU
    # over gloo it is never the faster one.  The 4-rank case -- launched under torch.distributed.run -- is behind the `slow` marker.)
    line = _bench(["--gpus", str(nproc), "--backend", "gloo", "--size", "128", "--steps", "2", "--warmup", "1", "--full"] + (["--prefer-relay"] if nproc >= 4 else []),
                  nproc=nproc, port=29671 + nproc, self_launch=nproc != 4)      # 2 and 8 ranks: bench.py launches them itself
    assert line["n_gpus"] == nproc and line["round_trip_rel_linf"] < 1e-10
    assert line["config"]["decomposition"] == want
    if alt:
        assert line["config"]["alt"]["decomposition"].startswith(alt)
        assert line["config"]["alt"]["round_trip_rel_linf"] < 1e-10
        assert "hidden_frac" in line["config"]["alt"]["overlap"]
    else:
        assert "alt" not in line["config"]
    per = line["xgmi"]["per_exchange_per_transform"]
    assert per and all(m["links"] == m["group_ranks"] - 1 and m["predicted_ms"] > 0 and m["measured_ms"] >= 0 for m in per.values())
    vol = 16 * 128 ** 3 / nproc
    for m in per.values():
        assert abs(m["bytes_per_link"] - vol / m["group_ranks"]) < 1
    assert "hidden_frac" in line["overlap"] and line["overlap"]["step_ms"] == line["ms_per_step"]
    if alt:      # pencil grids: the same plan with the two-hop relay on exchange 2, measured next to the direct run
        rl = line["config"]["relay"]
        assert "error" not in rl, rl
        assert rl["relay"] == 3 and rl["round_trip_rel_linf"] < 1e-10 and rl["ms_per_step"] > 0
        assert rl["headline"] and line["ms_per_step"] == rl["ms_per_step"] and "relay" in line["config"]["transport"]
        assert line["config"]["direct"]["ms_per_step"] > 0 and line["config"]["direct"]["round_trip_rel_linf"] < 1e-10
        assert line["headline_is_best_of"] == 2 and line["headline_candidates"]["relayed_ms_per_step"] == rl["ms_per_step"]
        assert rl["transport_counters"]["relayed"] > 0 and rl["transport_counters"]["list"] == 2 * rl["transport_counters"]["relayed"]
        assert per["exchange 2"]["relay"]["links"] == nproc - 1 and per["exchange 2"]["relay"]["predicted_ms"] < per["exchange 2"]["predicted_ms"]
    else:
        assert "relay" not in line["config"]


def test_bench_single_gpu_line_carries_the_8gpu_kernels():
    """N = 1: roofline object, the multi-rank code path and the per-GPU kernels of the 8-GPU plans (exchange stubbed)"""
    line = _bench(["--size", "256", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline"])
    assert line["n_gpus"] == 1 and line["round_trip_rel_linf"] < 1e-10 and line["roofline"]["bound"] == "hbm"
    plans = line["config"]["per_gpu_kernels_8gpu"]["plans"]
    assert [p["decomposition"] for p in plans] == ["pencil 2x4", "slab P=8"]
    for p in plans:
        assert len(p["per_pass"]) == 6 and all(v["ms"] > 0 for v in p["per_pass"].values())
        assert p["alg_bytes_per_pass"] == 2 * 16 * 256 ** 3 / 8
    assert set(plans[0]["xgmi_model_per_transform"]) == {"exchange 1", "exchange 2"}
    assert set(plans[1]["xgmi_model_per_transform"]) == {"exchange 2"}


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """a plain run (no --full) carries the headline of --steps timed steps and none of the other legs; --dump-outputs writes what
    the last timed step computed from the same input in every run: two runs agree, and the inverse output is N^3 times the
    inverse transform of the spectrum"""
    n = 64
    lines, dumps = [], []
    for k in range(2):
        d = tmp_path / f"run{k}"
        lines.append(_bench(["--size", str(n), "--steps", "4", "--warmup", "1", "--dump-outputs", str(d)]))
        dumps.append({name: np.load(d / f"{name}.npy") for name in ("spectrum", "round_trip")})
    line = lines[0]
    assert line["n_gpus"] == 1 and line["steps"] == 4 and line["unit"] == "GFLOP/s" and line["higher_is_better"] and line["dtype"] == "f64"
    flops_step = 2 * 5.0 * n ** 3 * math.log2(n ** 3)
    assert line["ms_per_step"] > 0 and abs(line["value"] - flops_step / (line["ms_per_step"] * 1e-3) / 1e9) <= 0.05 * line["value"]
    assert not {"plain_buffers", "multi_rank_path", "per_gpu_kernels_8gpu", "alt"} & set(line["config"]) and "cpu_baseline" not in line
    spec, back = dumps[0]["spectrum"], dumps[0]["round_trip"]
    assert spec.shape == back.shape == (n ** 3, 2) and spec.dtype == back.dtype == np.float64
    spec_c = (spec[:, 0] + 1j * spec[:, 1]).reshape(n, n, n)
    back_c = (back[:, 0] + 1j * back[:, 1]).reshape(n, n, n)
    assert np.max(np.abs(np.fft.ifftn(spec_c) * n ** 3 - back_c)) < 1e-12 * np.max(np.abs(back_c))
    assert -1e-6 < back_c.real.min() / n ** 3 and back_c.real.max() / n ** 3 < 255.0 + 1e-6        # the input is uniform on [0, 255)
    for name in ("spectrum", "round_trip"):
        a, b = dumps[0][name], dumps[1][name]
        assert np.max(np.abs(a - b)) < 1e-12 * np.max(np.abs(a)), name
