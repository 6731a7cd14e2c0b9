"""What an exec issues on the GPU is the schedule the dry trace promised (option trace = 1: the sink of run_chain that issues the HIP
calls logs the same records the dry sink lists, csrc/dfft.hip), and the results still meet the oracle bounds.  The schedule itself
is checked on the CPU (tests/test_cpu_schedule.py); nothing here races on purpose."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import distributedfft_amd as dfft
from oracle import oracle as orc
from parity_metric import check_forward, rms
from test_gpu_parity import TOL_RT, rel, run_distributed, run_distributed_real

pytestmark = pytest.mark.gpu
F, I = dfft.FORWARD, dfft.INVERSE


def issued_equals_dry(plans, want_stream1=None):
    for pl in plans:
        for d in (F, I):
            issued = pl.debugTrace(d, 0)
            assert issued and issued == pl.debugTrace(d, 3)      # (nothing that decides the schedule changed since the exec)
            if want_stream1 is not None:      # (a chain that is not marked split -- a single rank's conjugated inverse -- stays on one stream)
                assert any(o["stream"] == 1 for o in issued) == bool(want_stream1 and pl.debugChain(d)[0]["split"])


# (shape, P1, P2, chunks, options): pencil, slab and 1 x P2 grids, depths that do not divide the extents, both settings of
# compute_streams, an x-contiguous spectrum, a shared level scratch (two_level; a 4099-point long-Bluestein axis)
PLANS = [((32, 32, 32), 2, 4, 4, {"compute_streams": 2}), ((32, 32, 32), 2, 4, 3, {"compute_streams": 1}), ((16, 16, 16), 3, 2, 5, {}),
         ((64, 32, 16), 8, 1, 2, {"compute_streams": 2}), ((64, 32, 16), 4, 1, 4, {}), ((16, 32, 16), 1, 4, 3, {"compute_streams": 2}),
         ((32, 32, 32), 2, 2, 4, {"spectral_layout": 1, "compute_streams": 2}), ((12, 10, 14), 2, 2, 3, {"two_level": 1, "compute_streams": 2}),
         ((4, 4, 4099), 2, 1, 2, {"compute_streams": 2}), ((32, 16, 64), 1, 1, 3, {"compute_streams": 2}), ((32, 16, 64), 1, 1, 1, {})]


@pytest.mark.parametrize("shape,P1,P2,chunks,options", PLANS)
def test_issued_operations_equal_the_dry_trace_c2c(shape, P1, P2, chunks, options):
    plans, ins, spec, backs = run_distributed(shape, P1, P2, "double", chunks=chunks, options=dict(options, trace=1))
    scratch = any(o["scratch"] for o in plans[0].debugTrace(F))
    assert scratch == ("two_level" in options or 4099 in shape)
    want1 = None if "compute_streams" not in options else options["compute_streams"] == 2 and plans[0].getPipelineChunks() > 1 and not scratch
    issued_equals_dry(plans, want1)
    want = orc.fft3d_c2c(orc.fill_block(shape, (0, 0, 0), shape, 2, seed=7), -1)
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        check_forward(spec[r], want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]], "double", want.size, want_rms=rms(want), zero_mean=False)
        assert rel(backs[r] / float(np.prod(shape)), ins[r]) < TOL_RT["double"]


@pytest.mark.parametrize("shape,P1,P2,options", [((32, 32, 32), 2, 4, {"compute_streams": 2}), ((64, 32, 16), 4, 1, {}), ((16, 32, 64), 1, 4, {"compute_streams": 1})])
def test_issued_operations_equal_the_dry_trace_r2c(shape, P1, P2, options):
    plans, ins, spec, backs = run_distributed_real(shape, P1, P2, "double", options=dict(options, trace=1))
    issued_equals_dry(plans, None if not options else options["compute_streams"] == 2)
    want = orc.fft3d_r2c(orc.fill_block(shape, (0, 0, 0), shape, 1, seed=13))
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        check_forward(spec[r], want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]], "double", int(np.prod(shape)), want_rms=rms(want), zero_mean=False)
        assert rel(backs[r] / float(np.prod(shape)), ins[r]) < TOL_RT["double"]


def test_compute_streams_set_after_the_work_area_exists_takes_effect():
    """initFFT(allocate=True) has made the work area and the streams of the options as they stood (one compute stream); the option set
    afterwards is read by the next exec, which creates the second stream -- no silent one-stream run"""
    shape, P1, P2 = (32, 32, 32), 2, 4
    P = P1 * P2
    world = dfft.Comm.local(P)
    plans, ins, outs, backs = [], [], [], []
    for r in range(P):
        pl = dfft.MPIcuFFT_Pencil_Opt1(dfft.Configurations(), world, precision="double", rank=r)
        pl.setPipelineChunks(4)
        pl.setOption("compute_streams", 1)
        pl.setOption("trace", 1)
        pl.initFFT(dfft.GlobalSize(*shape), dfft.Pencil_Partition(P1, P2), True, c2c=True)
        blk = orc.fill_block(shape, pl.getInStart(), pl.getInSize(), 2, seed=7)
        plans.append(pl)
        ins.append(torch.from_numpy(blk).cuda())
        outs.append(torch.zeros(pl.getDomainSize() // 16, dtype=torch.complex128, device="cuda"))
        backs.append(torch.zeros_like(ins[-1]))
    torch.cuda.synchronize()
    results = []
    for cs in (1, 2):
        for pl in plans:
            pl.setOption("compute_streams", cs)
        dry = [pl.debugTrace(F) for pl in plans]
        with ThreadPoolExecutor(P) as ex:
            list(ex.map(lambda r: plans[r].execC2C(outs[r], ins[r], F), range(P)))
        torch.cuda.synchronize()
        for r, pl in enumerate(plans):
            assert pl.debugTrace(F, 0) == dry[r]
            assert any(o["stream"] == 1 for o in dry[r]) == (cs == 2)
        results.append([plans[r].spectrumView(outs[r]).contiguous().cpu().numpy() for r in range(P)])
    want = orc.fft3d_c2c(orc.fill_block(shape, (0, 0, 0), shape, 2, seed=7), -1)
    for r, pl in enumerate(plans):
        s, o = pl.getOutSize(), pl.getOutStart()
        assert np.array_equal(results[0][r], results[1][r])
        check_forward(results[1][r], want[:, o[1]:o[1] + s[1], o[2]:o[2] + s[2]], "double", want.size, want_rms=rms(want), zero_mean=False)
