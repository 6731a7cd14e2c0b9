"""execSpectralSum through the C++ binding (include/mpicufft_amd.hpp): tests/cpp/shim_spectral_sum.cpp computes a divergence, three
inputs into one output in one call, and compares it with the host sum of three execSpectralOp results on the same plan (1e-12 of the
rms: rounding alone), and a one-input call with memcmp against execSpectralOp.  Built as tests/test_gpu_cpp_shim.py builds its callers."""
import subprocess

import pytest

from test_gpu_cpp_shim import build, needs_mpich

pytestmark = pytest.mark.gpu


@needs_mpich
def test_cpp_shim_spectral_sum(tmp_path):
    exe, env = build(tmp_path, "shim_spectral_sum.cpp")
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "one input: identical" in out.stdout and "within 1e-12" in out.stdout and "spectral sum ok" in out.stdout, out.stdout
