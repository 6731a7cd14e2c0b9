"""execSpectralOps through the C++ binding (include/mpicufft_amd.hpp): tests/cpp/shim_spectral_ops.cpp computes two outputs in one call
and compares each with memcmp against execSpectralOp on the same plan.  Built as tests/test_gpu_cpp_shim.py builds its callers."""
import subprocess

import pytest

from test_gpu_cpp_shim import build, needs_mpich

pytestmark = pytest.mark.gpu


@needs_mpich
def test_cpp_shim_spectral_ops(tmp_path):
    exe, env = build(tmp_path, "shim_spectral_ops.cpp")
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("identical") == 2 and "spectral ops ok" in out.stdout, out.stdout
