"""Build and run a check program of tests/cpp/ on the host: the one place that knows the hipcc command line of the CPU-only kernel checks
(tests/test_cpu_host.py, test_cpu_spectral_kernel.py, test_cpu_spectral_factors.py, test_cpu_spectral_mixed_kernel.py).

run(tmp_path, source, variants, flags) compiles tests/cpp/<source> once per (tag, extra flags) variant, all compilers at once, waits for
them, runs all executables at once and returns {tag: output} (stdout and stderr together) in the order of the variants.  A compiler or a
program that exits with another status than 0 fails the test with the tail of its output; what the output must say is the caller's to
assert.  Skips the test where there is no hipcc."""
import os
import shutil
import subprocess

import pytest

FLAGS = ["-O1", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize"]


def run(tmp_path, source, variants=(("", []),), flags=FLAGS):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(os.path.dirname(__file__), "cpp", source)
    stem = os.path.splitext(source)[0]
    builds = []
    for tag, extra in variants:
        exe = str(tmp_path / (stem + "_" + tag if tag else stem))
        log = open(exe + ".log", "w+")
        builds.append((tag, exe, log, subprocess.Popen([hipcc, *flags, *extra, src, "-o", exe], stdout=log, stderr=subprocess.STDOUT)))
    for tag, exe, log, proc in builds:      # every compiler has ended before the first assertion: a failure leaves nothing running
        proc.wait()
    for tag, exe, log, proc in builds:
        log.seek(0)
        said = log.read()
        log.close()
        assert proc.returncode == 0, f"{source} {tag}: hipcc exited with {proc.returncode}\n{said[-2000:]}"
    runs = [(tag, subprocess.Popen([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)) for tag, exe, _, _ in builds]
    outputs = {}
    for tag, r in runs:
        outputs[tag] = r.communicate()[0]
    for tag, r in runs:
        assert r.returncode == 0, f"{source} {tag}: exit status {r.returncode}\n{outputs[tag][-2000:]}"
    return outputs
