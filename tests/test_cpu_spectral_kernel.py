"""The register hand-off of fft_spectral_kernel (csrc/fft_pass.hip.h) without a GPU: tests/cpp/spectral_chain_check.hip drives the
kernel's own building blocks on the host -- forward chain, w[sigma(c)] = conj(v[c] * m), second chain, conjugation, the store's index
map -- for every configuration csrc/spectral_f64.hip / spectral_f32.hip instantiates, against N * ifft(fft(x) * m) in long double.
Three forms per configuration: the array multiplier, and the table forms w[sigma(c)] = conj(v[c]) * f with f = scale * sum and
f = scale / sum (0 at a zero sum), sum = tx[t + NT * sigma(c)] + sy + sz from integer tables that contain zero sums.  A failure of
tests/test_gpu_spectral_op.py::test_table_multiplier_against_numpy with this test green points at the plan's table offsets (Launch::ty_off,
the rank's slices of ay and az), not at the kernel's hand-off."""
import host_check


def test_forward_multiply_inverse_chain_emulated_on_the_host(tmp_path):
    for out in host_check.run(tmp_path, "spectral_chain_check.hip", (("f64", []), ("f32", ["-DCHAIN_F32"]))).values():
        assert "33 forms of 11 configurations checked, 0 failed" in out and "ALL OK" in out, out[-2000:]
