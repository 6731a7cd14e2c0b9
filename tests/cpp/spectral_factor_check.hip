// tests/cpp/spectral_factor_check.hip -- host-side emulation of the factor-table forms of fft_spectral_kernel (fft_pass.hip.h; mkind 3, 4, 5 of
// dfft_exec_spectral_op), no GPU needed: check_fused of tests/cpp/chain_emulation.hpp, as tests/cpp/spectral_chain_check.hip runs it for the
// array and the real-table forms, with the hand-off w[spectral_sigma(c)] = spectral_factor_point(v[c], cx[k], line, mkind, sum), k = t + NT *
// spectral_sigma(c), line = spectral_factor_line(scale, cy, cz) and sum = (tx[k] + sy) + sz -- the two functions the kernel itself calls, so
// this is the kernel's arithmetic and not a restatement of it.  Tables: cx over the points and (cy, cz) per line drawn from {+-1, +-i, +-1 +-i};
// integer sum tables -3 .. 3 that contain zero sums.  Each form is compared with N * ifft(fft(x) * m), m = scale * cx * cy * cz * {1, sum,
// 1 / sum or 0}, by long-double DFTs, for every configuration csrc/spectral_f64.hip / spectral_f32.hip instantiates (-DCHAIN_F32: fp32).
// Built and run by tests/test_cpu_spectral_factors.py.
#ifdef CHAIN_F32
#include "../../distributedfft_amd/csrc/cfg_f32.hip.h"
#define CHECK(n) check_fused<F32_##n>("F32_" #n, 3, 5);
#else
#include "../../distributedfft_amd/csrc/cfg_f64.hip.h"
#define CHECK(n) check_fused<F64_##n>("F64_" #n, 3, 5);
#endif
#include "chain_emulation.hpp"

int main()
{
    CHECK(2) CHECK(4) CHECK(8) CHECK(16) CHECK(32) CHECK(64) CHECK(128) CHECK(256) CHECK(512) CHECK(1024) CHECK(2048)
    printf("%d forms of %d configurations checked, %d failed\n%s\n", checked, checked / 3, failures, failures ? "FAILED" : "ALL OK");
    return failures ? 1 : 0;
}
