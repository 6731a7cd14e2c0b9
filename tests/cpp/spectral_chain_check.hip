// tests/cpp/spectral_chain_check.hip -- host-side emulation of the register hand-off of fft_spectral_kernel (fft_pass.hip.h), no GPU needed:
// check_fused of tests/cpp/chain_emulation.hpp (tests/cpp/chain_check.hip runs its one-chain sibling) for the array form,
// w[spectral_sigma(c)] = conj(v[c] * m[k]) with k = t + NT * spectral_sigma(c), and the two real-table forms in its place,
// w[sigma(c)] = conj(v[c]) * f, f = scale * sum or scale / sum (0 at a zero sum) with sum = tx[k] + sy + sz from integer tables.  Each of the
// three forms is compared with N * ifft(fft(x) * m) by long-double DFTs, for every configuration csrc/spectral_f64.hip / spectral_f32.hip
// instantiates (-DCHAIN_F32: fp32).  Built and run by tests/test_cpu_spectral_kernel.py.
#ifdef CHAIN_F32
#include "../../distributedfft_amd/csrc/cfg_f32.hip.h"
#define CHECK(n) check_fused<F32_##n>("F32_" #n, 0, 2);
#else
#include "../../distributedfft_amd/csrc/cfg_f64.hip.h"
#define CHECK(n) check_fused<F64_##n>("F64_" #n, 0, 2);
#endif
#include "chain_emulation.hpp"

int main()
{
    CHECK(2) CHECK(4) CHECK(8) CHECK(16) CHECK(32) CHECK(64) CHECK(128) CHECK(256) CHECK(512) CHECK(1024) CHECK(2048)
    printf("%d forms of %d configurations checked, %d failed\n%s\n", checked, checked / 3, failures, failures ? "FAILED" : "ALL OK");
    return failures ? 1 : 0;
}
