// tests/cpp/chain_check.hip -- host-side emulation of the whole Stockham chain of fft_pass.hip.h (no GPU needed): check_chain of
// tests/cpp/chain_emulation.hpp -- the kernel's own pass_compute, lds_scatter / lds_gather and the store's slot -> output index map, driven
// for every (thread, line) of a workgroup, every line with its own random input, against a long-double DFT -- for a selection of
// power-of-two configurations and every generated mixed-radix configuration of kernels_mixed.inc (-DCHAIN_F32: fp32).  Built and run by
// tests/test_cpu_host.py.
#include "chain_emulation.hpp"

namespace dfft {
#ifdef CHAIN_F32
#define DFFT_MIXED_F32
#else
#define DFFT_MIXED_F64
#endif
#include "../../distributedfft_amd/csrc/kernels_mixed.inc"
}  // namespace dfft

int main()
{
#define X(n, v, cfg) check_chain<cfg>(#cfg);
#ifdef CHAIN_F32
    using P64 = PassCfg<float, 64, 8, 16, 2, 8, 8, 1, 1, 2>;
    using P1024 = PassCfg<float, 1024, 32, 16, 1, 32, 8, 4, 1, 1, 1>;
    check_chain<P64>("pow2"); check_chain<P1024>("pow2");
    DFFT_F32_LIST_MIXED_ALL(X)
#else
    using P64 = PassCfg<double, 64, 8, 8, 4, 8, 8, 1, 1, 2>;
    using P512 = PassCfg<double, 512, 16, 8, 1, 8, 8, 8, 1, 1>;
    using P1024 = PassCfg<double, 1024, 16, 8, 1, 16, 16, 4, 1, 1, 1>;
    check_chain<P64>("pow2"); check_chain<P512>("pow2"); check_chain<P1024>("pow2");
    DFFT_F64_LIST_MIXED_ALL(X)
#endif
    printf("%d configurations checked, %d failed\n%s\n", checked, failures, failures ? "FAILED" : "ALL OK");
    return failures ? 1 : 0;
}
