// tests/cpp/spectral_mixed_chain_check.hip -- host-side emulation of the register hand-off of fft_spectral_kernel (fft_pass.hip.h) for the
// mixed-radix configurations of csrc/spectral_mixed.inc (option spectral_op = 2), no GPU needed.  What tests/cpp/spectral_chain_check.hip and
// tests/cpp/spectral_factor_check.hip do for the powers of two, check_fused of tests/cpp/chain_emulation.hpp, with all six forms: the array
// form, the two real-table forms and the factor forms (mkind 3, 4, 5).  The hand-off walks the registers in the kernel's own chunks
// (spectral_chunk<Cfg>(): a chunk width that does not cover E, as 4 does not for E = 10, 18, 30, 50, fails here).  The configurations are those
// of the list macros DFFT_F64_SPECTRAL_MIXED / DFFT_F32_SPECTRAL_MIXED (-DCHAIN_F32), the ones the launchers switch over; -DCHECK_PARTS=n
// -DCHECK_PART=k checks every n-th of them.  Built and run by tests/test_cpu_spectral_mixed_kernel.py.
#include "chain_emulation.hpp"

#ifndef CHECK_PARTS
#define CHECK_PARTS 1
#define CHECK_PART 0
#endif

namespace dfft {
#ifdef CHAIN_F32
#define DFFT_MIXED_F32
#else
#define DFFT_MIXED_F64
#endif
#include "../../distributedfft_amd/csrc/kernels_mixed.inc"
#include "../../distributedfft_amd/csrc/spectral_mixed.inc"
}  // namespace dfft

static int configurations = 0;

template <typename Cfg, int IDX> static void check_share(const char *name)
{
    if constexpr (IDX % CHECK_PARTS == CHECK_PART) { check_fused<Cfg>(name, 0, 5); configurations++; }
}

int main()
{
    constexpr int first = __COUNTER__ + 1;
#define CHECK(n, v, cfg) check_share<cfg, __COUNTER__ - first>(#cfg);
#ifdef CHAIN_F32
    DFFT_F32_SPECTRAL_MIXED(CHECK)
#else
    DFFT_F64_SPECTRAL_MIXED(CHECK)
#endif
    printf("%d forms of %d configurations checked, %d failed\n%s\n", checked, configurations, failures, failures ? "FAILED" : "ALL OK");
    return failures ? 1 : 0;
}
