// kernels.hip.inc -- launchers shared by the kernel translation units (kernels_*.hip, real_*.hip, bluestein_*.hip,
// mixed_*.hip, rmixed_*.hip): one instantiation per configuration behind length-indexed entry points.
#include "fft_pass.hip.h"
#include "dfft_internal.hpp"

namespace dfft {

template <typename Cfg> static int launch_cfg(const PassArgs &A, hipStream_t stream)
{
    if constexpr (Cfg::kFIX != 0) {          // compiled for one pair of address forms: every other launch runs the generic sibling
        if (!fix_ok<Cfg>(A)) return launch_cfg<typename Cfg::Generic>(A, stream);
    }
    static bool attr_set = false;
    if (!attr_set && Cfg::LDS_BYTES > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&fft_pass_kernel<Cfg>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cfg::LDS_BYTES);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    uint32_t grid = (A.ntiles + Cfg::kG - 1) / Cfg::kG * Cfg::kSUB;
    if (grid == 0) return 0;
    if constexpr (Cfg::kPERSIST) {
        // persistent form: as many workgroups as the device holds at once (a multiple of 8, so that a workgroup and the
        // virtual workgroups it walks share an XCD), each walks the tiles with a stride of the grid
        static uint32_t resident = 0;
        if (!resident) {
            int dev = 0, cus = 0, per_cu = 0;
            if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
                hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fft_pass_kernel<Cfg>, Cfg::THREADS, Cfg::LDS_BYTES) != hipSuccess || per_cu < 1)
                return (int)hipErrorLaunchFailure;
            resident = (uint32_t)cus * (uint32_t)per_cu / 8 * 8;
            if (!resident) resident = 8;
        }
        if (grid > resident) grid = resident;
    }
    hipLaunchKernelGGL(fft_pass_kernel<Cfg>, dim3(grid), dim3(Cfg::THREADS), Cfg::LDS_BYTES, stream, A);
    return (int)hipGetLastError();
}

// fft_spectral_kernel (forward transform, pointwise multiplier, inverse transform of complete x lines in one launch): whole tiles,
// one workgroup per G tiles, the dynamic-LDS attribute as for launch_cfg.  TABLES = the part of spectral_<p>.hip (-DDFFT_PART):
// 0 array multiplier, 1 real table multipliers, 2 complex factor tables.  ACC = 1: the accumulating store (PassArgs::acc; parts 3 and 4 =
// TABLES 1 and 2; STORE_TILED_SAME is the one store kind that has a load twin, which the host engine's launch_spectral checks)
template <typename Cfg, int TABLES, int ACC = 0> static int launch_spectral_cfg(const PassArgs &A, hipStream_t stream)
{
    static_assert(!ACC || TABLES != 0, "the array form has no accumulating instantiation");
    static bool attr_set = false;
    if (!attr_set && Cfg::LDS_BYTES > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&fft_spectral_kernel<Cfg, TABLES, ACC>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cfg::LDS_BYTES);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    const uint32_t grid = (A.ntiles + Cfg::kG - 1) / Cfg::kG;
    if (grid == 0) return 0;
    hipLaunchKernelGGL((fft_spectral_kernel<Cfg, TABLES, ACC>), dim3(grid), dim3(Cfg::THREADS), Cfg::LDS_BYTES, stream, A);
    return (int)hipGetLastError();
}
// (spectral_mixed_<p>.hip has several parts per multiplier form and sets DFFT_SPECTRAL_TABLES itself; the accumulating parts of either
// family set both)
#ifndef DFFT_SPECTRAL_TABLES
#define DFFT_SPECTRAL_TABLES DFFT_PART
#endif
#ifndef DFFT_SPECTRAL_ACC
#define DFFT_SPECTRAL_ACC 0
#endif
#define DFFT_CASE_SPECTRAL(n, v, cfg) case n: return launch_spectral_cfg<cfg, DFFT_SPECTRAL_TABLES, DFFT_SPECTRAL_ACC>(A, stream);
#define DFFT_CASE_SPECTRAL_OK(n, v, cfg) case n: return true;

// MODE 1 = R2C (ONEPLANE: 0 two-plane split through LDS, 1 one-plane split, 2 split in registers with the conjugate-pair
// butterfly assignment), MODE 3 = R2C on strided real lines, MODE 2 = C2R (ONEPLANE 2: merge in registers)
template <typename Cfg, int MODE, int ONEPLANE> struct RealKernel;
template <typename Cfg, int ONEPLANE> struct RealKernel<Cfg, 1, ONEPLANE> {
    static constexpr auto kern = &fft_r2c_kernel<Cfg, ONEPLANE>;
    static constexpr size_t lds = RealCfg<Cfg, ONEPLANE>::LDS_BYTES;
};
template <typename Cfg, int ONEPLANE> struct RealKernel<Cfg, 3, ONEPLANE> {      // R2C on strided real lines (Y_Then_ZX y pass)
    static constexpr auto kern = &fft_r2c_kernel<Cfg, ONEPLANE, 1>;
    static constexpr size_t lds = RealCfg<Cfg, ONEPLANE>::LDS_BYTES;
};
template <typename Cfg, int ONEPLANE> struct RealKernel<Cfg, 2, ONEPLANE> {
    static constexpr auto kern = &fft_c2r_kernel<Cfg, ONEPLANE == 2>;
    static constexpr size_t lds = Cfg::LDS_BYTES;
};
template <typename Cfg, int MODE, int ONEPLANE = 0> static int launch_real_cfg(const PassArgs &A, hipStream_t stream)
{
    constexpr auto kern = RealKernel<Cfg, MODE, ONEPLANE>::kern;
    const size_t lds = RealKernel<Cfg, MODE, ONEPLANE>::lds;
    static bool attr_set = false;
    if (!attr_set && lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    const uint32_t grid = (A.ntiles + Cfg::kG - 1) / Cfg::kG;
    if (grid == 0) return 0;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(Cfg::THREADS), lds, stream, A);
    return (int)hipGetLastError();
}

template <typename Cfg> static int launch_bluestein_cfg(const PassArgs &A, hipStream_t stream)
{
    const size_t lds = Cfg::LDS_BYTES;
    static bool attr_set = false;
    if (!attr_set && lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&fft_bluestein_kernel<Cfg>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    if (A.plain && A.NL != (uint32_t)Cfg::kN) return -1;
    // two-level lines: one kernel tile per (tile, sub-line), or per (line, block of TL sub-lines)
    const uint64_t tiles = !A.lv ? A.ntiles : !A.lvqm ? (uint64_t)A.ntiles * A.lvQ : (uint64_t)A.na * A.LB * ((A.lvQ + Cfg::kTL - 1) / Cfg::kTL);
    if ((tiles + Cfg::kG - 1) / Cfg::kG * Cfg::kSUB > 0x7fffffffull) return -1;
    const uint32_t grid = (uint32_t)((tiles + Cfg::kG - 1) / Cfg::kG) * Cfg::kSUB;
    if (grid == 0) return 0;
    hipLaunchKernelGGL(fft_bluestein_kernel<Cfg>, dim3(grid), dim3(Cfg::THREADS), lds, stream, A);
    return (int)hipGetLastError();
}

// The kernel translation units are compiled in parts (-DDFFT_PART=k, see the Makefile) so that a parallel make spreads the
// template instantiations; a part defines a launcher and an info function for its share of a (length, variant) list.
#define DFFT_CAT_(a, b) a##b
#define DFFT_CAT(a, b) DFFT_CAT_(a, b)
// LIST entries are X(N, variant, cfg)
#define DFFT_PASS_FUNCS(LAUNCH, INFO, LIST)                                                          \
    int LAUNCH(int N, int variant, const PassArgs &A, hipStream_t stream)                            \
    {                                                                                                \
        if (variant < 0 || variant > 15) return -1;      /* the key below has four bits for the variant */ \
        switch (N * 16 + variant) { LIST(DFFT_CASE_LAUNCH) }                                         \
        return -1;                                                                                   \
    }                                                                                                \
    bool INFO(int N, int variant, PassInfo *pi)                                                      \
    {                                                                                                \
        if (variant < 0 || variant > 15) return false;                                               \
        switch (N * 16 + variant) { LIST(DFFT_CASE_INFO) }                                           \
        return false;                                                                                \
    }
#define DFFT_CASE_LAUNCH(n, v, cfg) case n * 16 + v: return launch_cfg<cfg>(A, stream);
#define DFFT_CASE_INFO(n, v, cfg) case n * 16 + v: info_cfg<cfg>(pi); return true;
// packed real z passes of the mixed-radix lengths: LIST entries are Y(M, R2C cfg, ONEPLANE, C2R cfg, PAIRED) -- ONEPLANE = 2 / PAIRED = 2:
// Hermitian split / merge in registers (the configuration's last resp. first pass has an even number of butterflies per thread)
#define DFFT_REAL_MIXED_FUNCS(LAUNCH, INFO, LIST)                                                    \
    int LAUNCH(int M, int mode, const PassArgs &A, hipStream_t stream)                               \
    {                                                                                                \
        switch (M) { LIST(DFFT_CASE_REAL) }                                                          \
        return -1;                                                                                   \
    }                                                                                                \
    bool INFO(int M)                                                                                 \
    {                                                                                                \
        switch (M) { LIST(DFFT_CASE_REAL_INFO) }                                                     \
        return false;                                                                                \
    }
#define DFFT_CASE_REAL(n, cfg, op, ccfg, paired) case n: return mode == 1 ? launch_real_cfg<cfg, 1, op>(A, stream) : launch_real_cfg<ccfg, 2, paired>(A, stream);
#define DFFT_CASE_REAL_INFO(n, cfg, op, ccfg, paired) case n: return true;

template <typename Cfg> static void info_cfg(PassInfo *pi)
{
    pi->N = Cfg::kN; pi->E = Cfg::kE; pi->TL = Cfg::kTL; pi->G = Cfg::kG; pi->sub = Cfg::kSUB;
    pi->threads = Cfg::THREADS; pi->lds_bytes = (int)Cfg::LDS_BYTES; pi->npass = Cfg::NPASS;
}
}  // namespace dfft
