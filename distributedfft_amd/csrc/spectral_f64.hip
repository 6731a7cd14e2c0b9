// spectral_f64.hip -- fft_spectral_kernel (fft_pass.hip.h), f64: the fused forward-multiply-inverse x pass of dfft_exec_spectral_op for the
// power-of-two lengths 2 .. 2048, each with the default (variant 0) configuration of its length.  Compiled in three parts (-DDFFT_PART =
// 0: the array multiplier and the entry points, 1: the real table multipliers, 2: the complex factor tables, mkind 3 .. 5), and two more
// for the accumulating store of dfft_exec_spectral_sum (PassArgs::acc): 3 = the kernels of part 1, 4 = those of part 2, with ACC = 1.
// The mixed-radix x lengths of option spectral_op = 2 are spectral_mixed_f64.hip's, in libdfft_amd_any.so.
#if DFFT_PART == 3 || DFFT_PART == 4
#define DFFT_SPECTRAL_TABLES (DFFT_PART - 2)
#define DFFT_SPECTRAL_ACC 1
#endif
#include "cfg_f64.hip.h"

namespace dfft {
#define DFFT_F64_SPECTRAL(X) X(2, 0, F64_2) X(4, 0, F64_4) X(8, 0, F64_8) X(16, 0, F64_16) X(32, 0, F64_32) X(64, 0, F64_64) \
    X(128, 0, F64_128) X(256, 0, F64_256) X(512, 0, F64_512) X(1024, 0, F64_1024) X(2048, 0, F64_2048)
int launch_spectral_f64_p0(int N, const PassArgs &A, hipStream_t stream);
int launch_spectral_f64_p1(int N, const PassArgs &A, hipStream_t stream);
int launch_spectral_f64_p2(int N, const PassArgs &A, hipStream_t stream);
int launch_spectral_f64_p3(int N, const PassArgs &A, hipStream_t stream);
int launch_spectral_f64_p4(int N, const PassArgs &A, hipStream_t stream);
#if DFFT_PART == 0
int launch_spectral_f64_p0(int N, const PassArgs &A, hipStream_t stream)
{
    switch (N) { DFFT_F64_SPECTRAL(DFFT_CASE_SPECTRAL) }
    return -1;
}
int launch_spectral_f64(int N, const PassArgs &A, hipStream_t stream)
{
    if (A.acc) return A.mkind <= 2 ? launch_spectral_f64_p3(N, A, stream) : launch_spectral_f64_p4(N, A, stream);
    return A.mkind == 0 ? launch_spectral_f64_p0(N, A, stream) : A.mkind <= 2 ? launch_spectral_f64_p1(N, A, stream) : launch_spectral_f64_p2(N, A, stream);
}
bool spectral_supported_f64(int N)
{
    switch (N) { DFFT_F64_SPECTRAL(DFFT_CASE_SPECTRAL_OK) }
    return false;
}
#elif DFFT_PART == 1
int launch_spectral_f64_p1(int N, const PassArgs &A, hipStream_t stream)
{
    switch (N) { DFFT_F64_SPECTRAL(DFFT_CASE_SPECTRAL) }
    return -1;
}
#elif DFFT_PART == 2
int launch_spectral_f64_p2(int N, const PassArgs &A, hipStream_t stream)
{
    switch (N) { DFFT_F64_SPECTRAL(DFFT_CASE_SPECTRAL) }
    return -1;
}
#elif DFFT_PART == 3
int launch_spectral_f64_p3(int N, const PassArgs &A, hipStream_t stream)
{
    switch (N) { DFFT_F64_SPECTRAL(DFFT_CASE_SPECTRAL) }
    return -1;
}
#elif DFFT_PART == 4
int launch_spectral_f64_p4(int N, const PassArgs &A, hipStream_t stream)
{
    switch (N) { DFFT_F64_SPECTRAL(DFFT_CASE_SPECTRAL) }
    return -1;
}
#else
#error "DFFT_PART must be 0 .. 4"
#endif
}  // namespace dfft
