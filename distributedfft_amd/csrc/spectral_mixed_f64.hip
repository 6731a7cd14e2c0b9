// spectral_mixed_f64.hip -- fft_spectral_kernel (fft_pass.hip.h), f64: the fused forward-multiply-inverse x pass of dfft_exec_spectral_op for
// the mixed-radix lengths of spectral_mixed.inc (option spectral_op = 2); kernels of libdfft_amd_any.so.  One object per multiplier form and
// share of the list (spectral_mixed.hip.inc; the Makefile's NSH_f64 is the number of shares).
#define DFFT_MIXED_F64
#define DFFT_SM_P f64
#define DFFT_SM_LIST DFFT_F64_SPECTRAL_MIXED
#define DFFT_SM_AXIS F64_M
#include "spectral_mixed.hip.inc"
