// axis.hpp -- the axis layer of libdfft_amd.so (axis.hip): how the lines of one axis are planned (native chain, Bluestein, two levels,
// long Bluestein), which tables they need and how one pass over them is launched.  The only place that picks a kernel entry point by
// precision: everything above it (dfft.hip, tune.hip) goes through kernels(prec) or the functions below.
#pragma once
#include "plan.hpp"

namespace dfft {

// the entry points of one precision (dfft_internal.hpp: the *_f64 / *_f32 functions), its element size and the lines of its tiles
struct Kernels {
    int (*launch_pass)(int N, int variant, const PassArgs &A, hipStream_t stream);
    bool (*pass_info)(int N, int variant, PassInfo *pi);
    int (*launch_real)(int M, int mode, int variant, const PassArgs &A, hipStream_t stream);
    bool (*real_supported)(int M);
    int (*launch_bluestein)(int M, const PassArgs &A, hipStream_t stream);
    int (*launch_spectral)(int N, const PassArgs &A, hipStream_t stream);
    bool (*spectral_supported)(int N);
    int (*launch_spectral_mixed)(int N, const PassArgs &A, hipStream_t stream);
    bool (*spectral_mixed_supported)(int N);
    size_t esz;
    int TL;
};
const Kernels &kernels(int prec);

bool pass_info(int prec, int N, PassInfo *pi);      // the default configuration of length N, if there is one
// does the length of a native axis have a kernel configuration for this role (PassRole / variant number)?  (*pi: that configuration)
bool has_variant(int prec, const Axis &ax, int role, PassInfo *pi = nullptr);

// twiddle table exp(-2*pi*i*j/N) on the device, evaluated in long double, rounded once
int make_twiddles(int prec, size_t N, void **dev);

// decide how an axis of length N is transformed; returns false if unsupported.  mixed: the mixed-radix lengths run the native chain;
// two_level: 0 = only lengths with no other plan, 1 = wherever a split exists (tests, A/B runs)
bool axis_plan(int prec, size_t N, Axis &a, bool mixed = true, int two_level = 0);
// Bluestein even for a power of two: its kernel is the one with a strided real-line load (Y_Then_ZX) and the real modes;
// lengths beyond its reach in two levels (the generic kernel again, real modes included)
bool axis_plan_bluestein(int prec, size_t N, Axis &a, int two_level = 0);
int axis_upload(int prec, Axis &a);      // the device tables of the plan that are not there yet
void axis_free(Axis &a);

// One pass over the lines of `ax`: the native chain in configuration `variant`, long Bluestein, two levels or the one-launch generic
// kernel.  real_mode / NK: real lines on one side, the NK = N/2 + 1 points of the Hermitian half on the other (0 / N: complex; generic
// kernel only).  scratch: scratch_bytes >= axis_scratch_bytes(...) between the levels of a two-level or long Bluestein line (else unused)
int launch_axis(int prec, const Axis &ax, PassArgs &A, int variant, int real_mode, size_t NK, void *scratch, size_t scratch_bytes, int TL,
                hipStream_t stream);
size_t axis_scratch_bytes(int prec, const Axis &ax, const PassArgs &A, int TL);

// The fused forward-multiply-inverse x pass (fft_spectral_kernel) of x axis `x` under option spectral_op = option_value: a kernel of this
// library (powers of two), of libdfft_amd_any.so (mixed radix, value 2), or none -- then *why says so, in dfft_init's words
enum SpectralKernel { SPECTRAL_NONE = 0, SPECTRAL_CORE = 1, SPECTRAL_ANY = 2 };
int spectral_kernel_for(int prec, const Axis &x, int option_value, std::string *why);

}  // namespace dfft
