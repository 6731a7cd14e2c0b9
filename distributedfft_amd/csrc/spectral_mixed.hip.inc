// spectral_mixed.hip.inc -- the body of spectral_mixed_f64.hip / spectral_mixed_f32.hip: one object per (multiplier form, share of the length
// list), chosen by the Makefile with -DDFFT_SPECTRAL_TABLES=<form> -DDFFT_SHARE=<share> (form 0: the array multiplier, 1: the real table
// multipliers, 2: the complex factor tables, mkind 3 .. 5; share: DFFT_<P>_SPECTRAL_MIXED<share> of spectral_mixed.inc).  The accumulating twins
// of forms 1 and 2 (PassArgs::acc, dfft_exec_spectral_sum) are objects of their own: -DDFFT_SPECTRAL_ACC=1 -DDFFT_SM_FORM=3|4 next to
// -DDFFT_SPECTRAL_TABLES=1|2; DFFT_SM_FORM names the object's launcher and defaults to the multiplier form.  The object of form 0,
// share 0 also holds the entry points.  The including file defines DFFT_MIXED_<P>, DFFT_SM_P (f64 | f32), DFFT_SM_LIST (the list macro) and
// DFFT_SM_AXIS (the prefix of the axis pass's own configurations, F64_M | F32_M).
#if !defined(DFFT_SPECTRAL_TABLES) || !defined(DFFT_SHARE) || DFFT_SPECTRAL_TABLES < 0 || DFFT_SPECTRAL_TABLES > 2
#error "compile with -DDFFT_SPECTRAL_TABLES=0|1|2 -DDFFT_SHARE=<share>"
#endif
#ifndef DFFT_SM_FORM
#define DFFT_SM_FORM DFFT_SPECTRAL_TABLES
#endif
#if defined(DFFT_SPECTRAL_ACC) && DFFT_SPECTRAL_ACC && (DFFT_SPECTRAL_TABLES == 0 || DFFT_SM_FORM != DFFT_SPECTRAL_TABLES + 2)
#error "the accumulating objects are forms 3 (tables 1) and 4 (tables 2)"
#endif
#include "kernels.hip.inc"

namespace dfft {
#include "kernels_mixed.inc"
#include "spectral_mixed.inc"

#define DFFT_SM_NAME_(p, f, s) launch_spectral_mixed_##p##_##f##_##s
#define DFFT_SM_NAME(p, f, s) DFFT_SM_NAME_(p, f, s)
#define DFFT_SM_SHARES DFFT_CAT(DFFT_SM_LIST, _FOREACH_SHARE)

// dfft_exec_spectral_op checks the 32-bit lane offsets of the array form with G and NT = N / E of the AXIS pass's configuration
// (pass_info) where G == 1 (G > 1: 64-bit addresses per lane, nothing to check): a configuration of this kernel's own keeps that check
// valid while it has the same G and, at G == 1, no more threads per line
#define DFFT_SM_CHECK(n, v, cfg) static_assert(cfg::kG == DFFT_CAT(DFFT_SM_AXIS, n)::kG && (cfg::kG != 1 || cfg::NT <= DFFT_CAT(DFFT_SM_AXIS, n)::NT) && \
                                               cfg::kTL == DFFT_CAT(DFFT_SM_AXIS, n)::kTL && cfg::kSUB == 1 && cfg::kMAP == 0, #cfg);
DFFT_SM_LIST(DFFT_SM_CHECK)

int DFFT_SM_NAME(DFFT_SM_P, DFFT_SM_FORM, DFFT_SHARE)(int N, const PassArgs &A, hipStream_t stream)
{
    switch (N) { DFFT_CAT(DFFT_SM_LIST, DFFT_SHARE)(DFFT_CASE_SPECTRAL) }
    return -1;
}
#if DFFT_SPECTRAL_TABLES == 0 && DFFT_SHARE == 0
#define DFFT_SM_DECL(s) int DFFT_SM_NAME(DFFT_SM_P, 1, s)(int, const PassArgs &, hipStream_t); int DFFT_SM_NAME(DFFT_SM_P, 2, s)(int, const PassArgs &, hipStream_t); \
                        int DFFT_SM_NAME(DFFT_SM_P, 0, s)(int, const PassArgs &, hipStream_t); \
                        int DFFT_SM_NAME(DFFT_SM_P, 3, s)(int, const PassArgs &, hipStream_t); int DFFT_SM_NAME(DFFT_SM_P, 4, s)(int, const PassArgs &, hipStream_t);
DFFT_SM_SHARES(DFFT_SM_DECL)
int DFFT_CAT(launch_spectral_mixed_, DFFT_SM_P)(int N, const PassArgs &A, hipStream_t stream)
{
    int r = -1;      // the share that has the length answers; -1: no share has it
#define DFFT_SM_TRY(s) if (r == -1) r = A.acc ? (A.mkind <= 2 ? DFFT_SM_NAME(DFFT_SM_P, 3, s)(N, A, stream) : DFFT_SM_NAME(DFFT_SM_P, 4, s)(N, A, stream)) \
                                        : A.mkind == 0 ? DFFT_SM_NAME(DFFT_SM_P, 0, s)(N, A, stream) : A.mkind <= 2 ? DFFT_SM_NAME(DFFT_SM_P, 1, s)(N, A, stream) \
                                                                                                          : DFFT_SM_NAME(DFFT_SM_P, 2, s)(N, A, stream);
    DFFT_SM_SHARES(DFFT_SM_TRY)
    return r;
}
bool DFFT_CAT(spectral_mixed_supported_, DFFT_SM_P)(int N)
{
    switch (N) { DFFT_SM_LIST(DFFT_CASE_SPECTRAL_OK) }
    return false;
}
#endif
}  // namespace dfft
