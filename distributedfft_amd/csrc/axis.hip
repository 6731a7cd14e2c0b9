// axis.hip -- the axis layer (axis.hpp): the per-precision table of kernel entry points, the plan of one axis and its device tables, and
// the launch of one pass over its lines.  Host code; the kernels themselves are in kernels_*.hip, real_*.hip, spectral_*.hip and, for
// every length that is not a power of two up to 8192, behind any_loader.hip.
#include "axis.hpp"

#include <math.h>
#include <stdlib.h>
#include <algorithm>
#include <complex>
#include <vector>

#include "host_common.hpp"

namespace dfft {

static const Kernels kKernels[2] = {
    {launch_pass_f64, pass_info_f64, launch_real_f64, real_supported_f64, launch_bluestein_f64, launch_spectral_f64, spectral_supported_f64,
     launch_spectral_mixed_f64, spectral_mixed_supported_f64, 16, TL_F64},
    {launch_pass_f32, pass_info_f32, launch_real_f32, real_supported_f32, launch_bluestein_f32, launch_spectral_f32, spectral_supported_f32,
     launch_spectral_mixed_f32, spectral_mixed_supported_f32, 8, TL_F32}};
const Kernels &kernels(int prec) { return kKernels[prec == DFFT_F64 ? 0 : 1]; }

bool pass_info(int prec, int N, PassInfo *pi) { return kernels(prec).pass_info(N, 0, pi); }
bool has_variant(int prec, const Axis &ax, int role, PassInfo *pi)
{
    PassInfo own;
    return !ax.bluestein && kernels(prec).pass_info((int)ax.N, role, pi ? pi : &own);
}

#ifdef DFFT_EXPERIMENTS
// A/B build only (make exp): DFFT_EXP_F32_TWIDDLES=1 rounds every fp64 table -- tw, twN, tw_zr, the Bluestein chirp and bhat
// (upload_table) -- through fp32: the defect the per-entry forward bound of tests/parity_metric.py has to catch
// (profiles/r6_f32_twiddle_proof.txt, profiles/entry_parity_mutation.txt); the shipped library has no such switch
static const bool f32_tw = [] { const char *e = getenv("DFFT_EXP_F32_TWIDDLES"); return e && atoi(e) != 0; }();
#else
constexpr bool f32_tw = false;
#endif

static const long double PI = 3.141592653589793238462643383279502884L;

// a device table of n complex entries value(j), evaluated in long double and rounded once to the precision's element
template <typename F> static int upload_table(int prec, size_t n, F value, void **dev)
{
    const size_t esz = kernels(prec).esz;
    std::vector<char> host(esz * n);
    for (size_t j = 0; j < n; j++) {
        const std::complex<long double> v = value(j);
        if (prec == DFFT_F64) {
            double *d = reinterpret_cast<double *>(host.data()) + 2 * j;
            d[0] = (double)v.real(); d[1] = (double)v.imag();
            if (f32_tw) { d[0] = (double)(float)d[0]; d[1] = (double)(float)d[1]; }
        } else {
            float *d = reinterpret_cast<float *>(host.data()) + 2 * j;
            d[0] = (float)v.real(); d[1] = (float)v.imag();
        }
    }
    HIP_TRY(hipMalloc(dev, host.size()));
    HIP_TRY(hipMemcpy(*dev, host.data(), host.size(), hipMemcpyHostToDevice));
    return 0;
}

int make_twiddles(int prec, size_t N, void **dev)
{
    return upload_table(prec, N, [N](size_t j) {
        const long double a = -2.0L * PI * (long double)j / (long double)N;
        return std::complex<long double>(cosl(a), sinl(a));
    }, dev);
}

static void host_fft_pow2(std::vector<std::complex<long double>> &a)
{
    const size_t n = a.size();
    for (size_t i = 1, j = 0; i < n; i++) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        for (size_t i = 0; i < n; i += len)
            for (size_t k = 0; k < len / 2; k++) {
                long double ang = -2.0L * PI * (long double)k / (long double)len;
                std::complex<long double> w(cosl(ang), sinl(ang));
                auto u = a[i + k], v = a[i + k + len / 2] * w;
                a[i + k] = u + v;
                a[i + k + len / 2] = u - v;
            }
    }
}

void axis_free(Axis &a)
{
    for (void **t : {&a.tw, &a.chirp, &a.bhat, &a.twN}) if (*t) { (void)hipFree(*t); *t = nullptr; }
    for (auto &l : a.lv) axis_free(l);
}

// Two-level plan of an axis: N = N1*N2 with both factors within reach of the generic kernel -- a power of two up to 8192 (plain
// chain) or any length F with a Bluestein inner transform of next_pow2(2F-1) <= 8192 points.  The cheapest split by a model of
// the launches' cost in passes over the data: plain 1 (2 on the sub-tile workgroups of 4096 / 8192 points), Bluestein 1.5 plus
// the padding ratio M/F.  Largest N: 2^24 (32-bit point indices in the kernel).
static bool axis_plan_two_level(int prec, size_t N, Axis &a)
{
    a.N = N;
    if (N < 4 || N > ((size_t)1 << 24)) return false;
    PassInfo pi;
    auto level_cost = [&](size_t F, bool &blue, size_t &M) -> double {
        if (is_pow2(F) && F <= 8192 && pass_info(prec, (int)F, &pi)) { blue = false; M = F; return F > 2048 ? 2.0 : 1.0; }
        M = next_pow2(2 * F - 1);
        if (F < 2 || M > 8192 || !pass_info(prec, (int)M, &pi)) return -1.0;
        blue = true;
        return 1.5 + (double)M / (double)F + (M > 2048 ? 2.0 : 0.0);
    };
    double best = -1.0;
    size_t b1 = 0;
    for (size_t n1 = 2; n1 * n1 <= N; n1++) {
        if (N % n1) continue;
        for (size_t f : {n1, N / n1}) {
            bool bl1, bl2; size_t m1, m2;
            const double c1 = level_cost(f, bl1, m1), c2 = level_cost(N / f, bl2, m2);
            if (c1 < 0 || c2 < 0) continue;
            // ties: the smaller largest inner transform, then the longer second level (its scratch reads are contiguous)
            const double c = c1 + c2 + 1e-6 * (double)std::max(m1, m2) + (f > N / f ? 1e-9 : 0.0);
            if (best < 0 || c < best) { best = c; b1 = f; }
        }
    }
    if (best < 0) return false;
    a.two = true; a.bluestein = true; a.M = 0;
    a.lv.assign(2, Axis());
    const size_t f[2] = {b1, N / b1};
    for (int k = 0; k < 2; k++) {
        bool bl; size_t M;
        level_cost(f[k], bl, M);
        a.lv[k].N = f[k]; a.lv[k].bluestein = bl; a.lv[k].M = M;
    }
    return true;
}

// Long Bluestein plan: any length up to 2^23 whose padded length M = next_pow2(2N - 1) <= 2^24 runs as a two-level line
static bool axis_plan_long(int prec, size_t N, Axis &a)
{
    a = Axis();
    a.N = N;
    if (N < 2) return false;
    const size_t M = next_pow2(2 * N - 1);
    if (M > ((size_t)1 << 24)) return false;
    Axis inner;
    if (!axis_plan_two_level(prec, M, inner)) return false;
    a.longb = true; a.bluestein = true; a.two = false; a.M = M;
    a.lv.assign(1, inner);
    return true;
}

bool axis_plan_bluestein(int prec, size_t N, Axis &a, int two_level)
{
    PassInfo pi;
    a.N = N;
    if (two_level == 1 && axis_plan_two_level(prec, N, a)) return true;
    const size_t M = next_pow2(2 * N - 1);
    if (N < 2 || M > 8192 || !pass_info(prec, (int)M, &pi)) return axis_plan_two_level(prec, N, a) || axis_plan_long(prec, N, a);
    a.bluestein = true; a.M = M;
    return true;
}

bool axis_plan(int prec, size_t N, Axis &a, bool mixed, int two_level)
{
    PassInfo pi;
    a.N = N;
    if (two_level == 1 && axis_plan_two_level(prec, N, a)) return true;
    // native chain: powers of two 2..8192 and the mixed-radix lengths of kernels_mixed.inc (2^a 3^b 5^c 7^d <= 2048)
    if ((is_pow2(N) || mixed) && N <= 8192 && pass_info(prec, (int)N, &pi)) { a.bluestein = false; a.M = N; return true; }
    return axis_plan_bluestein(prec, N, a);      // (the two-level attempt above need not be repeated)
}

int axis_upload(int prec, Axis &a)
{
    if (a.two) {
        for (auto &l : a.lv) TRY(axis_upload(prec, l));
        if (!a.twN) TRY(make_twiddles(prec, a.N, &a.twN));
        return 0;
    }
    if (a.longb) TRY(axis_upload(prec, a.lv[0]));
    else if (!a.tw) TRY(make_twiddles(prec, a.M, &a.tw));
    if (a.bluestein && !a.chirp) {
        const size_t N = a.N, M = a.M;
        std::vector<std::complex<long double>> ch(N), b(M, std::complex<long double>(0, 0));
        for (size_t n = 0; n < N; n++) {
            const size_t q = (size_t)(((unsigned __int128)n * n) % (2 * N));      // n^2 mod 2N keeps the angle exact
            const long double ang = PI * (long double)q / (long double)N;
            ch[n] = std::complex<long double>(cosl(ang), -sinl(ang));           // exp(-i pi n^2 / N)
            b[n] = std::conj(ch[n]);
            if (n) b[M - n] = std::conj(ch[n]);
        }
        host_fft_pow2(b);
        for (auto &v : b) v /= (long double)M;
        TRY(upload_table(prec, N, [&](size_t j) { return ch[j]; }, &a.chirp));
        TRY(upload_table(prec, M, [&](size_t j) { return b[j]; }, &a.bhat));
    }
    return 0;
}

// one launch of the generic kernel for the lines (or sub-lines) of `ax`: plain chain or Bluestein
static int launch_generic(int prec, const Axis &ax, PassArgs &A, hipStream_t s)
{
    A.tw = ax.tw; A.tw2 = ax.chirp; A.tw3 = ax.bhat; A.NL = (uint32_t)ax.N; A.plain = ax.bluestein ? 0 : 1;
    return kernels(prec).launch_bluestein((int)ax.M, A, s);
}

// The scratch between the two levels N1, N2 of a line whose level 1 loads natural lines (q1) / whose level 2 stores them (q2): lanes
// over the lines of a tile, or over neighbouring sub-lines of one line where the level's outer side has natural lines; the scratch
// layout that keeps both levels in runs (fft_pass.hip.h)
static void level_layout(PassArgs &A, bool q1, bool q2, uint32_t N1, uint32_t N2, int TL)
{
    if (!q1 && !q2) { A.lvlay = 0; A.lvs1 = N2 * (uint32_t)TL; A.lvs2 = (uint32_t)TL; }
    else if (q1) { A.lvlay = 1; A.lvs1 = N2; A.lvs2 = 1; }
    else { A.lvlay = 1; A.lvs1 = 1; A.lvs2 = N1; }
}

// two-level line (fft_pass.hip.h): level 1 through the pass's load form into the scratch, level 2 from the scratch through its
// store form.  real_mode / NK as for a one-launch generic pass.
static int launch_two_level(int prec, const Axis &ax, PassArgs A, int real_mode, size_t NK, void *scratch, int TL, hipStream_t s)
{
    A.lvN = (uint32_t)ax.N; A.lvNK = (uint32_t)NK; A.NK = (uint32_t)NK; A.real_mode = real_mode; A.lvtw = ax.twN; A.lvw = scratch;
    const bool q1 = A.load_kind == LOAD_LINES, q2 = A.store_kind == STORE_LINES;
    level_layout(A, q1, q2, (uint32_t)ax.lv[0].N, (uint32_t)ax.lv[1].N, TL);
    for (int level = 1; level <= 2; level++) {
        PassArgs B = A;
        B.lv = level; B.lvQ = (uint32_t)ax.lv[2 - level].N; B.lvqm = level == 1 ? q1 : q2;
        const int r = launch_generic(prec, ax.lv[level - 1], B, s);
        if (r != 0) return fail(r == -1 ? ERR_UNSUPPORTED : r, "two-level pass launch failed for length " + std::to_string(ax.N));
    }
    return 0;
}

// Long Bluestein pass (fft_pass.hip.h, PassArgs::lb): X = ch * IFFT_M(FFT_M(x * ch, zero-padded) * bhat), the two M-point transforms
// as two-level lines.  Launch 1 reads the pass's own load form (chirp and padding on the fly), launch 4 writes its own store form
// (chirp on the fly), so unpack / pack / transposes stay fused as for every other pass; between them the line lives in a scratch of
// natural M-point lines (S2) and the two-level scratch (S1).  The inverse M-point transform is the forward one between re <-> im
// swaps; an inverse PASS swaps at its own two ends (PassArgs::swap of launches 1 and 4) like every inverse pass.
//   1  level 1, pass's load form -> S1   lb = 1: x[n] * ch[n], 0 beyond the line          2  level 2, S1 -> S2 natural, * bhat, swapped
//   3  level 1, S2 natural -> S1                                                           4  level 2, S1 -> pass's store form: swap, * ch
static int launch_long_bluestein(int prec, const Axis &ax, const PassArgs &P, int real_mode, size_t NK, void *scratch, int TL, hipStream_t s)
{
    const Axis &in = ax.lv[0];      // the two-level plan of M
    const uint32_t M = (uint32_t)ax.M, N1 = (uint32_t)in.lv[0].N, N2 = (uint32_t)in.lv[1].N;
    char *S1 = static_cast<char *>(scratch), *S2 = S1 + (size_t)P.ntiles * (size_t)TL * M * kernels(prec).esz;
    auto level = [&](PassArgs B, int lv, bool qm) {
        B.lvN = M; B.lvNK = M; B.lvtw = in.twN; B.lvw = S1; B.lv = lv; B.lvQ = (uint32_t)in.lv[2 - lv].N; B.lvqm = qm ? 1 : 0;
        const int r = launch_generic(prec, in.lv[lv - 1], B, s);
        return r == 0 ? 0 : fail(r == -1 ? ERR_UNSUPPORTED : r, "long Bluestein launch failed for length " + std::to_string(ax.N));
    };
    // natural M-point lines in S2 for the same tiles
    auto natural_side = [&](PassArgs &B, bool store) {
        if (store) { B.store_kind = STORE_LINES; B.out = S2; B.KS_out = 0; B.AS_out = 0; B.stab = nullptr; B.sseg = nullptr; B.snseg = 0; B.suni = 0; B.shift = 0; }
        else { B.load_kind = LOAD_LINES; B.in = S2; B.KS_in = 0; B.AS_in = 0; B.ltab = nullptr; B.lseg = nullptr; B.lnseg = 0; B.luni = 0; }
    };
    const bool qin = P.load_kind == LOAD_LINES, qout = P.store_kind == STORE_LINES;      // (as launch_two_level decides)
    {   // forward M-point transform: pass's load form -> S2
        PassArgs A = P;
        A.shift = 0;
        natural_side(A, true);
        level_layout(A, qin, true, N1, N2, TL);
        PassArgs L1 = A;
        L1.lb = 1; L1.lbL = (uint32_t)ax.N; L1.lbK = (uint32_t)NK; L1.lbtab = ax.chirp; L1.real_mode = real_mode;      // (swap: the pass's)
        TRY(level(L1, 1, qin));
        PassArgs L2 = A;
        L2.lb = 2; L2.lbL = M; L2.lbK = M; L2.lbtab = ax.bhat; L2.real_mode = 0; L2.swap = 1;
        TRY(level(L2, 2, true));
    }
    {   // inverse M-point transform: S2 -> pass's store form
        PassArgs A = P;
        natural_side(A, false);
        level_layout(A, true, qout, N1, N2, TL);
        PassArgs L3 = A;
        L3.lb = 0; L3.real_mode = 0; L3.swap = 0; L3.shift = 0;
        natural_side(L3, true);      // (its store side is the scratch S1: unused, but must not carry the pass's tables)
        L3.out = nullptr;
        TRY(level(L3, 1, true));
        PassArgs L4 = A;
        L4.lb = 6; L4.lbL = (uint32_t)ax.N; L4.lbK = (uint32_t)NK; L4.lbtab = ax.chirp; L4.real_mode = real_mode;      // (swap: the pass's)
        TRY(level(L4, 2, qout));
    }
    return 0;
}

// every line of the launch's tiles: N points between the two levels; long Bluestein: M points in each of S1 and S2
size_t axis_scratch_bytes(int prec, const Axis &ax, const PassArgs &A, int TL)
{
    return (size_t)A.ntiles * (size_t)TL * (ax.longb ? 2 * ax.M : ax.two ? ax.N : 0) * kernels(prec).esz;
}

int launch_axis(int prec, const Axis &ax, PassArgs &A, int variant, int real_mode, size_t NK, void *scratch, size_t scratch_bytes, int TL,
                hipStream_t stream)
{
    if (!ax.bluestein) {
        if (real_mode) return fail(ERR_UNSUPPORTED, "real pass without a packed or Bluestein plan");      // (dfft_init rules this out)
        if (variant && !has_variant(prec, ax, variant)) variant = 0;      // a length without a configuration for the role: the default
        const int r = kernels(prec).launch_pass((int)ax.N, variant, A, stream);
        if (r == -1) return fail(ERR_UNSUPPORTED, "unsupported line length " + std::to_string(ax.N));
        return r == 0 ? 0 : fail(r, std::string("kernel launch failed: ") + hipGetErrorString((hipError_t)r));
    }
    if (ax.longb || ax.two) {
        if (axis_scratch_bytes(prec, ax, A, TL) > scratch_bytes)
            return fail(ERR_STATE, ax.longb ? "long Bluestein pass: scratch region too small" : "two-level pass: scratch region too small");
        return ax.longb ? launch_long_bluestein(prec, ax, A, real_mode, NK, scratch, TL, stream)
                        : launch_two_level(prec, ax, A, real_mode, NK, scratch, TL, stream);
    }
    A.NK = (uint32_t)NK; A.real_mode = real_mode;
    const int r = launch_generic(prec, ax, A, stream);
    if (r != 0) return fail(r == -1 ? ERR_UNSUPPORTED : r, "Bluestein pass launch failed for length " + std::to_string(ax.N));
    return 0;
}

// the fused x pass has the default configuration of the powers of two 2 .. 2048 (csrc/spectral_*.hip) and, with value 2, the
// mixed-radix lengths of csrc/spectral_mixed.inc (kernels of libdfft_amd_any.so); no unfused fallback.  The refusals in the order
// dfft_init reports them: value 1, a Bluestein / two-level axis, the second library's symbols, no such length
int spectral_kernel_for(int prec, const Axis &x, int option_value, std::string *why)
{
    const Kernels &K = kernels(prec);
    const int Nx = (int)x.N;
    const bool pow2 = is_pow2(x.N);
    if (!x.bluestein && pow2 && K.spectral_supported(Nx)) return SPECTRAL_CORE;
    const std::string len = "an x length of " + std::to_string(Nx) + " points";
    const std::string has = " (spectral_op = 2: powers of two from 2 to 2048 and the mixed-radix lengths 2^a 3^b 5^c 7^d up to 2000 that "
                            "dfft_spectral_op_supported reports, on a native chain)";
    std::string no, lib;
    if (option_value == 1)
        no = "spectral_op: " + len + " has no fused forward-multiply-inverse kernel (powers of two from 2 to 2048 on a native chain)";
    else if (x.bluestein)
        no = "spectral_op: " + len + " runs the Bluestein / two-level kernel in this plan, which has no fused forward-multiply-inverse form" + has;
    else if (!pow2 && !any_spectral_mixed_available(&lib))
        no = "spectral_op: the fused kernel of " + len + " is one of libdfft_amd_any.so: " + lib;
    else if (pow2 || !K.spectral_mixed_supported(Nx))
        no = "spectral_op: " + len + " has no fused forward-multiply-inverse kernel" + has;
    else
        return SPECTRAL_ANY;
    if (why) *why = no;
    return SPECTRAL_NONE;
}

}  // namespace dfft
