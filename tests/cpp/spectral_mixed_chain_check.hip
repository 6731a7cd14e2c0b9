// tests/cpp/spectral_mixed_chain_check.hip -- host-side emulation of the register hand-off of fft_spectral_kernel (fft_pass.hip.h) for the
// mixed-radix configurations of csrc/spectral_mixed.inc (option spectral_op = 2), no GPU needed.  What tests/cpp/spectral_chain_check.hip and
// tests/cpp/spectral_factor_check.hip do for the powers of two: the kernel's own pass_compute / lds_scatter / lds_gather drive the forward
// chain for every (thread, line) of a workgroup, then the hand-off into register spectral_sigma(c), walked in the kernel's own chunks
// (spectral_chunk<Cfg>(): a chunk width that does not cover E, as 4 does not for E = 10, 18, 30, 50, fails here) -- the array form, the two real-table
// forms, and the factor forms (mkind 3, 4, 5) through the kernel's own spectral_factor_point / spectral_factor_line -- the second chain, the
// final conjugation and the store's slot -> output index map.  Each of the six forms is compared with N * ifft(fft(x) * m) by long-double
// DFTs, with the tolerance of those two files.  The configurations are those of the list macros DFFT_F64_SPECTRAL_MIXED /
// DFFT_F32_SPECTRAL_MIXED (-DCHAIN_F32), the ones the launchers switch over; -DCHECK_PARTS=n -DCHECK_PART=k checks every n-th of them.
// Built and run by tests/test_cpu_spectral_mixed_kernel.py.
#include "../../distributedfft_amd/csrc/fft_pass.hip.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <complex>
#include <type_traits>
#include <vector>

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

using namespace dfft;
typedef std::complex<long double> cld;

static int failures = 0, checked = 0, configurations = 0;

template <typename Cfg, int RP, int NS> static void run_pass(std::vector<typename Cfg::C> &regs, const typename Cfg::C *W)
{
    for (int tid = 0; tid < Cfg::THREADS; tid++) {
        int lw, t;
        thread_map<Cfg, false>(tid, lw, t);
        pass_compute<Cfg, RP, NS>(&regs[(size_t)tid * Cfg::kE], t, W);
    }
}
template <typename Cfg, int RP, int NS> static void run_exchange(std::vector<typename Cfg::C> &regs, std::vector<typename Cfg::real> &plane)
{
    static_for<0, 2>([&](auto pc) {
        constexpr int comp = decltype(pc)::value;
        for (int tid = 0; tid < Cfg::THREADS; tid++) {
            int lw, t;
            thread_map<Cfg, false>(tid, lw, t);
            lds_scatter<Cfg, RP, NS, comp>(&regs[(size_t)tid * Cfg::kE], plane.data(), t, lw);
        }
        for (int tid = 0; tid < Cfg::THREADS; tid++) {
            int lw, t;
            thread_map<Cfg, false>(tid, lw, t);
            lds_gather<Cfg, comp>(&regs[(size_t)tid * Cfg::kE], plane.data(), t, lw);
        }
    });
}
template <typename Cfg> static void run_chain(std::vector<typename Cfg::C> &regs, std::vector<typename Cfg::real> &plane, const typename Cfg::C *W)
{
    constexpr int R1 = Cfg::r1, R2 = Cfg::r2, R3 = Cfg::r3, R4 = Cfg::r4;
    run_pass<Cfg, R1, 1>(regs, W);
    if constexpr (R2 > 1) { run_exchange<Cfg, R1, 1>(regs, plane); run_pass<Cfg, R2, R1>(regs, W); }
    if constexpr (R3 > 1) { run_exchange<Cfg, R2, R1>(regs, plane); run_pass<Cfg, R3, R1 * R2>(regs, W); }
    if constexpr (R4 > 1) { run_exchange<Cfg, R3, R1 * R2>(regs, plane); run_pass<Cfg, R4, R1 * R2 * R3>(regs, W); }
}

// forward (sign = -1) or unnormalised inverse (+1) DFT of one line
static std::vector<cld> dft(const std::vector<cld> &x, int sign)
{
    const long double PI = 3.141592653589793238462643383279502884L;
    const int N = (int)x.size();
    std::vector<cld> w(N), X(N);
    for (int j = 0; j < N; j++) w[j] = cld(cosl(2 * PI * j / N), sign * sinl(2 * PI * j / N));
    for (int k = 0; k < N; k++) {
        cld s(0, 0);
        for (int n = 0; n < N; n++) s += x[n] * w[(size_t)((long)k * n % N)];
        X[k] = s;
    }
    return X;
}

// The hand-off visits the registers as the kernel's multiplier loop does: E / CH chunks of CH = spectral_chunk<Cfg>() registers, c = q * CH + j.
// A chunk width that does not divide E leaves registers of the second chain unset: they start as NaN here, and the comparison fails.
template <typename Cfg, typename F> static void walk_chunks(F &&f)
{
    constexpr int CH = spectral_chunk<Cfg>();
    static_for<0, Cfg::kE / CH>([&](auto qq) {
        static_for<0, CH>([&](auto jj) { f(std::integral_constant<int, decltype(qq)::value * CH + decltype(jj)::value>{}); });
    });
}
template <typename C> static void unset(std::vector<C> &regs)
{
    for (auto &v : regs) { v.x = NAN; v.y = NAN; }
}

template <typename Cfg> static void check_cfg(const char *name)
{
    using C = typename Cfg::C;
    using R = typename Cfg::real;
    static_assert(Cfg::kMAP == 0, "line-fastest configurations only");
    constexpr int N = Cfg::kN, E = Cfg::kE, NT = Cfg::NT, TW = Cfg::TW;
    const long double PI = 3.141592653589793238462643383279502884L;
    std::vector<C> W(N);
    for (int j = 0; j < N; j++) { W[j].x = (R)cosl(-2 * PI * j / N); W[j].y = (R)sinl(-2 * PI * j / N); }
    std::vector<cld> x((size_t)TW * N), m((size_t)TW * N);      // input and multiplier: line lw, point n resp. k
    srand(N * 31 + TW);
    auto rnd = [] { return (long double)(R)(rand() / (double)RAND_MAX - 0.5); };
    for (auto &v : x) v = cld(rnd(), rnd());
    for (auto &v : m) v = cld(rnd(), rnd());
    std::vector<C> regs((size_t)Cfg::THREADS * E), next((size_t)Cfg::THREADS * E);
    for (int tid = 0; tid < Cfg::THREADS; tid++) {
        int lw, t;
        thread_map<Cfg, false>(tid, lw, t);
        for (int c = 0; c < E; c++) {          // the kernel's load: register c holds point t + NT*c of the lane's line
            const cld v = x[(size_t)lw * N + t + NT * c];
            regs[(size_t)tid * E + c].x = (R)v.real();
            regs[(size_t)tid * E + c].y = (R)v.imag();
        }
    }
    std::vector<R> plane(Cfg::PLANE_SLOTS + 1, (R)0);
    run_chain<Cfg>(regs, plane, W.data());
    // integer tables for the table forms: tx over the points, (sy, sz) per line -- what the kernel reads at mty[P.a] and mtz[P.e]; zero
    // sums are frequent (values -3 .. 3), and the first line's first point is made one
    std::vector<R> tx(N), sy(TW), sz(TW);
    auto small = [] { return (R)(rand() % 7 - 3); };
    for (auto &v : tx) v = small();
    for (int l = 0; l < TW; l++) { sy[l] = small(); sz[l] = small(); }
    sz[0] = -(tx[0] + sy[0]);
    // form 0: the array, w[sigma(c)] = conj(v[c] * m[t + NT*sigma(c)]); forms 1, 2: the tables, w[sigma(c)] = conj(v[c]) * f with
    // f = scale * sum resp. scale / sum (0 at a zero sum), sum = (tx[t + NT*sigma(c)] + sy) + sz in the kernel's own arithmetic
    for (int form = 0; form < 3; form++) {
        const R scale = form == 1 ? (R)(1.0 / 9.0) : (R)1;
        long zeros = 0;
        unset(next);
        for (int tid = 0; tid < Cfg::THREADS; tid++) {
            int lw, t;
            thread_map<Cfg, false>(tid, lw, t);
            walk_chunks<Cfg>([&](auto cc) {
                constexpr int c = decltype(cc)::value, s = spectral_sigma<Cfg>(c);
                const C v = regs[(size_t)tid * E + c];
                if (form == 0) {
                    const cld mk = m[(size_t)lw * N + t + NT * s];
                    C mm; mm.x = (R)mk.real(); mm.y = (R)mk.imag();
                    const C y = cmul2(v, mm, ci(mm));
                    next[(size_t)tid * E + s].x = y.x;
                    next[(size_t)tid * E + s].y = -y.y;
                } else {
                    const R *txt = tx.data() + t;
                    const R sum = (txt[NT * s] + sy[lw]) + sz[lw];
                    const R f = form == 2 ? (sum != (R)0 ? scale / sum : (R)0) : scale * sum;
                    zeros += sum == (R)0;
                    next[(size_t)tid * E + s].x = v.x * f;
                    next[(size_t)tid * E + s].y = -(v.y * f);
                }
            });
        }
        run_chain<Cfg>(next, plane, W.data());
        constexpr int RL = Cfg::RLAST, S = E / RL;
        double worst = 0, size = 0;
        for (int lw = 0; lw < TW; lw += (TW > 2 ? TW - 1 : 1)) {            // first and last line of the workgroup
            std::vector<cld> X = dft(std::vector<cld>(x.begin() + (size_t)lw * N, x.begin() + (size_t)(lw + 1) * N), -1);
            for (int k = 0; k < N; k++) {
                const long double sum = (long double)tx[k] + (long double)sy[lw] + (long double)sz[lw];
                if (form == 0) X[k] *= m[(size_t)lw * N + k];
                else if (form == 1) X[k] *= sum / 9.0L;
                else X[k] *= sum != 0 ? 1.0L / sum : 0.0L;
            }
            const std::vector<cld> want = dft(X, +1);
            for (int k = 0; k < N; k++) size = std::max(size, (double)std::abs(want[k]));
            for (int tid = 0; tid < Cfg::THREADS; tid++) {
                int l2, t;
                thread_map<Cfg, false>(tid, l2, t);
                if (l2 != lw) continue;
                for (int c = 0; c < E; c++) {      // the kernel's store after the final conjugation
                    const int k = t + NT * (c % S) + brev(c / S, RL) * (N / RL);
                    const C g = next[(size_t)tid * E + c];
                    if (std::isnan(g.x) || std::isnan(g.y)) worst = INFINITY;      // a register the hand-off never wrote
                    worst = std::max(worst, (double)std::abs(want[k] - cld(g.x, -g.y)));
                }
            }
        }
        // two chains: twice the bound of chain_check.hip, relative to the size of the result (|f| <= 1 in the table forms: the
        // factor costs two roundings at most, on values the chains' bound already covers)
        const double tol = 2 * (sizeof(R) == 8 ? 2e-15 : 1e-6) * sqrt((double)N) * log2((double)N) * std::max(1.0, size / sqrt((double)N));
        checked++;
        const bool ok = worst <= tol && (form == 0 || zeros > 0) && size > 0;
        if (!ok) { failures++; printf("%-12s N = %4d  form %d  max abs error %.2e  (bound %.2e), %ld zero sums, result size %.2e  FAIL\n", name, N, form, worst, tol, zeros, size); }
    }
    // factor tables: cx over the points, (cy, cz) per line -- what the kernel reads at mcx[k], mcy[P.a] and mcz[P.e] -- from the eight
    // values {+-1, +-i, +-1 +-i}; the integer sum tables of the forms above
    static const R eight[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};
    auto unit = [] { const int i = rand() % 8; return cmake<C>(eight[i][0], eight[i][1]); };
    std::vector<C> cx(N), cy(TW), cz(TW);
    for (auto &v : cx) v = unit();
    for (int l = 0; l < TW; l++) { cy[l] = unit(); cz[l] = unit(); }
    const R fscale = (R)0.25;
    for (int kind = 3; kind <= 5; kind++) {
        long zeros = 0;
        unset(next);
        for (int tid = 0; tid < Cfg::THREADS; tid++) {
            int lw, t;
            thread_map<Cfg, false>(tid, lw, t);
            const C line = spectral_factor_line<C>(fscale, cy[lw], cz[lw]);
            walk_chunks<Cfg>([&](auto cc) {
                constexpr int c = decltype(cc)::value, s = spectral_sigma<Cfg>(c);
                const int k = t + NT * s;
                const R sum = (tx[k] + sy[lw]) + sz[lw];
                zeros += sum == (R)0;
                next[(size_t)tid * E + s] = spectral_factor_point<C>(regs[(size_t)tid * E + c], cx[k], line, kind, sum);
            });
        }
        run_chain<Cfg>(next, plane, W.data());
        constexpr int RL = Cfg::RLAST, S = E / RL;
        double worst = 0, size = 0;
        for (int lw = 0; lw < TW; lw += (TW > 2 ? TW - 1 : 1)) {            // first and last line of the workgroup
            std::vector<cld> X = dft(std::vector<cld>(x.begin() + (size_t)lw * N, x.begin() + (size_t)(lw + 1) * N), -1);
            for (int k = 0; k < N; k++) {
                const long double sum = (long double)tx[k] + (long double)sy[lw] + (long double)sz[lw];
                const cld P = cld(cx[k].x, cx[k].y) * cld(cy[lw].x, cy[lw].y) * cld(cz[lw].x, cz[lw].y) * 0.25L;
                X[k] *= kind == 3 ? P : kind == 4 ? P * sum : sum != 0 ? P / sum : cld(0, 0);
            }
            const std::vector<cld> want = dft(X, +1);
            for (int k = 0; k < N; k++) size = std::max(size, (double)std::abs(want[k]));
            for (int tid = 0; tid < Cfg::THREADS; tid++) {
                int l2, t;
                thread_map<Cfg, false>(tid, l2, t);
                if (l2 != lw) continue;
                for (int c = 0; c < E; c++) {      // the kernel's store after the final conjugation
                    const int k = t + NT * (c % S) + brev(c / S, RL) * (N / RL);
                    const C g = next[(size_t)tid * E + c];
                    if (std::isnan(g.x) || std::isnan(g.y)) worst = INFINITY;      // a register the hand-off never wrote
                    worst = std::max(worst, (double)std::abs(want[k] - cld(g.x, -g.y)));
                }
            }
        }
        // the tolerance of spectral_chain_check.hip: two chains, relative to the size of the result (the factors are exact in either
        // precision, their product with an integer sum as well; 1 / sum is one rounding)
        const double tol = 2 * (sizeof(R) == 8 ? 2e-15 : 1e-6) * sqrt((double)N) * log2((double)N) * std::max(1.0, size / sqrt((double)N));
        checked++;
        const bool ok = worst <= tol && zeros > 0 && size > 0;
        if (!ok) { failures++; printf("%-12s N = %4d  kind %d  max abs error %.2e  (bound %.2e), %ld zero sums, result size %.2e  FAIL\n", name, N, kind, worst, tol, zeros, size); }
    }
    configurations++;
}

template <typename Cfg, int IDX> static void check_share(const char *name)
{
    if constexpr (IDX % CHECK_PARTS == CHECK_PART) check_cfg<Cfg>(name);
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
