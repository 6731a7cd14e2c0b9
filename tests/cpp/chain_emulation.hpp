// tests/cpp/chain_emulation.hpp -- the one host-side emulation of a workgroup of fft_pass.hip.h that the check programs of this directory
// share (chain_check.hip, spectral_chain_check.hip, spectral_factor_check.hip, spectral_mixed_chain_check.hip), no GPU needed.  The kernel's
// own building blocks -- thread_map, pass_compute (twiddles + butterflies), lds_scatter / lds_gather (the exchange through the padded LDS
// plane), spectral_sigma, spectral_chunk, spectral_factor_point / spectral_factor_line -- are compiled for the host and driven for every
// (thread, line) of a workgroup in program order, with an array standing in for LDS and the loop boundaries standing in for the barriers.
// Two checks: check_chain, one forward chain against a long-double DFT, and check_fused, fft_spectral_kernel's forward chain, hand-off
// w[sigma(c)] = conj(v[c] * m[k]), second chain, final conjugation and store map against N * ifft(fft(x) * m), for the multiplier forms
// mkind 0 .. 5 of dfft_exec_spectral_op.  Forms 0 .. 2 restate the kernel's arithmetic (it has no function of its own for them); forms
// 3 .. 5 call the two functions the kernel itself calls.  The including program brings the configurations and says which forms it runs.
#pragma once
#include "../../distributedfft_amd/csrc/fft_pass.hip.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <complex>
#include <vector>

using namespace dfft;
typedef std::complex<long double> cld;

static int failures = 0, checked = 0;
static const long double PI = 3.141592653589793238462643383279502884L;

// forward (sign = -1) or unnormalised inverse (+1) DFT of one line
static std::vector<cld> dft(const std::vector<cld> &x, int sign)
{
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

// uniform in [-0.5, 0.5), rounded to the precision R
template <typename R> static long double rnd() { return (long double)(R)(rand() / (double)RAND_MAX - 0.5); }

// One workgroup of Cfg: twiddle table, LDS plane and the random input of its TW lines (line lw, point n at x[lw * N + n]); the registers
// of all its threads are one vector, register c of thread tid at regs[tid * E + c].
template <typename Cfg> struct Workgroup {
    using C = typename Cfg::C;
    using R = typename Cfg::real;
    static_assert(Cfg::kMAP == 0, "line-fastest configurations only");
    static constexpr int N = Cfg::kN, E = Cfg::kE, NT = Cfg::NT, TW = Cfg::TW;
    std::vector<C> W = std::vector<C>(N);
    std::vector<R> plane = std::vector<R>(Cfg::PLANE_SLOTS + 1, (R)0);
    std::vector<cld> x = std::vector<cld>((size_t)TW * N);

    Workgroup()
    {
        for (int j = 0; j < N; j++) W[j] = cmake<C>((R)cosl(-2 * PI * j / N), (R)sinl(-2 * PI * j / N));
        srand(N * 31 + TW);
        for (auto &v : x) v = cld(rnd<R>(), rnd<R>());
    }
    // f(tid, lw, t) for every thread of the workgroup: its line and its position on the line
    template <typename F> static void threads(F &&f)
    {
        for (int tid = 0; tid < Cfg::THREADS; tid++) {
            int lw, t;
            thread_map<Cfg, false>(tid, lw, t);
            f(tid, lw, t);
        }
    }
    // the kernel's load: register c holds point t + NT*c of the lane's line
    std::vector<C> load() const
    {
        std::vector<C> regs((size_t)Cfg::THREADS * E);
        threads([&](int tid, int lw, int t) {
            for (int c = 0; c < E; c++) {
                const cld v = x[(size_t)lw * N + t + NT * c];
                regs[(size_t)tid * E + c] = cmake<C>((R)v.real(), (R)v.imag());
            }
        });
        return regs;
    }
    template <int RP, int NS> void pass(std::vector<C> &regs) const
    {
        threads([&](int tid, int, int t) { pass_compute<Cfg, RP, NS>(&regs[(size_t)tid * E], t, W.data()); });
    }
    template <int RP, int NS> void exchange(std::vector<C> &regs)
    {
        static_for<0, 2>([&](auto pc) {
            constexpr int comp = decltype(pc)::value;
            threads([&](int tid, int lw, int t) { lds_scatter<Cfg, RP, NS, comp>(&regs[(size_t)tid * E], plane.data(), t, lw); });
            threads([&](int tid, int lw, int t) { lds_gather<Cfg, comp>(&regs[(size_t)tid * E], plane.data(), t, lw); });
        });
    }
    // the passes and exchanges of one transform, in program order
    void chain(std::vector<C> &regs)
    {
        constexpr int R1 = Cfg::r1, R2 = Cfg::r2, R3 = Cfg::r3, R4 = Cfg::r4;
        pass<R1, 1>(regs);
        if constexpr (R2 > 1) { exchange<R1, 1>(regs); pass<R2, R1>(regs); }
        if constexpr (R3 > 1) { exchange<R2, R1>(regs); pass<R3, R1 * R2>(regs); }
        if constexpr (R4 > 1) { exchange<R3, R1 * R2>(regs); pass<R4, R1 * R2 * R3>(regs); }
    }
    // The hand-off of fft_spectral_kernel: next[sigma(c)] = point(v[c], lw, k), k = t + NT * sigma(c), visiting the registers as the
    // kernel's multiplier loop does, E / CH chunks of CH = spectral_chunk<Cfg>() registers, c = q * CH + j.  A chunk width that does not
    // cover E leaves registers of the second chain unset: they start as NaN here, and the comparison fails.
    template <typename F> static std::vector<C> hand_off(const std::vector<C> &regs, F &&point)
    {
        constexpr int CH = spectral_chunk<Cfg>();
        std::vector<C> next(regs.size(), cmake<C>((R)NAN, (R)NAN));
        threads([&](int tid, int lw, int t) {
            static_for<0, E / CH>([&](auto qq) {
                static_for<0, CH>([&](auto jj) {
                    constexpr int c = decltype(qq)::value * CH + decltype(jj)::value, s = spectral_sigma<Cfg>(c);
                    next[(size_t)tid * E + s] = point(regs[(size_t)tid * E + c], lw, t + NT * s);
                });
            });
        });
        return next;
    }
    // the kernel's store: register c = i + mr*S of thread t holds output k = t + NT*i + brev(mr, RL)*(N/RL); f(k, value) for line lw
    template <typename F> static void outputs(const std::vector<C> &regs, int lw, F &&f)
    {
        constexpr int RL = Cfg::RLAST, S = E / RL;
        threads([&](int tid, int l2, int t) {
            if (l2 != lw) return;
            for (int c = 0; c < E; c++) f(t + NT * (c % S) + brev(c / S, RL) * (N / RL), regs[(size_t)tid * E + c]);
        });
    }
    // First and last line of the workgroup against want(line lw of x), the registers conjugated first where conj is set: the largest
    // error and the largest |want|.  A NaN among the outputs -- a register the hand-off never wrote -- is an infinite error.
    template <typename F> void compare(const std::vector<C> &regs, bool conj, F &&want, double &worst, double &size) const
    {
        worst = size = 0;
        for (int lw = 0; lw < TW; lw += (TW > 2 ? TW - 1 : 1)) {
            const std::vector<cld> X = want(std::vector<cld>(x.begin() + (size_t)lw * N, x.begin() + (size_t)(lw + 1) * N), lw);
            for (int k = 0; k < N; k++) size = std::max(size, (double)std::abs(X[k]));
            outputs(regs, lw, [&](int k, C g) {
                if (std::isnan(g.x) || std::isnan(g.y)) worst = INFINITY;
                worst = std::max(worst, (double)std::abs(X[k] - cld(g.x, conj ? -g.y : g.y)));
            });
        }
    }
    // the bound of one chain; two chains have twice that, relative to the size of the result (the multiplier costs two roundings at
    // most, on values the chains' bound already covers: |f| <= 1 in the table forms, exact factors, one rounding for 1 / sum)
    static double tolerance() { return (sizeof(R) == 8 ? 2e-15 : 1e-6) * sqrt((double)N) * log2((double)N); }
    static double tolerance(double size) { return 2 * tolerance() * std::max(1.0, size / sqrt((double)N)); }
};

static void report(const char *name, int N, const char *what, bool ok, double worst, double tol, long zeros, double size)
{
    checked++;
    if (ok) return;
    failures++;
    printf("%-14s N = %4d  %s  max abs error %.2e  (bound %.2e), %ld zero sums, result size %.2e  FAIL\n", name, N, what, worst, tol, zeros, size);
}

// one forward chain against the DFT
template <typename Cfg> static void check_chain(const char *name)
{
    Workgroup<Cfg> wg;
    auto regs = wg.load();
    wg.chain(regs);
    double worst, size;
    wg.compare(regs, false, [](const std::vector<cld> &line, int) { return dft(line, -1); }, worst, size);
    report(name, Cfg::kN, "one chain", worst <= wg.tolerance(), worst, wg.tolerance(), 0, size);
}

// The multipliers of one workgroup for the six forms (mkind of dfft_exec_spectral_op), as the kernel finds them: the array m (line lw,
// point k); integer sum tables tx over the points and (sy, sz) per line -- what the kernel reads at mty[P.a] and mtz[P.e] -- with values
// -3 .. 3, so zero sums are frequent, and the first line's first point is made one; factor tables cx over the points and (cy, cz) per line
// from the eight values {+-1, +-i, +-1 +-i}, with line[lw] = spectral_factor_line(0.25, cy, cz).  Scales: 1, 1/9, 1 and 0.25 for kinds 3 .. 5.
template <typename Cfg> struct Multipliers {
    using C = typename Cfg::C;
    using R = typename Cfg::real;
    static constexpr int N = Cfg::kN, TW = Cfg::TW;
    std::vector<cld> m = std::vector<cld>((size_t)TW * N);
    std::vector<R> tx = std::vector<R>(N), sy = std::vector<R>(TW), sz = std::vector<R>(TW);
    std::vector<C> cx = std::vector<C>(N), cy = std::vector<C>(TW), cz = std::vector<C>(TW), line = std::vector<C>(TW);

    Multipliers()
    {
        static const R eight[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};
        auto small = [] { return (R)(rand() % 7 - 3); };
        auto unit = [] { const int i = rand() % 8; return cmake<C>(eight[i][0], eight[i][1]); };
        for (auto &v : m) v = cld(rnd<R>(), rnd<R>());
        for (auto &v : tx) v = small();
        for (int l = 0; l < TW; l++) { sy[l] = small(); sz[l] = small(); }
        sz[0] = -(tx[0] + sy[0]);
        for (auto &v : cx) v = unit();
        for (int l = 0; l < TW; l++) { cy[l] = unit(); cz[l] = unit(); line[l] = spectral_factor_line<C>((R)0.25, cy[l], cz[l]); }
    }
    R sum(int lw, int k) const { return (tx[k] + sy[lw]) + sz[lw]; }      // in the kernel's own arithmetic
    static C conj_times(C v, R f) { return cmake<C>(v.x * f, -(v.y * f)); }
    // the point the second chain starts from, conj(v * m[k]), per form
    C array(C v, int lw, int k) const
    {
        const cld mk = m[(size_t)lw * N + k];
        const C mm = cmake<C>((R)mk.real(), (R)mk.imag()), y = cmul2(v, mm, ci(mm));
        return cmake<C>(y.x, -y.y);
    }
    C times_sum(C v, int lw, int k) const { return conj_times(v, (R)(1.0 / 9.0) * sum(lw, k)); }
    C over_sum(C v, int lw, int k) const { const R s = sum(lw, k); return conj_times(v, s != (R)0 ? (R)1 / s : (R)0); }
    template <int KIND> C factor(C v, int lw, int k) const { return spectral_factor_point<C>(v, cx[k], line[lw], KIND, sum(lw, k)); }
    // the same multipliers in long double
    long double lsum(int lw, int k) const { return (long double)tx[k] + (long double)sy[lw] + (long double)sz[lw]; }
    cld P(int lw, int k) const { return cld(cx[k].x, cx[k].y) * cld(cy[lw].x, cy[lw].y) * cld(cz[lw].x, cz[lw].y) * 0.25L; }
    cld ref_array(int lw, int k) const { return m[(size_t)lw * N + k]; }
    cld ref_times_sum(int lw, int k) const { return lsum(lw, k) / 9.0L; }
    cld ref_over_sum(int lw, int k) const { const long double s = lsum(lw, k); return s != 0 ? 1.0L / s : 0.0L; }
    cld ref_factor(int lw, int k) const { return P(lw, k); }
    cld ref_factor_times_sum(int lw, int k) const { return P(lw, k) * lsum(lw, k); }
    cld ref_factor_over_sum(int lw, int k) const { const long double s = lsum(lw, k); return s != 0 ? P(lw, k) / s : cld(0, 0); }

    struct Form {
        C (Multipliers::*point)(C, int, int) const;
        cld (Multipliers::*reference)(int, int) const;
    };
    static Form form(int kind)
    {
        static const Form forms[6] = {{&Multipliers::array, &Multipliers::ref_array},
                                      {&Multipliers::times_sum, &Multipliers::ref_times_sum},
                                      {&Multipliers::over_sum, &Multipliers::ref_over_sum},
                                      {&Multipliers::template factor<3>, &Multipliers::ref_factor},
                                      {&Multipliers::template factor<4>, &Multipliers::ref_factor_times_sum},
                                      {&Multipliers::template factor<5>, &Multipliers::ref_factor_over_sum}};
        return forms[kind];
    }
};

// fft_spectral_kernel for the forms first .. last against N * ifft(fft(x) * m).  Every table and factor form must have met a zero sum.
template <typename Cfg> static void check_fused(const char *name, int first, int last)
{
    using C = typename Cfg::C;
    Workgroup<Cfg> wg;
    const Multipliers<Cfg> mult;
    auto regs = wg.load();
    wg.chain(regs);
    for (int kind = first; kind <= last; kind++) {
        const auto form = mult.form(kind);
        long zeros = 0;
        auto next = wg.hand_off(regs, [&](C v, int lw, int k) {
            zeros += kind != 0 && mult.sum(lw, k) == 0;
            return (mult.*form.point)(v, lw, k);
        });
        wg.chain(next);
        double worst, size;
        wg.compare(next, true, [&](const std::vector<cld> &line, int lw) {
            std::vector<cld> X = dft(line, -1);
            for (int k = 0; k < Cfg::kN; k++) X[k] *= (mult.*form.reference)(lw, k);
            return dft(X, +1);
        }, worst, size);
        const bool ok = worst <= wg.tolerance(size) && (kind == 0 || zeros > 0) && size > 0;
        static const char *const what[6] = {"form 0", "form 1", "form 2", "kind 3", "kind 4", "kind 5"};
        report(name, Cfg::kN, what[kind], ok, worst, wg.tolerance(size), zeros, size);
    }
}
