// tests/cpp/spectral_factor_check.hip -- host-side emulation of the factor-table forms of fft_spectral_kernel (fft_pass.hip.h; mkind 3, 4, 5 of
// dfft_exec_spectral_op), no GPU needed.  As tests/cpp/spectral_chain_check.hip does for the array and the real-table forms: the kernel's own
// pass_compute / lds_scatter / lds_gather drive the forward chain for every (thread, line) of a workgroup, then the hand-off
// w[spectral_sigma(c)] = spectral_factor_point(v[c], cx[k], line, mkind, sum) with k = t + NT * spectral_sigma(c), line =
// spectral_factor_line(scale, cy, cz) and sum = (tx[k] + sy) + sz -- the two functions the kernel itself calls, so this is the kernel's
// arithmetic and not a restatement of it -- then the second chain, the final conjugation and the store's slot -> output index map.
// Tables: cx over the points and (cy, cz) per line drawn from {+-1, +-i, +-1 +-i}; integer sum tables -3 .. 3 that contain zero sums.
// Each form is compared with N * ifft(fft(x) * m), m = scale * cx * cy * cz * {1, sum, 1 / sum or 0}, by long-double DFTs, for every
// configuration csrc/spectral_f64.hip / spectral_f32.hip instantiates (-DCHAIN_F32: fp32).  Built and run by tests/test_cpu_spectral_factors.py.
#ifdef CHAIN_F32
#include "../../distributedfft_amd/csrc/cfg_f32.hip.h"
#else
#include "../../distributedfft_amd/csrc/cfg_f64.hip.h"
#endif
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <complex>
#include <vector>

using namespace dfft;
typedef std::complex<long double> cld;

static int failures = 0, checked = 0;

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

template <typename Cfg> static void check_cfg(const char *name)
{
    using C = typename Cfg::C;
    using R = typename Cfg::real;
    static_assert(Cfg::kMAP == 0, "line-fastest configurations only");
    constexpr int N = Cfg::kN, E = Cfg::kE, NT = Cfg::NT, TW = Cfg::TW;
    const long double PI = 3.141592653589793238462643383279502884L;
    std::vector<C> W(N);
    for (int j = 0; j < N; j++) { W[j].x = (R)cosl(-2 * PI * j / N); W[j].y = (R)sinl(-2 * PI * j / N); }
    std::vector<cld> x((size_t)TW * N);      // input: line lw, point n
    srand(N * 37 + TW);
    auto rnd = [] { return (long double)(R)(rand() / (double)RAND_MAX - 0.5); };
    for (auto &v : x) v = cld(rnd(), rnd());
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
    // factor tables: cx over the points, (cy, cz) per line -- what the kernel reads at mcx[k], mcy[P.a] and mcz[P.e] -- from the eight
    // values {+-1, +-i, +-1 +-i}; integer sum tables as in spectral_chain_check.hip, the first line's first point a zero sum
    static const R eight[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};
    auto unit = [] { const int i = rand() % 8; return cmake<C>(eight[i][0], eight[i][1]); };
    auto small = [] { return (R)(rand() % 7 - 3); };
    std::vector<C> cx(N), cy(TW), cz(TW);
    std::vector<R> tx(N), sy(TW), sz(TW);
    for (auto &v : cx) v = unit();
    for (auto &v : tx) v = small();
    for (int l = 0; l < TW; l++) { cy[l] = unit(); cz[l] = unit(); sy[l] = small(); sz[l] = small(); }
    sz[0] = -(tx[0] + sy[0]);
    const R scale = (R)0.25;
    for (int kind = 3; kind <= 5; kind++) {
        long zeros = 0;
        for (int tid = 0; tid < Cfg::THREADS; tid++) {
            int lw, t;
            thread_map<Cfg, false>(tid, lw, t);
            const C line = spectral_factor_line<C>(scale, cy[lw], cz[lw]);
            static_for<0, E>([&](auto cc) {
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
}

int main()
{
#ifdef CHAIN_F32
#define CHECK(n) check_cfg<F32_##n>("F32_" #n);
#else
#define CHECK(n) check_cfg<F64_##n>("F64_" #n);
#endif
    CHECK(2) CHECK(4) CHECK(8) CHECK(16) CHECK(32) CHECK(64) CHECK(128) CHECK(256) CHECK(512) CHECK(1024) CHECK(2048)
    printf("%d forms of %d configurations checked, %d failed\n%s\n", checked, checked / 3, failures, failures ? "FAILED" : "ALL OK");
    return failures ? 1 : 0;
}
