// execSpectralSum through include/mpicufft_amd.hpp: the divergence of a vector field, three inputs with the factor tables i*kx, i*ky, i*kz
// (kind 3, the Nyquist entries zeroed: an R2C plan) summed into one output in one call.  Compared with the sum of three execSpectralOp
// results on the same plan, taken on the host in the same order: the inverse half is linear, so the two differ by rounding alone
// (held to 1e-12 of the result's rms in fp64; a dropped or doubled term misses that by eleven orders of magnitude).  With one input the
// call is compared with memcmp against execSpectralOp.  Single MPI rank.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mpicufft_amd.hpp"

int main(int argc, char **argv)
{
    MPI_Init(&argc, &argv);
    int world_size;
    MPI_Comm_size(MPI_COMM_WORLD, &world_size);
    const size_t Nx = 16, Ny = 12, Nz = 10, N[3] = {Nx, Ny, Nz};
    hipSetDevice(0);
    Configurations config{true, 0, All2All, Sync, "../benchmarks", All2All, Sync};
    MPIcuFFT_Pencil_Opt1<double> *fft = new MPIcuFFT_Pencil_Opt1<double>(config, MPI_COMM_WORLD, world_size);
    fft->setOption("spectral_op", 1);
    fft->setOption("spectral_inputs", 3);
    Pencil_Partition partition(1, 1);
    GlobalSize global_size(Nx, Ny, Nz);
    fft->initFFT(&global_size, &partition, true);
    size_t isize[3], osize[3];
    fft->getInSize(isize);
    fft->getOutSize(osize);
    const size_t n = isize[0] * isize[1] * isize[2], bytes = n * sizeof(double);
    std::vector<double> in_h[3];
    unsigned long long s = 88172645463325252ull;
    for (int d = 0; d < 3; d++) {
        in_h[d].resize(n);
        for (size_t i = 0; i < n; i++) {
            s ^= s << 13; s ^= s >> 7; s ^= s << 17;
            in_h[d][i] = 255.0 * (double)(s >> 11) / 9007199254740992.0 - 127.5;
        }
    }
    // i * k_d in the wrapped order, 0 at the Nyquist point; the z table holds kz = 0 .. Nz / 2 of the R2C spectrum
    std::vector<std::complex<double>> t[3];
    for (int d = 0; d < 3; d++) {
        t[d].resize(osize[d]);
        for (size_t k = 0; k < osize[d]; k++) {
            const double w = 2 * k < N[d] ? (double)k : 2 * k == N[d] ? 0.0 : (double)k - (double)N[d];
            t[d][k] = std::complex<double>(0.0, w);
        }
    }
    double *in_d[3], *sum_d, *one_d, *single_d[3];
    void *tab_d[3];
    for (int d = 0; d < 3; d++) {
        hipMalloc((void **)&in_d[d], bytes);
        hipMemcpy(in_d[d], in_h[d].data(), bytes, hipMemcpyHostToDevice);
        hipMalloc(&tab_d[d], t[d].size() * sizeof(t[d][0]));
        hipMemcpy(tab_d[d], t[d].data(), t[d].size() * sizeof(t[d][0]), hipMemcpyHostToDevice);
        hipMalloc((void **)&single_d[d], bytes); hipMemset(single_d[d], 0xFF, bytes);
    }
    hipMalloc((void **)&sum_d, bytes); hipMemset(sum_d, 0xFF, bytes);
    hipMalloc((void **)&one_d, bytes); hipMemset(one_d, 0xFF, bytes);
    dfft_spectral_op ops[3];
    memset(ops, 0, sizeof(ops));
    for (int d = 0; d < 3; d++) {
        ops[d].kind = 3;
        ops[d].scale = 1.0 / (double)(Nx * Ny * Nz);
        (d == 0 ? ops[d].cx : d == 1 ? ops[d].cy : ops[d].cz) = tab_d[d];
    }
    hipDeviceSynchronize();
    const void *ins[3] = {in_d[0], in_d[1], in_d[2]};
    fft->execSpectralSum(sum_d, ins, ops, 3);
    fft->execSpectralSum(one_d, ins + 1, ops + 1, 1);
    for (int d = 0; d < 3; d++) fft->execSpectralOp(single_d[d], in_d[d], ops[d]);
    int bad = 0;
    std::vector<double> got(n), a(n), want(n, 0.0);
    for (int d = 0; d < 3; d++) {
        hipMemcpy(a.data(), in_d[d], bytes, hipMemcpyDeviceToHost);
        if (memcmp(a.data(), in_h[d].data(), bytes)) { printf("input %d was modified\n", d); bad = 1; }
        hipMemcpy(a.data(), single_d[d], bytes, hipMemcpyDeviceToHost);
        double rms = 0;
        for (size_t i = 0; i < n; i++) { want[i] += a[i]; rms += a[i] * a[i]; }
        printf("term %d: rms %.6e\n", d, std::sqrt(rms / (double)n));
        if (!(rms > 0)) bad = 1;
        if (d == 1) {
            hipMemcpy(got.data(), one_d, bytes, hipMemcpyDeviceToHost);
            const bool same = memcmp(got.data(), a.data(), bytes) == 0;
            printf("one input: %s\n", same ? "identical" : "DIFFERENT");
            if (!same) bad = 1;
        }
    }
    hipMemcpy(got.data(), sum_d, bytes, hipMemcpyDeviceToHost);
    double err = 0, rms = 0;
    bool finite = true;
    for (size_t i = 0; i < n; i++) {
        finite = finite && std::isfinite(got[i]);
        err += (got[i] - want[i]) * (got[i] - want[i]); rms += want[i] * want[i];
    }
    const double rel = std::sqrt(err / rms);
    printf("divergence: %s, rms %.6e, relative difference %.3e, %s\n", finite ? "finite" : "NOT FINITE", std::sqrt(rms / (double)n), rel,
           rel <= 1e-12 ? "within 1e-12" : "TOO LARGE");
    if (!finite || !(rms > 0) || !(rel <= 1e-12)) bad = 1;
    delete fft;
    for (int d = 0; d < 3; d++) { hipFree(in_d[d]); hipFree(tab_d[d]); hipFree(single_d[d]); }
    hipFree(sum_d); hipFree(one_d);
    MPI_Finalize();
    printf(bad ? "FAILED\n" : "spectral sum ok\n");
    return bad;
}
