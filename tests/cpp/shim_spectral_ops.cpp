// execSpectralOps through include/mpicufft_amd.hpp: two operators on one input in one call (a Laplacian-like sum of tables and its
// reciprocal), each output compared with memcmp against execSpectralOp with the same operator on the same plan.  Single MPI rank.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mpicufft_amd.hpp"

int main(int argc, char **argv)
{
    MPI_Init(&argc, &argv);
    int world_size;
    MPI_Comm_size(MPI_COMM_WORLD, &world_size);
    const size_t Nx = 16, Ny = 12, Nz = 10;
    hipSetDevice(0);
    Configurations config{true, 0, All2All, Sync, "../benchmarks", All2All, Sync};
    MPIcuFFT_Pencil_Opt1<double> *fft = new MPIcuFFT_Pencil_Opt1<double>(config, MPI_COMM_WORLD, world_size);
    fft->setOption("spectral_op", 1);
    fft->setOption("spectral_outputs", 2);
    Pencil_Partition partition(1, 1);
    GlobalSize global_size(Nx, Ny, Nz);
    fft->initFFT(&global_size, &partition, true);
    size_t isize[3], osize[3];
    fft->getInSize(isize);
    fft->getOutSize(osize);
    const size_t n = isize[0] * isize[1] * isize[2], bytes = n * sizeof(double);
    std::vector<double> in_h(n);
    unsigned long long s = 88172645463325252ull;
    for (size_t i = 0; i < n; i++) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        in_h[i] = 255.0 * (double)(s >> 11) / 9007199254740992.0 - 127.5;
    }
    // -k^2 per axis; the z table holds kz = 0 .. Nz / 2 of the R2C spectrum
    std::vector<double> t[3];
    for (int d = 0; d < 3; d++) {
        const size_t N = d == 0 ? Nx : d == 1 ? Ny : Nz;
        t[d].resize(osize[d]);
        for (size_t k = 0; k < osize[d]; k++) {
            const double w = (double)(k < N - k ? k : N - k);
            t[d][k] = -w * w;
        }
    }
    double *in_d, *tab_d[3], *multi_d[2], *single_d[2];
    hipMalloc((void **)&in_d, bytes);
    hipMemcpy(in_d, in_h.data(), bytes, hipMemcpyHostToDevice);
    for (int d = 0; d < 3; d++) {
        hipMalloc((void **)&tab_d[d], t[d].size() * sizeof(double));
        hipMemcpy(tab_d[d], t[d].data(), t[d].size() * sizeof(double), hipMemcpyHostToDevice);
    }
    for (int j = 0; j < 2; j++) {
        hipMalloc((void **)&multi_d[j], bytes); hipMemset(multi_d[j], 0xFF, bytes);
        hipMalloc((void **)&single_d[j], bytes); hipMemset(single_d[j], 0xFF, bytes);
    }
    dfft_spectral_op ops[2];
    memset(ops, 0, sizeof(ops));
    for (int j = 0; j < 2; j++) {
        ops[j].kind = 1 + j;      // the sum of the tables, and its reciprocal
        ops[j].scale = 1.0 / (double)(Nx * Ny * Nz);
        ops[j].ax = tab_d[0]; ops[j].ay = tab_d[1]; ops[j].az = tab_d[2];
    }
    hipDeviceSynchronize();
    void *outs[2] = {multi_d[0], multi_d[1]};
    fft->execSpectralOps(outs, in_d, ops, 2);
    for (int j = 0; j < 2; j++) fft->execSpectralOp(single_d[j], in_d, ops[j]);
    int bad = 0;
    std::vector<double> a(n), b(n), in_after(n);
    hipMemcpy(in_after.data(), in_d, bytes, hipMemcpyDeviceToHost);
    if (memcmp(in_after.data(), in_h.data(), bytes)) { printf("the input was modified\n"); bad = 1; }
    for (int j = 0; j < 2; j++) {
        hipMemcpy(a.data(), multi_d[j], bytes, hipMemcpyDeviceToHost);
        hipMemcpy(b.data(), single_d[j], bytes, hipMemcpyDeviceToHost);
        double sum = 0;
        bool finite = true;
        for (size_t i = 0; i < n; i++) { finite = finite && std::isfinite(a[i]); sum += std::fabs(a[i]); }
        const bool same = memcmp(a.data(), b.data(), bytes) == 0;
        printf("output %d: %s, sum |x| = %.6e, %s\n", j, finite ? "finite" : "NOT FINITE", sum, same ? "identical" : "DIFFERENT");
        if (!finite || !same || !(sum > 0)) bad = 1;
    }
    // the two operators are not the same one: their outputs differ
    hipMemcpy(a.data(), multi_d[0], bytes, hipMemcpyDeviceToHost);
    hipMemcpy(b.data(), multi_d[1], bytes, hipMemcpyDeviceToHost);
    if (!memcmp(a.data(), b.data(), bytes)) { printf("both outputs are the same\n"); bad = 1; }
    delete fft;
    hipFree(in_d);
    for (int d = 0; d < 3; d++) hipFree(tab_d[d]);
    for (int j = 0; j < 2; j++) { hipFree(multi_d[j]); hipFree(single_d[j]); }
    MPI_Finalize();
    printf(bad ? "FAILED\n" : "spectral ops ok\n");
    return bad;
}
