// Positional and relative uncertainty from a block's rigorous variance matrix where it sits in HBM (uncertainty.h: the math).
// Both kernels are gathers: per lane 6 (station) or 24 (pair) doubles of the lower triangle at scattered addresses, then ~100 flops.
// They are bound by the latency of those loads, and one launch per block covers all of the block's stations (or pairs).
#include <hip/hip_runtime.h>

#include "../../include/dnagpu.h"
#include "uncertainty.h"

namespace dnagpu {
namespace {

constexpr int UN_THREADS = 256;

__global__ __launch_bounds__(UN_THREADS) void station_uncertainty_kernel(const double* __restrict__ S, uint32_t ld,
                                                                         const uint32_t* __restrict__ idx, const double* __restrict__ latlon,
                                                                         double* __restrict__ out, uint32_t count) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    double c6[6];
    un::gather_station(S, ld, idx[t], c6);
    un::uncertainty_3x3(c6, latlon[2 * (size_t)t], latlon[2 * (size_t)t + 1], out + (size_t)un::RECORD_DOUBLES * t);
}

__global__ __launch_bounds__(UN_THREADS) void pair_uncertainty_kernel(const double* __restrict__ S, uint32_t ld,
                                                                      const uint32_t* __restrict__ idx, const double* __restrict__ latlon,
                                                                      double* __restrict__ out, uint32_t count) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    double c6[6];
    un::gather_pair(S, ld, idx[2 * (size_t)t], idx[2 * (size_t)t + 1], c6);
    un::uncertainty_3x3(c6, latlon[2 * (size_t)t], latlon[2 * (size_t)t + 1], out + (size_t)un::RECORD_DOUBLES * t);
}

}  // namespace

void launch_station_uncertainty(const double* S, uint32_t ld, const uint32_t* idx, const double* latlon, double* out, uint32_t count,
                                hipStream_t st) {
    if (!count) return;
    station_uncertainty_kernel<<<(count + UN_THREADS - 1) / UN_THREADS, UN_THREADS, 0, st>>>(S, ld, idx, latlon, out, count);
}

void launch_pair_uncertainty(const double* S, uint32_t ld, const uint32_t* idx, const double* latlon, double* out, uint32_t count,
                             hipStream_t st) {
    if (!count) return;
    pair_uncertainty_kernel<<<(count + UN_THREADS - 1) / UN_THREADS, UN_THREADS, 0, st>>>(S, ld, idx, latlon, out, count);
}

}  // namespace dnagpu

static_assert(sizeof(dnagpu_uncertainty) == dnagpu::un::RECORD_DOUBLES * sizeof(double), "dnagpu_uncertainty is RECORD_DOUBLES doubles");

extern "C" void dnagpu_debug_uncertainty_3x3(const double cxyz[6], double lat, double lon, dnagpu_uncertainty* out) {
    if (!cxyz || !out) return;
    dnagpu::un::uncertainty_3x3(cxyz, lat, lon, reinterpret_cast<double*>(out));
}
