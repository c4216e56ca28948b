// Running feature statistics of the Frechet distance on the device: raw_mean[D] += sum_r x_r and
// raw_cov[D][D] += X^T X in fp64, in place (reference metrics/metric_utils.py:109-124 `FeatureStats.append`:
// every batch copied to the host, widened and multiplied there as `x64.T @ x64` in numpy).
//
// xtx_kernel: a workgroup (256 threads, 2 x 2 waves) owns a 64 x 64 tile of the covariance and walks all n
// rows of the batch, so an element has one owner and one summation order whatever the grid: no atomics, two
// runs agree bitwise. A wave holds 2 x 2 tiles of v_mfma_f64_16x16x4_f64 (4 rows of X per step); both
// operands are row segments of X read straight from global memory (lane l: row r0 + (l >> 4), column
// c0 + (l & 15): 16 consecutive columns of 4 rows, 128-B segments) and widened to fp64 in registers --
// products of widened fp32 / fp16 values are exact in fp64, only the additions round. The batch is small
// (n x D against the D x D tile traffic), so it is served from L2 and no LDS stage is needed.
// C/D layout of the f64 MFMA: col = lane & 15, row = (lane >> 4) + 4 reg.
// colsum_kernel: one thread per column, rows in ascending order.
#include "vfm_common.h"

namespace {

using namespace vfm;

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int TB = 64, NT = 256;

__device__ __forceinline__ double widen(const float* p) { return (double)*p; }
__device__ __forceinline__ double widen(const __half* p) { return (double)__half2float(*p); }

template <class T>
__global__ __launch_bounds__(NT) void xtx_kernel(const T* __restrict__ x, long long ld, int n, int D,
                                                 double* __restrict__ cov) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, kk = lane >> 4;
    const int i0 = blockIdx.y * TB + 32 * (wave & 1), j0 = blockIdx.x * TB + 32 * (wave >> 1);
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{};
    const bool iok[2] = {i0 + c < D, i0 + 16 + c < D}, jok[2] = {j0 + c < D, j0 + 16 + c < D};
    for (int r0 = 0; r0 < n; r0 += 4) {
        const int r = r0 + kk;
        const T* row = x + (long long)r * ld;
        double a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = (r < n && iok[i]) ? widen(row + i0 + 16 * i + c) : 0.0;
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = (r < n && jok[j]) ? widen(row + j0 + 16 * j + c) : 0.0;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = i0 + 16 * i + kk + 4 * e, col = j0 + 16 * j + c;
                if (row < D && col < D) cov[(long long)row * D + col] += acc[i][j][e];
            }
}

template <class T>
__global__ __launch_bounds__(NT) void colsum_kernel(const T* __restrict__ x, long long ld, int n, int D,
                                                    double* __restrict__ mean) {
    const int col = blockIdx.x * NT + threadIdx.x;
    if (col >= D) return;
    double s = 0.0;
    for (int r = 0; r < n; ++r) s += widen(x + (long long)r * ld + col);
    mean[col] += s;
}

template <class T>
int launch(const void* x, long long ld, int n, int D, double* raw_mean, double* raw_cov, hipStream_t st) {
    const unsigned tiles = (unsigned)((D + TB - 1) / TB);
    VFM_LAUNCH(colsum_kernel<T>, dim3((unsigned)((D + NT - 1) / NT)), dim3(NT), 0, st, static_cast<const T*>(x), ld, n, D,
               raw_mean);
    VFM_LAUNCH(xtx_kernel<T>, dim3(tiles, tiles), dim3(NT), 0, st, static_cast<const T*>(x), ld, n, D, raw_cov);
    return launch_status();
}

}  // namespace

extern "C" int vfm_feature_stats_accum(const void* x, int dtype, long long ld, int n, int D, double* raw_mean,
                                       double* raw_cov, void* stream) {
    if (!x || !raw_mean || !raw_cov || n < 0 || D < 1 || ld < D) return VFM_ERR_ARGS;
    if (D > 65535 * TB) return VFM_ERR_ARGS;                   // the tile grid's y extent
    if (dtype != VFM_F32 && dtype != VFM_F16) return VFM_NO_KERNEL;
    if (n == 0) return VFM_OK;
    hipStream_t st = (hipStream_t)stream;
    return dtype == VFM_F32 ? launch<float>(x, ld, n, D, raw_mean, raw_cov, st)
                            : launch<__half>(x, ld, n, D, raw_mean, raw_cov, st);
}
