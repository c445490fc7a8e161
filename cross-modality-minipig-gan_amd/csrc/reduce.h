// Fixed-order block reductions: the ONE place a wave or block sum of the loss, metric, norm-finalize and optimiser
// kernels is written.  Each helper's comment states its order of additions; "bitwise reproducible" anywhere in those
// kernels means that order, a launch geometry that depends on the sizes alone, and no floating-point atomics.
// (The conv kernels' partial-wave folds over their own lane layouts stay with those kernels.)
#pragma once
#include <hip/hip_runtime.h>

namespace mpgan {

// Order: xor butterfly over the 64 lanes, offsets 32, 16, 8, 4, 2, 1; every lane ends with the same bits.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// 256 threads.  Order: wave_sum, lane 0 of wave w stores sh[w], barrier, ((sh[0] + sh[1]) + sh[2]) + sh[3]; every
// thread gets the sum.  REUSE adds the barrier behind the reads that a caller needs before it writes sh again.
template <bool REUSE = false, typename T>
__device__ __forceinline__ T block_sum4(T v, T* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const T r = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  if (REUSE) __syncthreads();
  return r;
}

// 256 threads, N <= 16 values each, through LDS (a dozen wave_sums per block cost more LDS cycles in their cross-lane
// permutes than this costs in all).  Order: thread t stores sh[j * 256 + t] = v[j], barrier; thread t < 16 N, with
// j = t / 16 and p = t % 16, adds sh[j * 256 + p], sh[j * 256 + p + 16], .. sh[j * 256 + p + 240] in that order (onto 0),
// then the 16 lanes of a value fold by xor butterfly, offsets 8, 4, 2, 1.  Returns the sum of value t / 16 in the
// threads t < 16 N (all 16 lanes of a value hold the same bits) and 0 in the others.  sh holds 256 * N values.
template <int N, typename T>
__device__ __forceinline__ T block_sum_n(const T (&v)[N], T* sh) {
  static_assert(N >= 1 && N <= 16, "16 lanes per value");
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < N; ++j) sh[j * 256 + t] = v[j];
  __syncthreads();
  T s = T(0);
  if (t < 16 * N) {
    const T* p = sh + (t >> 4) * 256 + (t & 15);
#pragma unroll
    for (int i = 0; i < 16; ++i) s += p[i * 16];
  }
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  return s;
}

// N threads, N a power of two.  Order: red[tid] = v, then for s = N/2, N/4, .. 1: red[tid] += red[tid + s] for
// tid < s, a barrier behind every level; returns red[0].  LEAD puts a barrier in front, for a red that the block may
// still be reading (a second sum through the same array).
template <int N, bool LEAD = false>
__device__ __forceinline__ double block_tree_sum(double v, double* red) {
  const int tid = threadIdx.x;
  if (LEAD) __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = N / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// Two sums at once through two arrays, one barrier per level: each sum's order is block_tree_sum<N>'s.
template <int N>
__device__ __forceinline__ void block_tree_sum2(double& a, double& b, double* ra, double* rb) {
  const int tid = threadIdx.x;
  ra[tid] = a;
  rb[tid] = b;
  __syncthreads();
  for (int s = N / 2; s > 0; s >>= 1) {
    if (tid < s) { ra[tid] += ra[tid + s]; rb[tid] += rb[tid + s]; }
    __syncthreads();
  }
  a = ra[0];
  b = rb[0];
}

// 256 threads over n values.  Order: thread t adds x[t], x[t + 256], .. in index order into sh[t], barrier, thread 0
// adds sh[0 .. 255] in index order.  The sum is thread 0's alone.
template <typename T>
__device__ __forceinline__ double strided_serial_sum256(const T* __restrict__ x, int n, double* sh) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)x[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int i = 0; i < 256; ++i) t += sh[i];
  return t;
}

// The tail of a tiled pair loss (loss_ops.hip), two launches: item[i] = block_tree_sum<256>(tile partials of item i,
// thread t taking slots t, t + 256, ..) * inv, then over the items in item order the sum of item[i] (ONE_MINUS: of
// 1.0 - item[i]) as its mean (reduction 0), as it is (1), or per batch entry the mean over its channels (2).
void launch_loss_tail(const double* partials, long tiles, double inv, double* item, int items, int channels,
                      int reduction, bool one_minus, float* loss, hipStream_t stream);

// The tail of a tiled pair loss whose items have a divisor of their own, found on the device (masked SSIM): per item
// n = the sum of its int64 tile counts (integers: no order to fix), s = its tile partials by the order above,
// stats[i] = (s / n, n) and NaN for n == 0; then over the items the sum of 1.0 - s / n, 0 for n == 0, as above.
void launch_counted_loss_tail(const double* partials, const long long* counts, long tiles, double* item, double* stats,
                              int items, int channels, int reduction, float* loss, hipStream_t stream);

// The second of those two launches alone, for a loss whose per-item value has a divisor of its own (foreground.hip).
void launch_loss_reduce(const double* item, int items, int channels, int reduction, bool one_minus, float* loss,
                        hipStream_t stream);

}  // namespace mpgan
