// Evaluation metrics of the reference's offline scripts, on the device:
//   inferrence.py:188-204  rescale a volume to 0..255 (ScaleIntensityRangePercentiles 0/100 ==
//                          min/max), round, then MAE against the ground truth;
//   metrics.py:213-223, psnr_ssim_metric.py:88-106  MSE and PSNR with data_range = 256 (SSIM: ssim_loss.hip, whose
//                          forward kernel serves the metric and the loss).
// HBM-bound two-stage reductions (fixed order, no atomics).  The joint histogram's bin rule, wave peel, chunk planner
// and value-range refusals are image_stats.h's, shared with Otsu's histogram (foreground.hip).
#include "image_stats.h"

namespace mpgan {

constexpr int MET_BLOCKS = 1024;

__global__ __launch_bounds__(256) void minmax_partial_kernel(const float* __restrict__ x, long n,
                                                             float* __restrict__ partials) {
  __shared__ float smin[4], smax[4];
  float lo = 3.4e38f, hi = -3.4e38f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = x[i];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, 64));
    hi = fmaxf(hi, __shfl_xor(hi, off, 64));
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { smin[w] = lo; smax[w] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
    partials[2 * blockIdx.x + 1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
  }
}

__global__ __launch_bounds__(64) void minmax_final_kernel(const float* __restrict__ partials, int nb,
                                                          float* __restrict__ out2) {
  float lo = 3.4e38f, hi = -3.4e38f;
  for (int i = threadIdx.x; i < nb; i += 64) {
    lo = fminf(lo, partials[2 * i]);
    hi = fmaxf(hi, partials[2 * i + 1]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, off, 64));
    hi = fmaxf(hi, __shfl_xor(hi, off, 64));
  }
  if (threadIdx.x == 0) { out2[0] = lo; out2[1] = hi; }
}

// y = round((x - min) / (max - min) * (b_max - b_min) + b_min), clipped to [b_min, b_max]
__global__ __launch_bounds__(256) void rescale_round_kernel(const float* __restrict__ x, long n,
                                                            const float* __restrict__ mm, float b_min, float b_max,
                                                            int do_round, float* __restrict__ y) {
  const float lo = mm[0], hi = mm[1];
  const float span = hi - lo;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float v = span != 0.f ? (x[i] - lo) / span : 0.f;
    v = v * (b_max - b_min) + b_min;
    v = fminf(fmaxf(v, b_min), b_max);
    y[i] = do_round ? rintf(v) : v;
  }
}

__global__ __launch_bounds__(256) void err_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                          long n, float* __restrict__ partials) {
  __shared__ float s1[4], s2[4];
  float ae = 0.f, se = 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float d = a[i] - b[i];
    ae += fabsf(d);
    se += d * d;
  }
  ae = block_sum4(ae, s1);
  se = block_sum4(se, s2);
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = ae;
    partials[2 * blockIdx.x + 1] = se;
  }
}

// out3 = (MAE, MSE, PSNR = 10 log10(range^2 / MSE))
__global__ __launch_bounds__(64) void err_final_kernel(const float* __restrict__ partials, int nb, double inv_n,
                                                       float data_range, float* __restrict__ out3) {
  double ae = 0.0, se = 0.0;
  for (int i = threadIdx.x; i < nb; i += 64) {
    ae += (double)partials[2 * i];
    se += (double)partials[2 * i + 1];
  }
  ae = wave_sum(ae);
  se = wave_sum(se);
  if (threadIdx.x == 0) {
    const double mae = ae * inv_n, mse = se * inv_n;
    out3[0] = (float)mae;
    out3[1] = (float)mse;
    out3[2] = mse > 0.0 ? (float)(10.0 * log10((double)data_range * data_range / mse)) : INFINITY;
  }
}

// ---- np.percentile on the device (ScaleIntensityRangePercentilesd, GAN_final.py:386-394) --------
// Exact order statistics by a 3-pass radix select (11 + 11 + 10 bits) over the monotone uint32
// image of the floats; integer atomics only, so the result does not depend on execution order.
constexpr int PCT_MAXT = 4;                     // order statistics per call (2 percentiles x {lo, lo+1})
constexpr int PCT_BINS = 2048;
struct PctState {
  unsigned prefix[PCT_MAXT];                    // key bits fixed so far (left-aligned)
  unsigned long long k[PCT_MAXT];               // rank still to find inside the prefix class
};

__device__ __forceinline__ unsigned pct_key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pct_unkey(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// pass 0: bits 31..21, one histogram shared by all targets; pass 1: bits 20..10 among the keys whose
// top 11 bits equal the target's prefix; pass 2: bits 9..0 among those whose top 22 bits do.
template <int PASS>
__global__ __launch_bounds__(256) void pct_hist_kernel(const float* __restrict__ x, long n, int nt,
                                                       const PctState* __restrict__ stt, unsigned* __restrict__ hist) {
  extern __shared__ unsigned lh[];              // [PASS == 0 ? 1 : nt][PCT_BINS]
  const int nh = PASS == 0 ? 1 : nt;
  for (int i = threadIdx.x; i < nh * PCT_BINS; i += 256) lh[i] = 0;
  unsigned pre[PCT_MAXT];
#pragma unroll
  for (int t = 0; t < PCT_MAXT; ++t) pre[t] = (PASS > 0 && t < nt) ? stt->prefix[t] : 0u;
  __syncthreads();
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const unsigned key = pct_key(x[i]);
    if (PASS == 0) {
      atomicAdd(&lh[key >> 21], 1u);
    } else {
#pragma unroll
      for (int t = 0; t < PCT_MAXT; ++t) {
        if (t >= nt) break;
        if (PASS == 1 && (key >> 21) == (pre[t] >> 21)) atomicAdd(&lh[t * PCT_BINS + ((key >> 10) & 2047u)], 1u);
        if (PASS == 2 && (key >> 10) == (pre[t] >> 10)) atomicAdd(&lh[t * PCT_BINS + (key & 1023u)], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nh * PCT_BINS; i += 256)
    if (lh[i]) atomicAdd(&hist[i], lh[i]);
}

// one thread per target walks its histogram to the bin that holds rank k; clears the histogram
template <int PASS>
__global__ __launch_bounds__(64) void pct_scan_kernel(int nt, PctState* __restrict__ stt, unsigned* __restrict__ hist) {
  const int t = threadIdx.x;
  if (t < nt) {
    const unsigned* h = hist + (PASS == 0 ? 0 : t * PCT_BINS);
    unsigned long long k = stt->k[t], cum = 0;
    const int bins = PASS == 2 ? 1024 : PCT_BINS;
    int bsel = bins - 1;
    for (int b2 = 0; b2 < bins; ++b2) {
      const unsigned c = h[b2];
      if (k < cum + c) { bsel = b2; break; }
      cum += c;
    }
    stt->k[t] = k - cum;
    const int shift = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);
    stt->prefix[t] |= (unsigned)bsel << shift;
  }
  __syncthreads();
  const int nh = PASS == 0 ? 1 : nt;
  for (int i = threadIdx.x; i < nh * PCT_BINS; i += 64) hist[i] = 0;
}

__global__ void pct_init_kernel(PctState* stt, unsigned* hist, int nt, unsigned long long k0, unsigned long long k1,
                                unsigned long long k2, unsigned long long k3) {
  const unsigned long long ks[4] = {k0, k1, k2, k3};
  if (threadIdx.x < PCT_MAXT) {
    stt->prefix[threadIdx.x] = 0;
    stt->k[threadIdx.x] = threadIdx.x < nt ? ks[threadIdx.x] : 0;
  }
  for (int i = threadIdx.x; i < PCT_MAXT * PCT_BINS; i += blockDim.x) hist[i] = 0;
}

// out[j] = s[lo_j] + frac_j * (s[lo_j + 1] - s[lo_j])   (numpy's linear interpolation, in double).  With frac_j == 0
// or two equal order statistics the result is s[lo_j] itself, without arithmetic: an infinite minimum / maximum
// stays infinite (the interpolation would form inf - inf).
__global__ void pct_final_kernel(const PctState* __restrict__ stt, int nq, double f0, double f1,
                                 float* __restrict__ out) {
  const double fr[2] = {f0, f1};
  if ((int)threadIdx.x < nq) {
    const double a = (double)pct_unkey(stt->prefix[2 * threadIdx.x]);
    const double b = (double)pct_unkey(stt->prefix[2 * threadIdx.x + 1]);
    const double t = fr[threadIdx.x];
    const double v = (t == 0.0 || a == b) ? a : (t >= 0.5 ? b - (b - a) * (1.0 - t) : a + (b - a) * t);
    out[threadIdx.x] = (float)v;
  }
}

// y = (x - a_min) / (a_max - a_min) * (b_max - b_min) + b_min, optionally clipped (MONAI ScaleIntensityRange)
__global__ __launch_bounds__(256) void scale_range_kernel(const float* __restrict__ x, long n,
                                                          const float* __restrict__ a_minmax, float b_min, float b_max,
                                                          int clip, float* __restrict__ y) {
  const float lo = a_minmax[0], hi = a_minmax[1];
  const float span = hi - lo;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float v = x[i] - lo;
    if (span != 0.f) {                           // MONAI: a_min == a_max -> warn and return x - a_min
      v = v / span * (b_max - b_min) + b_min;
      if (clip) v = fminf(fmaxf(v, b_min), b_max);
    }
    y[i] = v;
  }
}

}  // namespace mpgan

using namespace mpgan;

extern "C" int32_t mpgan_metric_partials(void) { return 2 * MET_BLOCKS; }

extern "C" int mpgan_rescale_minmax(const float* x, int64_t numel, float b_min, float b_max, int32_t do_round,
                                    float* partials, float* minmax2, float* y, void* stream) {
  MPGAN_CHECK_ARG(x && partials && minmax2 && y && numel > 0, "rescale_minmax: bad argument");
  long blocks = (numel + 255) / 256;
  if (blocks > MET_BLOCKS) blocks = MET_BLOCKS;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(minmax_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, (long)numel, partials);
  hipLaunchKernelGGL(minmax_final_kernel, dim3(1), dim3(64), 0, st, partials, (int)blocks, minmax2);
  hipLaunchKernelGGL(rescale_round_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, (long)numel, minmax2, b_min,
                     b_max, do_round, y);
  return check_launch("rescale_minmax");
}

extern "C" int mpgan_image_errors(const float* a, const float* b, int64_t numel, float data_range, float* partials,
                                  float* out3, void* stream) {
  MPGAN_CHECK_ARG(a && b && partials && out3 && numel > 0, "image_errors: bad argument");
  long blocks = (numel + 255) / 256;
  if (blocks > MET_BLOCKS) blocks = MET_BLOCKS;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(err_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, b, (long)numel, partials);
  hipLaunchKernelGGL(err_final_kernel, dim3(1), dim3(64), 0, st, partials, (int)blocks, 1.0 / (double)numel,
                     data_range, out3);
  return check_launch("image_errors");
}

extern "C" int64_t mpgan_percentile_workspace(void) {
  return (int64_t)sizeof(PctState) + (int64_t)PCT_MAXT * PCT_BINS * (int64_t)sizeof(unsigned) + 64;
}

extern "C" int mpgan_percentiles(const float* x, int64_t numel, const double* q_host, int32_t nq, void* workspace,
                                 int64_t workspace_bytes, float* out, void* stream) {
  MPGAN_CHECK_ARG(x && q_host && workspace && out && numel > 0, "percentiles: bad argument");
  MPGAN_UNSUPPORTED(nq < 1 || nq > 2, "percentiles: 1 or 2 percentiles per call (got %d)", nq);
  MPGAN_UNSUPPORTED(numel >= (1LL << 32), "percentiles: numel >= 2^32 would overflow the uint32 histogram counters");
  MPGAN_CHECK_ARG(workspace_bytes >= mpgan_percentile_workspace(), "percentiles: workspace too small");
  MPGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "percentiles: workspace must be 8-byte aligned");
  unsigned long long ks[4] = {0, 0, 0, 0};
  double fr[2] = {0, 0};
  for (int j = 0; j < nq; ++j) {
    MPGAN_CHECK_ARG(q_host[j] >= 0.0 && q_host[j] <= 100.0, "percentiles: q outside [0, 100]");
    const double r = q_host[j] / 100.0 * (double)(numel - 1);      // numpy: virtual index q * (n - 1)
    long lo = (long)r;
    if (lo > numel - 1) lo = numel - 1;
    const long hi = lo + 1 < numel ? lo + 1 : lo;
    ks[2 * j] = (unsigned long long)lo;
    ks[2 * j + 1] = (unsigned long long)hi;
    fr[j] = r - (double)lo;
  }
  PctState* stt = static_cast<PctState*>(workspace);
  unsigned* hist = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + ((sizeof(PctState) + 63) / 64) * 64);
  const int nt = 2 * nq;
  hipStream_t st = (hipStream_t)stream;
  long blocks = (numel + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(pct_init_kernel, dim3(1), dim3(256), 0, st, stt, hist, nt, ks[0], ks[1], ks[2], ks[3]);
  hipLaunchKernelGGL((pct_hist_kernel<0>), dim3((unsigned)blocks), dim3(256), PCT_BINS * sizeof(unsigned), st, x,
                     (long)numel, nt, stt, hist);
  hipLaunchKernelGGL((pct_scan_kernel<0>), dim3(1), dim3(64), 0, st, nt, stt, hist);
  hipLaunchKernelGGL((pct_hist_kernel<1>), dim3((unsigned)blocks), dim3(256), nt * PCT_BINS * sizeof(unsigned), st, x,
                     (long)numel, nt, stt, hist);
  hipLaunchKernelGGL((pct_scan_kernel<1>), dim3(1), dim3(64), 0, st, nt, stt, hist);
  hipLaunchKernelGGL((pct_hist_kernel<2>), dim3((unsigned)blocks), dim3(256), nt * PCT_BINS * sizeof(unsigned), st, x,
                     (long)numel, nt, stt, hist);
  hipLaunchKernelGGL((pct_scan_kernel<2>), dim3(1), dim3(64), 0, st, nt, stt, hist);
  hipLaunchKernelGGL(pct_final_kernel, dim3(1), dim3(64), 0, st, stt, nq, fr[0], fr[1], out);
  return check_launch("percentiles");
}

extern "C" int mpgan_scale_intensity_range(const float* x, int64_t numel, const float* a_minmax, float b_min,
                                           float b_max, int32_t clip, float* y, void* stream) {
  MPGAN_CHECK_ARG(x && a_minmax && y && numel > 0, "scale_intensity_range: bad argument");
  long blocks = (numel + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(scale_range_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, (long)numel,
                     a_minmax, b_min, b_max, clip, y);
  return check_launch("scale_intensity_range");
}

// ---------------------------------------------------------------------------------------------------
// Resampling onto the 256 mm identity grid (next-row N3, code/GAN/transforms.py:79-213: ResampleT1T2d =
// itk.resample_image_filter(identity transform, LinearInterpolateImageFunction, reference image with
// origin = -size/2, spacing = 256/size, identity direction), default pixel 0).  ITK is not in this image; the
// kernel restates ITK 5's published algorithm:
//   p   = origin_out + i * spacing_out                         (output physical point, identity direction)
//   c   = (Direction_in * diag(spacing_in))^-1 (p - origin_in)  (continuous index into the input)
//   inside  <=>  -0.5 <= c_d < size_d - 0.5 for every d        (ImageFunction::IsInsideBuffer)
//   value   = trilinear interpolation at c, the base index clamped to [0, size-1] and a neighbour beyond the last
//             index dropped (LinearInterpolateImageFunction::EvaluateOptimized), else 0.
// One thread per output voxel: an HBM/L2-bound gather (8 reads, 1 write).
// ---------------------------------------------------------------------------------------------------
struct ResampleGeom {
  double m[9];        // inverse of Direction*diag(spacing), row-major, in ITK (x, y, z) order
  double origin_in[3];
  double origin_out[3], spacing_out[3];
  int in_size[3];     // (x, y, z)
  int out_size[3];
};

__global__ __launch_bounds__(256) void resample_linear_kernel(const float* __restrict__ in, ResampleGeom g,
                                                              float* __restrict__ out) {
  const long total = (long)g.out_size[0] * g.out_size[1] * g.out_size[2];
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ox = (int)(i % g.out_size[0]);
    const long q = i / g.out_size[0];
    const int oy = (int)(q % g.out_size[1]), oz = (int)(q / g.out_size[1]);
    const double d0 = g.origin_out[0] + ox * g.spacing_out[0] - g.origin_in[0];
    const double d1 = g.origin_out[1] + oy * g.spacing_out[1] - g.origin_in[1];
    const double d2 = g.origin_out[2] + oz * g.spacing_out[2] - g.origin_in[2];
    double c[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) c[r] = g.m[3 * r] * d0 + g.m[3 * r + 1] * d1 + g.m[3 * r + 2] * d2;
    bool inside = true;
    int b[3];
    double f[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      inside = inside && c[d] >= -0.5 && c[d] < (double)g.in_size[d] - 0.5;
      int bi = (int)floor(c[d]);
      if (bi < 0) bi = 0;
      b[d] = bi;
      double fr = c[d] - (double)bi;
      if (fr < 0.0) fr = 0.0;                       // c in [-0.5, 0): the base sample alone
      if (bi + 1 > g.in_size[d] - 1) fr = 0.0;      // no neighbour beyond the last index
      f[d] = fr;
    }
    float v = 0.f;
    if (inside) {
      const long sx = 1, sy = g.in_size[0], sz = (long)g.in_size[0] * g.in_size[1];
      const long base = b[0] * sx + b[1] * sy + b[2] * sz;
      const long ax = f[0] > 0.0 ? sx : 0, ay = f[1] > 0.0 ? sy : 0, az = f[2] > 0.0 ? sz : 0;
      const double v000 = in[base], v100 = in[base + ax], v010 = in[base + ay], v110 = in[base + ax + ay];
      const double v001 = in[base + az], v101 = in[base + ax + az], v011 = in[base + ay + az],
                   v111 = in[base + ax + ay + az];
      const double x00 = v000 + f[0] * (v100 - v000), x10 = v010 + f[0] * (v110 - v010);
      const double x01 = v001 + f[0] * (v101 - v001), x11 = v011 + f[0] * (v111 - v011);
      const double y0 = x00 + f[1] * (x10 - x00), y1 = x01 + f[1] * (x11 - x01);
      v = (float)(y0 + f[2] * (y1 - y0));
    }
    out[i] = v;
  }
}

extern "C" int mpgan_resample_to_identity_grid(const float* vol, const int32_t* in_dhw, const double* origin_xyz,
                                               const double* spacing_xyz, const double* direction_3x3,
                                               const int32_t* out_dhw, double extent_mm, float* out, void* stream) {
  MPGAN_CHECK_ARG(vol && in_dhw && origin_xyz && spacing_xyz && direction_3x3 && out_dhw && out && extent_mm > 0,
                  "resample: null argument");
  ResampleGeom g;
  double a[9];   // A = Direction * diag(spacing)
  for (int d = 0; d < 3; ++d) {
    MPGAN_CHECK_ARG(in_dhw[d] > 0 && out_dhw[d] > 0 && spacing_xyz[d] > 0, "resample: bad size / spacing in dim %d", d);
    g.in_size[d] = in_dhw[2 - d];               // arrays are (z, y, x); ITK indexes (x, y, z)
    g.out_size[d] = out_dhw[2 - d];
    g.origin_in[d] = origin_xyz[d];
    g.origin_out[d] = -0.5 * g.out_size[d];      // transforms.py:144: SetOrigin(-output_size / 2)
    g.spacing_out[d] = extent_mm / g.out_size[d];
    for (int r = 0; r < 3; ++r) a[3 * r + d] = direction_3x3[3 * r + d] * spacing_xyz[d];
  }
  const double det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
  MPGAN_CHECK_ARG(det != 0.0, "resample: singular direction matrix");
  g.m[0] = (a[4] * a[8] - a[5] * a[7]) / det; g.m[1] = (a[2] * a[7] - a[1] * a[8]) / det; g.m[2] = (a[1] * a[5] - a[2] * a[4]) / det;
  g.m[3] = (a[5] * a[6] - a[3] * a[8]) / det; g.m[4] = (a[0] * a[8] - a[2] * a[6]) / det; g.m[5] = (a[2] * a[3] - a[0] * a[5]) / det;
  g.m[6] = (a[3] * a[7] - a[4] * a[6]) / det; g.m[7] = (a[1] * a[6] - a[0] * a[7]) / det; g.m[8] = (a[0] * a[4] - a[1] * a[3]) / det;
  const long total = (long)out_dhw[0] * out_dhw[1] * out_dhw[2];
  long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(resample_linear_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, vol, g, out);
  return check_launch("resample_to_identity_grid");
}

// ---------------------------------------------------------------------------------------------------
// Joint histogram and mutual information (the reference's third stored quality figure).
//   hist[item][ia][ib] = number of admitted voxels whose a-value falls into bin ia and b-value into bin ib, with
//   idx = hist_bin(v) = min((int)floorf((v - lo) * s), bins - 1), s = (float)bins / (hi - lo), all in fp32 as
//   written (image_stats.h).  A voxel outside either range, NaN, or refused by the mask is dropped.
// A block privatises a band of a-rows in LDS as uint32 counters (LDS integer atomics), walks its chunk of the
// voxels, and flushes its non-zero counters once with 64-bit integer atomics: consecutive lanes flush consecutive
// counters, so the global atomics are contiguous 512-byte wave-instructions instead of one scattered atomic per
// voxel.  Integer sums only: the histogram does not depend on execution order.
// ---------------------------------------------------------------------------------------------------
namespace mpgan {

constexpr int JH_THREADS = 1024;
constexpr int JH_LDS_COUNTERS = 16384;          // 64 KB of uint32: two blocks share a CU's 160 KB
constexpr long JH_CHUNK_MIN = 16384;            // voxels a block walks at least (its zero + flush pass is 16 K counters)
constexpr int JH_TARGET_BLOCKS = 512;           // two 16-wave blocks per CU
constexpr int JH_PEEL_ROUNDS = 4;
enum { JH_MASK_NONE = 0, JH_MASK_BOTH_NONZERO = 1, JH_MASK_EITHER_NONZERO = 2, JH_MASK_EXPLICIT = 3 };

// The ONE place the form of a joint-histogram launch is decided: how many a-rows a block keeps in LDS (all of them
// up to 128 bins; above that a band of floor(16384 / bins) rows, and every band re-reads the voxels and skips those
// outside it), and how many blocks share one (item, band).
struct JhChoice {
  int band_rows, bands;
  long chunks, per_chunk;                       // per_chunk is a multiple of 4: every chunk starts float4-aligned
};

static JhChoice choose_joint_hist(int bins, long n, int batch) {
  JhChoice c;
  c.band_rows = bins * bins <= JH_LDS_COUNTERS ? bins : JH_LDS_COUNTERS / bins;
  c.bands = (bins + c.band_rows - 1) / c.band_rows;
  const StreamChunks sc = stream_chunks(n, (long)batch * c.bands, JH_CHUNK_MIN, JH_TARGET_BLOCKS);
  c.chunks = sc.chunks;
  c.per_chunk = sc.per_chunk;
  return c;
}

struct JhParams {
  const float* a;
  const float* b;
  const uint8_t* mask;
  long n;                                       // voxels per item
  float lo_a, hi_a, s_a, lo_b, hi_b, s_b;
  int bins, mask_mode, band_rows, bands;
  long chunks, per_chunk;
  unsigned long long* hist;
};

__device__ __forceinline__ void jh_voxel(unsigned* lh, const JhParams& p, int r0, int r1, bool valid, float va, float vb,
                                         unsigned mk) {
  bool ok = valid && va >= p.lo_a && va <= p.hi_a && vb >= p.lo_b && vb <= p.hi_b;   // NaN fails every comparison
  if (p.mask_mode == JH_MASK_BOTH_NONZERO) ok = ok && va != 0.f && vb != 0.f;
  else if (p.mask_mode == JH_MASK_EITHER_NONZERO) ok = ok && (va != 0.f || vb != 0.f);
  else if (p.mask_mode == JH_MASK_EXPLICIT) ok = ok && mk != 0u;
  unsigned key = 0;
  if (ok) {
    const int ia = hist_bin(va, p.lo_a, p.s_a, p.bins), ib = hist_bin(vb, p.lo_b, p.s_b, p.bins);
    ok = ia >= r0 && ia < r1;
    key = (unsigned)((ia - r0) * p.bins + ib);
  }
  hist_submit<JH_PEEL_ROUNDS>(lh, ok, ok ? key : 0u);
}

__global__ __launch_bounds__(JH_THREADS) void joint_hist_kernel(JhParams p) {
  extern __shared__ unsigned jh_lds[];          // [band rows][bins]
  const int tid = threadIdx.x;
  long blk = blockIdx.x;
  const long chunk = blk % p.chunks;
  blk /= p.chunks;
  const int band = (int)(blk % p.bands);
  const long item = blk / p.bands;
  const int r0 = band * p.band_rows;
  const int r1 = r0 + p.band_rows < p.bins ? r0 + p.band_rows : p.bins;
  const int counters = (r1 - r0) * p.bins;
  for (int i = tid; i < counters; i += JH_THREADS) jh_lds[i] = 0u;
  __syncthreads();
  const long c0 = chunk * p.per_chunk;
  long c1 = c0 + p.per_chunk;
  if (c1 > p.n) c1 = p.n;
  if (c0 < c1) {
    const float* a = p.a + item * p.n;
    const float* b = p.b + item * p.n;
    const uint8_t* mk = p.mask_mode == JH_MASK_EXPLICIT ? p.mask + item * p.n : nullptr;
    const long len = c1 - c0;
    // 16-byte loads when both item bases are 16-byte aligned (c0 is a multiple of 4); the scalar loop takes every
    // other alignment and the tail.  Trip counts are block-uniform: hist_submit needs every lane of a wave.
    const bool vec = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0;
    const long nvec = vec ? len >> 2 : 0;
    for (long j0 = 0; j0 < nvec; j0 += JH_THREADS) {
      const long j = j0 + tid;
      const bool valid = j < nvec;
      float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
      unsigned m0 = 1, m1 = 1, m2 = 1, m3 = 1;
      if (valid) {
        const long e = c0 + 4 * j;
        va = *reinterpret_cast<const float4*>(a + e);
        vb = *reinterpret_cast<const float4*>(b + e);
        if (mk) { m0 = mk[e]; m1 = mk[e + 1]; m2 = mk[e + 2]; m3 = mk[e + 3]; }
      }
      jh_voxel(jh_lds, p, r0, r1, valid, va.x, vb.x, m0);
      jh_voxel(jh_lds, p, r0, r1, valid, va.y, vb.y, m1);
      jh_voxel(jh_lds, p, r0, r1, valid, va.z, vb.z, m2);
      jh_voxel(jh_lds, p, r0, r1, valid, va.w, vb.w, m3);
    }
    for (long j0 = 4 * nvec; j0 < len; j0 += JH_THREADS) {
      const long j = j0 + tid;
      const bool valid = j < len;
      float va = 0.f, vb = 0.f;
      unsigned m0 = 1;
      if (valid) {
        va = a[c0 + j];
        vb = b[c0 + j];
        if (mk) m0 = mk[c0 + j];
      }
      jh_voxel(jh_lds, p, r0, r1, valid, va, vb, m0);
    }
  }
  __syncthreads();
  unsigned long long* out = p.hist + (item * p.bins + r0) * (long)p.bins;
  for (int i = tid; i < counters; i += JH_THREADS) {
    const unsigned c = jh_lds[i];
    if (c) atomicAdd(&out[i], (unsigned long long)c);
  }
}

// Mutual information of one item's histogram, one block per item.  Row and column sums are exact integers (LDS
// 64-bit integer atomics: order-free).  The three sums of c*log(c) are doubles: every thread adds its terms in a
// fixed order and the block folds the per-thread sums by a fixed tree, so the six outputs are bitwise reproducible.
//   H = log N - (sum c log c) / N   (nats);   out6 = (mi, h_a, h_b, h_ab, nmi, count)
constexpr int MI_THREADS = 1024;

__global__ __launch_bounds__(MI_THREADS) void mutual_info_kernel(const unsigned long long* __restrict__ hist, int bins,
                                                                  double* __restrict__ out6) {
  __shared__ unsigned long long rows[256], cols[256];
  __shared__ double red[MI_THREADS];
  __shared__ unsigned long long tot_s, nnz_s;
  const int tid = threadIdx.x;
  const unsigned long long* h = hist + (long)blockIdx.x * bins * bins;
  if (tid < 256) { rows[tid] = 0ull; cols[tid] = 0ull; }
  if (tid == 0) { tot_s = 0ull; nnz_s = 0ull; }
  __syncthreads();
  // a wave walks whole rows: lanes over the columns (coalesced), the row sum folded in the wave
  const int lane = tid & 63, wave = tid >> 6;
  double s_ab = 0.0;
  unsigned nnz = 0;
  for (int r = wave; r < bins; r += MI_THREADS / 64) {
    unsigned long long rs = 0ull;
    for (int c = lane; c < bins; c += 64) {
      const unsigned long long v = h[(long)r * bins + c];
      if (v) {
        rs += v;
        ++nnz;
        s_ab += (double)v * log((double)v);
        atomicAdd(&cols[c], v);
      }
    }
    rs = wave_sum(rs);
    if (lane == 0) rows[r] = rs;
  }
  if (nnz) atomicAdd(&nnz_s, (unsigned long long)nnz);
  __syncthreads();
  double s_a = 0.0, s_b = 0.0;
  if (tid < bins) {
    const unsigned long long ra = rows[tid], cb = cols[tid];
    if (ra) { s_a = (double)ra * log((double)ra); atomicAdd(&tot_s, ra); }
    if (cb) s_b = (double)cb * log((double)cb);
  }
  s_ab = block_tree_sum<MI_THREADS, true>(s_ab, red);
  s_a = block_tree_sum<MI_THREADS, true>(s_a, red);
  s_b = block_tree_sum<MI_THREADS, true>(s_b, red);
  if (tid == 0) {
    double* o = out6 + 6 * (long)blockIdx.x;
    const unsigned long long total = tot_s;
    if (total == 0ull) {
      const double qnan = __longlong_as_double(0x7ff8000000000000LL);
      o[0] = o[1] = o[2] = o[3] = o[4] = qnan;
      o[5] = 0.0;
    } else if (nnz_s == 1ull) {                  // every voxel in one bin: H_ab == 0
      o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; o[3] = 0.0; o[4] = 1.0;
      o[5] = (double)total;
    } else {
      const double n = (double)total, ln = log(n);
      const double ha = ln - s_a / n, hb = ln - s_b / n, hab = ln - s_ab / n;
      o[0] = ha + hb - hab;
      o[1] = ha; o[2] = hb; o[3] = hab;
      o[4] = (ha + hb) / hab;
      o[5] = n;
    }
  }
}

}  // namespace mpgan

extern "C" int mpgan_joint_histogram(const float* a, const float* b, const uint8_t* mask, int32_t mask_mode,
                                     int64_t numel_per_item, int32_t batch, float lo_a, float hi_a, float lo_b,
                                     float hi_b, int32_t bins, int64_t* hist, void* stream) {
  MPGAN_CHECK_ARG(bins >= 2 && bins <= 256, "joint_histogram: bins %d outside [2, 256]", bins);
  MPGAN_CHECK_ARG(batch >= 1, "joint_histogram: batch %d < 1", batch);
  MPGAN_CHECK_ARG(numel_per_item >= 0, "joint_histogram: negative numel_per_item");
  MPGAN_CHECK_ARG(mask_mode >= JH_MASK_NONE && mask_mode <= JH_MASK_EXPLICIT, "joint_histogram: unknown mask_mode %d",
                  mask_mode);
  MPGAN_CHECK_ARG(hist != nullptr, "joint_histogram: null hist");
  MPGAN_CHECK_ARG((a && b) || numel_per_item == 0, "joint_histogram: null input");
  MPGAN_CHECK_ARG(mask || mask_mode != JH_MASK_EXPLICIT || numel_per_item == 0,
                  "joint_histogram: mask_mode 3 needs a mask array");
  float s_a, s_b;
  if (int rc = check_bin_range("joint_histogram", lo_a, hi_a, bins, &s_a)) return rc;
  if (int rc = check_bin_range("joint_histogram", lo_b, hi_b, bins, &s_b)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const JhChoice c = choose_joint_hist(bins, numel_per_item, batch);
  const int64_t blocks = c.chunks * c.bands * (int64_t)batch;
  MPGAN_CHECK_ARG(blocks < (1LL << 31), "joint_histogram: too many blocks");
  hipError_t e = hipMemsetAsync(hist, 0, (size_t)batch * bins * bins * sizeof(int64_t), st);
  if (e != hipSuccess) { set_error("joint_histogram: hipMemsetAsync: %s", hipGetErrorString(e)); return MPGAN_ERR_HIP; }
  if (numel_per_item == 0) return MPGAN_OK;
  JhParams p;
  p.a = a; p.b = b; p.mask = mask; p.n = numel_per_item;
  p.lo_a = lo_a; p.hi_a = hi_a; p.s_a = s_a; p.lo_b = lo_b; p.hi_b = hi_b; p.s_b = s_b;
  p.bins = bins; p.mask_mode = mask_mode; p.band_rows = c.band_rows; p.bands = c.bands;
  p.chunks = c.chunks; p.per_chunk = c.per_chunk;
  p.hist = reinterpret_cast<unsigned long long*>(hist);
  const size_t smem = (size_t)c.band_rows * bins * sizeof(unsigned);
  hipLaunchKernelGGL(joint_hist_kernel, dim3((unsigned)blocks), dim3(JH_THREADS), smem, st, p);
  return check_launch("joint_histogram");
}

extern "C" int mpgan_mutual_information(const int64_t* hist, int32_t batch, int32_t bins, double* out6, void* stream) {
  MPGAN_CHECK_ARG(bins >= 2 && bins <= 256, "mutual_information: bins %d outside [2, 256]", bins);
  MPGAN_CHECK_ARG(batch >= 1, "mutual_information: batch %d < 1", batch);
  MPGAN_CHECK_ARG(hist && out6, "mutual_information: null pointer");
  hipLaunchKernelGGL(mutual_info_kernel, dim3((unsigned)batch), dim3(MI_THREADS), 0, (hipStream_t)stream,
                     reinterpret_cast<const unsigned long long*>(hist), (int)bins, out6);
  return check_launch("mutual_information");
}
