// Differentiable global mutual information with Parzen windows (include/mpgan_hip.h: "Parzen-window mutual
// information" states the definition and the gradient).  Three kernels:
//
//   pmi_joint_kernel     the K x K joint is an outer-product sum over the voxels, a GEMM whose contraction index is
//                        the voxel.  A wave runs it on v_mfma_f32_32x32x2_f32 (exact fp32): the bins are padded to 32
//                        with zero weights, lane l owns bin l & 31 of voxel l >> 5 of the instruction's two voxels,
//                        computes that one Gaussian of each image, and the per-voxel normalisers sum(e_a), sum(e_b)
//                        come from a 32-lane reduction (four DPP steps and one ds_swizzle, no memory).  The 32 x 32
//                        accumulator lives in 16 registers per lane: no LDS or global atomic per sample.  A wave owns
//                        one chunk of PMI_CHUNK = 512 consecutive voxels of one item, so an accumulator is an fp32
//                        fmaf chain of at most 512 products of weights <= 1 (the bound of the fp32 run length).  The
//                        16 waves of a block then add their tiles in wave order in fp64 through LDS and the block
//                        writes ONE fp64 tile to its own slot of the workspace: slots = ceil(N / 8192) per item, a
//                        function of N only.
//   pmi_finalize_kernel  one block per item: sums the slots in slot order (fp64), divides by N, forms the marginals
//                        from the joint, mi, and the two coefficient matrices of the gradient (G for the first image,
//                        G' transposed for the second) in fp64; a fixed tree folds mi: bitwise reproducible.
//   pmi_backward_kernel  one voxel per lane, the item's coefficients in LDS (every lane reads the same address: a
//                        broadcast); run with the roles of the two images swapped for the second image's gradient.
//
// (The other normaliser strategy -- one voxel per lane, K exps, normalised weights transposed through LDS -- was not
// built: the reduction is ten DPP adds and two swizzles in a step of about forty vector instructions.)
// The value-range refusals are image_stats.h's (without the fp32 binning rule: nothing is binned here), the reduction,
// wrt, upstream_stride and workspace checks mpgan_common.h's.
#include "image_stats.h"
#include "conv_geom.h"

namespace mpgan {

constexpr int PMI_T = 32;                       // padded bins: the MFMA tile
constexpr int PMI_TILE = PMI_T * PMI_T;
constexpr long PMI_CHUNK = 512;                 // voxels per wave == bound of an accumulator's fp32 run length
constexpr int PMI_WAVES = 16;                   // waves per block of the joint kernel; a block fills one slot

// The ONE place the slot geometry is decided: a function of N only.
static long pmi_slots(long n) { return (n + PMI_CHUNK * PMI_WAVES - 1) / (PMI_CHUNK * PMI_WAVES); }

template <int CTRL>
__device__ __forceinline__ float pmi_dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// Sum over the 32 lanes of a wave half; every lane of the half ends with the same bits (each step adds two values
// that both partners hold, in either order).  Needs all 64 lanes active.
__device__ __forceinline__ float pmi_half_sum(float v) {
  v = pmi_dpp_add<0xB1>(v);                     // quad_perm [1,0,3,2]
  v = pmi_dpp_add<0x4E>(v);                     // quad_perm [2,3,0,1]
  v = pmi_dpp_add<0x141>(v);                    // row_half_mirror: the other quad of the 8
  v = pmi_dpp_add<0x140>(v);                    // row_mirror: the other 8 of the 16
  return v + __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F));   // lane ^ 16
}

// exp(-p d^2) as v_exp_f32(c2 d^2) with c2 = -p log2(e) folded on the host: the argument carries the same two fp32
// roundings as -p d^2 would, and the instruction is good to one ulp; results below 2^-126 flush to zero, forty orders
// of magnitude under any weight that counts.
__device__ __forceinline__ float pmi_gauss(float c2, float d) { return __builtin_amdgcn_exp2f(c2 * d * d); }

// x' = clamp((x - lo) / span, 0, 1); a NaN stays NaN (both comparisons fail), as torch.clamp keeps it
__device__ __forceinline__ float pmi_map(float x, float lo, float span) {
  const float t = (x - lo) / span;
  return t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
}

struct PmiJoint {
  const float* a;
  const float* b;
  long n, slots;
  float lo_a, span_a, lo_b, span_b, c2;     // c2 = -p log2(e)
  int bins;
  double* ws;                                   // [batch][slots][32][32]
};

__global__ __launch_bounds__(64 * PMI_WAVES) void pmi_joint_kernel(PmiJoint q) {
  __shared__ float tiles[PMI_WAVES * PMI_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bin = lane & 31, half = lane >> 5;
  const long slot = blockIdx.x, item = blockIdx.y;
  const long c0 = (slot * PMI_WAVES + wave) * PMI_CHUNK;      // at or beyond n: this wave adds a zero tile
  const long c1 = c0 + PMI_CHUNK < q.n ? c0 + PMI_CHUNK : q.n;
  const float* a = q.a + item * q.n;
  const float* b = q.b + item * q.n;
  const bool bin_ok = bin < q.bins;             // bins >= K carry zero weight in both operands
  const float centre = (float)bin / (float)(q.bins - 1);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (long g0 = c0; g0 < c1; g0 += 64) {
    const long idx = g0 + lane;
    const bool ok = idx < c1;
    const float xa = ok ? pmi_map(a[idx], q.lo_a, q.span_a) : 0.f;
    const float xb = ok ? pmi_map(b[idx], q.lo_b, q.span_b) : 0.f;
    const int cnt = c1 - g0 < 64 ? (int)(c1 - g0) : 64;
    const int steps = __builtin_amdgcn_readfirstlane((cnt + 1) >> 1);
    for (int t = 0; t < steps; ++t) {
      const int v = 2 * t + half;
      const bool valid = v < cnt;               // a padded tail voxel has zero WEIGHT (a zero value would be bin 0)
      const float da = __shfl(xa, v, 64) - centre;
      const float db = __shfl(xb, v, 64) - centre;
      const float ea = (bin_ok && valid) ? pmi_gauss(q.c2, da) : 0.f;
      const float eb = (bin_ok && valid) ? pmi_gauss(q.c2, db) : 0.f;
      const float sa = pmi_half_sum(ea);
      const float sb = pmi_half_sum(eb);
      const float wa = valid ? ea * __builtin_amdgcn_rcpf(sa) : 0.f;
      const float wb = valid ? eb * __builtin_amdgcn_rcpf(sb) : 0.f;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa, wb, acc, 0, 0, 0);
    }
  }
  float* mine = tiles + wave * PMI_TILE;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * half;   // row: the first image's bin; column (lane & 31): the second's
    mine[row * PMI_T + bin] = acc[r];
  }
  __syncthreads();
  double s = 0.0;                               // thread = tile entry; the waves' tiles in wave order
#pragma unroll
  for (int w = 0; w < PMI_WAVES; ++w) s += (double)tiles[w * PMI_TILE + threadIdx.x];
  q.ws[(item * q.slots + slot) * PMI_TILE + threadIdx.x] = s;
}

// coef[item][0][i][j] = G_ij, coef[item][1][j][i] = G'_ij, each minus a constant (below); floats, zero outside K x K
__global__ __launch_bounds__(PMI_TILE) void pmi_finalize_kernel(const double* __restrict__ ws, long slots, long n,
                                                                int bins, double nr, double dr,
                                                                double* __restrict__ joint, double* __restrict__ mi,
                                                                float* __restrict__ coef) {
  __shared__ double sp[PMI_TILE], sd[PMI_TILE];
  __shared__ double pa[PMI_T], pb[PMI_T], ua[PMI_T], ub[PMI_T];
  const int tid = threadIdx.x, i = tid >> 5, j = tid & 31;
  const long item = blockIdx.x;
  const double* w = ws + item * slots * PMI_TILE + tid;
  double s = 0.0;
  long k = 0;
  for (; k + 8 <= slots; k += 8) {              // eight loads in flight, added in slot order
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = w[(k + u) * PMI_TILE];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; k < slots; ++k) s += w[k * PMI_TILE];
  s /= (double)n;
  sp[tid] = s;
  __syncthreads();
  if (tid < PMI_T) {
    double ra = 0.0, cb = 0.0;
    for (int k = 0; k < PMI_T; ++k) {
      ra += sp[tid * PMI_T + k];
      cb += sp[k * PMI_T + tid];
    }
    pa[tid] = ra;
    pb[tid] = cb;
  }
  __syncthreads();
  const bool in = i < bins && j < bins;
  const double den = pa[i] * pb[j] + dr;
  const double rd = (s + nr) / den + dr;
  const double lg = log(rd);
  const double A = lg + s / (rd * den);
  sd[tid] = in ? -s * (s + nr) / (rd * den * den) : 0.0;
  __syncthreads();
  if (tid < PMI_T) {
    double u = 0.0, v = 0.0;
    for (int k = 0; k < PMI_T; ++k) {
      u += sd[tid * PMI_T + k] * pb[k];
      v += sd[k * PMI_T + tid] * pa[k];
    }
    ua[tid] = u;
    ub[tid] = v;
  }
  __syncthreads();
  // Every wb(n) sums to 1, so a constant added to G adds the same constant to every h_i(n) and leaves h_i - hbar as
  // it is: store G minus its pab-weighted mean (the mean of hbar over the voxels), which keeps the fp32 backward's
  // h small against its spread.  Likewise for G'.
  const double ga = in ? A + ua[i] : 0.0, gb = in ? A + ub[j] : 0.0;
  const double ma = block_tree_sum<PMI_TILE, true>(s * ga, sd), mb = block_tree_sum<PMI_TILE, true>(s * gb, sd);
  if (coef) {
    float* c = coef + item * 2 * PMI_TILE;
    c[i * PMI_T + j] = in ? (float)(ga - ma) : 0.f;
    c[PMI_TILE + j * PMI_T + i] = in ? (float)(gb - mb) : 0.f;
  }
  if (joint && in) joint[(item * bins + i) * bins + j] = s;
  const double total = block_tree_sum<PMI_TILE, true>(in ? s * lg : 0.0, sd);
  if (tid == 0) mi[item] = total;
}

// loss = -mean(mi) (0), -sum(mi) (1), or loss[b] = -mi[b] (2); item order
__global__ void pmi_loss_kernel(const double* __restrict__ mi, int batch, int reduction, float* __restrict__ loss) {
  if (reduction == 2) {
    for (int b = threadIdx.x; b < batch; b += blockDim.x) loss[b] = (float)(-mi[b]);
    return;
  }
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int b = 0; b < batch; ++b) s += mi[b];
    loss[0] = (float)(reduction == 0 ? -s / (double)batch : -s);
  }
}

struct PmiBwd {
  const float* x;                               // the image the gradient is for
  const float* y;                               // the other image
  long n;
  float lo_x, span_x, lo_y, span_y, p, c2, scale;
  int bins, wrt, up_stride;
  const float* coef;
  const float* upstream;
  float* grad;
};

// KP: the bin count rounded up to a multiple of 8, so that every loop over bins unrolls and the per-voxel vectors
// stay in registers; bins in [K, KP) carry zero weight and zero coefficients.
template <int KP>
__global__ __launch_bounds__(256) void pmi_backward_kernel(PmiBwd q) {
  __shared__ __attribute__((aligned(16))) float sg[PMI_TILE];
  __shared__ float sc[PMI_T];
  const int tid = threadIdx.x;
  const long item = blockIdx.y;
  const float* g = q.coef + (item * 2 + q.wrt) * PMI_TILE;
  for (int k = tid; k < PMI_TILE; k += 256) sg[k] = g[k];
  if (tid < PMI_T) sc[tid] = (float)tid / (float)(q.bins - 1);
  __syncthreads();
  const float up = q.upstream[item * q.up_stride] * q.scale;
  const float* x = q.x + item * q.n;
  const float* y = q.y + item * q.n;
  float* out = q.grad + item * q.n;
  for (long idx = (long)blockIdx.x * 256 + tid; idx < q.n; idx += (long)gridDim.x * 256) {
    const float t = (x[idx] - q.lo_x) / q.span_x;
    const bool inside = t >= 0.f && t <= 1.f;   // the CLOSED interval: torch.clamp's rule
    const float xm = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
    const float ym = pmi_map(y[idx], q.lo_y, q.span_y);
    float wy[KP];
    float sy = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const float d = ym - sc[k];
      wy[k] = k < q.bins ? pmi_gauss(q.c2, d) : 0.f;
      sy += wy[k];
    }
    const float ry = __builtin_amdgcn_rcpf(sy);
#pragma unroll
    for (int k = 0; k < KP; ++k) wy[k] *= ry;
    // sum_i wa_i (h_i - hbar) d_i = (T1 - (T2 / S) T3) / S with T1 = sum e_i h_i d_i, T2 = sum e_i h_i, T3 = sum e_i d_i:
    // one pass over the rows, nothing but wy[] live across it (the finalize kernel centres the coefficients, so that
    // hbar is small against the spread of h and the subtraction costs no digits)
    float sx = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
#pragma unroll 1
    for (int r = 0; r < q.bins; ++r) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < KP; k += 4) {
        const float4 c4 = *reinterpret_cast<const float4*>(&sg[r * PMI_T + k]);
        acc = fmaf(c4.x, wy[k], acc);
        acc = fmaf(c4.y, wy[k + 1], acc);
        acc = fmaf(c4.z, wy[k + 2], acc);
        acc = fmaf(c4.w, wy[k + 3], acc);
      }
      const float d = xm - sc[r];
      const float e = pmi_gauss(q.c2, d);
      const float eh = e * acc;
      sx += e;
      t1 = fmaf(eh, d, t1);
      t2 += eh;
      t3 = fmaf(e, d, t3);
    }
    const float sum = -2.f * q.p * (t1 - (t2 / sx) * t3);
    out[idx] = inside ? up * (sum / sx) : 0.f * (up * (sum / sx));   // outside: 0, or NaN where the item's mi is NaN
  }
}

}  // namespace mpgan

using namespace mpgan;

extern "C" int64_t mpgan_parzen_mi_workspace(int32_t batch, int64_t numel_per_item, int32_t bins) {
  if (batch < 1 || numel_per_item < 1 || bins < 2 || bins > PMI_T) return -1;
  return (int64_t)batch * pmi_slots(numel_per_item) * PMI_TILE * (int64_t)sizeof(double);
}

static int pmi_check_geometry(const char* who, int64_t n, int32_t batch, float lo_a, float hi_a, float lo_b, float hi_b,
                              int32_t bins, double sigma_ratio) {
  MPGAN_CHECK_ARG(bins >= 2 && bins <= PMI_T, "%s: bins %d outside [2, 32]", who, bins);
  MPGAN_CHECK_ARG(batch >= 1 && batch <= 65535, "%s: batch %d outside [1, 65535]", who, batch);
  MPGAN_CHECK_ARG(n >= 1, "%s: numel_per_item < 1", who);
  if (int rc = check_bin_range(who, lo_a, hi_a, bins, nullptr)) return rc;
  if (int rc = check_bin_range(who, lo_b, hi_b, bins, nullptr)) return rc;
  MPGAN_CHECK_ARG(sigma_ratio > 0.0 && is_finite(sigma_ratio), "%s: sigma_ratio must be positive and finite",
                  who);
  return MPGAN_OK;
}

static double pmi_preterm(int32_t bins, double sigma_ratio) {
  const double sigma = sigma_ratio / (double)(bins - 1);
  return 1.0 / (2.0 * sigma * sigma);
}
constexpr double PMI_LOG2E = 1.4426950408889634;

extern "C" int mpgan_parzen_mi_forward(const float* a, const float* b, int64_t numel_per_item, int32_t batch, float lo_a,
                                       float hi_a, float lo_b, float hi_b, int32_t bins, double sigma_ratio,
                                       double smooth_nr, double smooth_dr, void* workspace, int64_t workspace_bytes,
                                       double* joint, double* mi, float* coef, int32_t reduction, float* loss,
                                       void* stream) {
  MPGAN_CHECK_ARG(a && b && mi, "parzen_mi_forward: null pointer");
  if (int rc = pmi_check_geometry("parzen_mi_forward", numel_per_item, batch, lo_a, hi_a, lo_b, hi_b, bins, sigma_ratio))
    return rc;
  if (int rc = check_reduction("parzen_mi_forward", reduction)) return rc;
  if (int rc = check_workspace("parzen_mi_forward", workspace, workspace_bytes,
                               mpgan_parzen_mi_workspace(batch, numel_per_item, bins)))
    return rc;
  PmiJoint q;
  q.a = a; q.b = b; q.n = numel_per_item;
  q.slots = pmi_slots(numel_per_item);
  q.lo_a = lo_a; q.span_a = hi_a - lo_a; q.lo_b = lo_b; q.span_b = hi_b - lo_b;
  q.c2 = (float)(-pmi_preterm(bins, sigma_ratio) * PMI_LOG2E);
  q.bins = bins;
  q.ws = static_cast<double*>(workspace);
  const long blocks = q.slots;
  MPGAN_CHECK_ARG(blocks < (1L << 31), "parzen_mi_forward: too many blocks");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pmi_joint_kernel, dim3((unsigned)blocks, (unsigned)batch), dim3(64 * PMI_WAVES), 0, st, q);
  hipLaunchKernelGGL(pmi_finalize_kernel, dim3((unsigned)batch), dim3(PMI_TILE), 0, st, (const double*)q.ws, q.slots,
                     (long)numel_per_item, (int)bins, smooth_nr, smooth_dr, joint, mi, coef);
  if (loss)
    hipLaunchKernelGGL(pmi_loss_kernel, dim3(1), dim3(64), 0, st, (const double*)mi, (int)batch, (int)reduction, loss);
  return check_launch("parzen_mi_forward");
}

extern "C" int mpgan_parzen_mi_backward(const float* a, const float* b, int64_t numel_per_item, int32_t batch, float lo_a,
                                        float hi_a, float lo_b, float hi_b, int32_t bins, double sigma_ratio,
                                        const float* coef, const float* upstream, int32_t upstream_stride, float scale,
                                        int32_t wrt, float* grad, void* stream) {
  MPGAN_CHECK_ARG(a && b && coef && upstream && grad, "parzen_mi_backward: null pointer");
  if (int rc = pmi_check_geometry("parzen_mi_backward", numel_per_item, batch, lo_a, hi_a, lo_b, hi_b, bins, sigma_ratio))
    return rc;
  if (int rc = check_wrt("parzen_mi_backward", wrt)) return rc;
  if (int rc = check_upstream_stride("parzen_mi_backward", upstream_stride)) return rc;
  MPGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(coef) & 15) == 0, "parzen_mi_backward: coef must be 16-byte aligned");
  PmiBwd q;
  q.x = wrt == 0 ? a : b;
  q.y = wrt == 0 ? b : a;
  q.n = numel_per_item;
  q.lo_x = wrt == 0 ? lo_a : lo_b; q.span_x = wrt == 0 ? hi_a - lo_a : hi_b - lo_b;
  q.lo_y = wrt == 0 ? lo_b : lo_a; q.span_y = wrt == 0 ? hi_b - lo_b : hi_a - lo_a;
  q.p = (float)pmi_preterm(bins, sigma_ratio);
  q.c2 = (float)(-pmi_preterm(bins, sigma_ratio) * PMI_LOG2E);
  q.scale = (float)((double)scale / ((double)numel_per_item * (double)q.span_x));
  q.bins = bins; q.wrt = wrt; q.up_stride = upstream_stride;
  q.coef = coef; q.upstream = upstream; q.grad = grad;
  long blocks = (numel_per_item + 255) / 256;
  const long cap = 4096 / batch > 1 ? 4096 / batch : 1;
  if (blocks > cap) blocks = cap;
  const dim3 grid((unsigned)blocks, (unsigned)batch), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (bins <= 8) hipLaunchKernelGGL((pmi_backward_kernel<8>), grid, block, 0, st, q);
  else if (bins <= 16) hipLaunchKernelGGL((pmi_backward_kernel<16>), grid, block, 0, st, q);
  else if (bins <= 24) hipLaunchKernelGGL((pmi_backward_kernel<24>), grid, block, 0, st, q);
  else hipLaunchKernelGGL((pmi_backward_kernel<32>), grid, block, 0, st, q);
  return check_launch("parzen_mi_backward");
}
