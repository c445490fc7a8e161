// Adversarial objectives computed on the discriminator's LOGITS (include/mpgan_hip.h): the numerically
// stable cross-entropy (F.binary_cross_entropy_with_logits) and least squares (F.mse_loss, LSGAN).  One launch leaves
// the mean loss's block partials and dL/dlogit for an upstream gradient of 1; a second, tiny one adds the partials
// (a single block finishes on its own).
//   arithmetic   element terms in fp32, every sum in fp64
//   sum order    per lane its elements in index order, then block_sum4 (reduce.h); one plain store per block; the
//                block partials in index order.  No atomics, and the grid depends on n
//                alone: two runs give the same bits.
//   access       16-byte loads and stores when logit / target / grad are 16-byte aligned, the n % 4 last elements
//                scalar; element by element otherwise.
#include "mpgan_common.h"

namespace mpgan {

constexpr int ADV_PER_BLOCK = 1024;    // elements per block and sweep: one quad per lane
constexpr int ADV_MAX_BLOCKS = 1024;   // more elements than 2^20: the blocks sweep again (grid-stride)

static inline int adv_blocks(long n) {
  long b = (n + ADV_PER_BLOCK - 1) / ADV_PER_BLOCK;
  return (int)(b > ADV_MAX_BLOCKS ? ADV_MAX_BLOCKS : b);
}

// term and dterm/dz * (1/n) of one element.  BCE: sigma from one exp of a non-positive argument, one add and one
// divide, so neither branch overflows; for z -> -inf the gradient tends to -t/n and does not vanish.
template <int KIND>
__device__ __forceinline__ float adv_elem(float z, float t, float nf, float* g) {
  if (KIND == MPGAN_ADV_BCE_LOGITS) {
    const float e = expf(-fabsf(z));
    const float sig = (z >= 0.f ? 1.f : e) / (1.f + e);
    *g = (sig - t) / nf;
    return fmaxf(z, 0.f) - z * t + log1pf(e);
  }
  const float d = z - t;
  *g = (2.f * d) / nf;
  return d * d;
}

template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void adv_loss_kernel(const float* __restrict__ logit,
                                                       const float* __restrict__ target, int n,
                                                       double* __restrict__ partials, float* __restrict__ loss,
                                                       float* __restrict__ grad) {
  __shared__ double sh[4];
  const float nf = (float)n;
  const long gt = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
  double acc = 0.0;
  if (VEC) {
    const long quads = n >> 2;
    for (long q = gt; q < quads; q += stride) {
      const float4 z = reinterpret_cast<const float4*>(logit)[q];
      const float4 t = reinterpret_cast<const float4*>(target)[q];
      float4 g;
      acc += (double)adv_elem<KIND>(z.x, t.x, nf, &g.x);
      acc += (double)adv_elem<KIND>(z.y, t.y, nf, &g.y);
      acc += (double)adv_elem<KIND>(z.z, t.z, nf, &g.z);
      acc += (double)adv_elem<KIND>(z.w, t.w, nf, &g.w);
      if (grad) reinterpret_cast<float4*>(grad)[q] = g;
    }
    if (gt < (n & 3)) {                            // the tail: threads 0..2 of block 0, after their quads
      const long i = quads * 4 + gt;
      float g;
      acc += (double)adv_elem<KIND>(logit[i], target[i], nf, &g);
      if (grad) grad[i] = g;
    }
  } else {
    for (long i = gt; i < n; i += stride) {
      float g;
      acc += (double)adv_elem<KIND>(logit[i], target[i], nf, &g);
      if (grad) grad[i] = g;
    }
  }
  const double s = block_sum4(acc, sh);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = s;
    if (gridDim.x == 1) *loss = (float)(s / (double)n);
  }
}

__global__ void adv_loss_final_kernel(const double* __restrict__ partials, int blocks, int n,
                                      float* __restrict__ loss) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < blocks; ++k) s += partials[k];
    *loss = (float)(s / (double)n);
  }
}

}  // namespace mpgan

using namespace mpgan;

static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int32_t mpgan_adv_loss_partials(int32_t n) {
  if (n <= 0) {
    set_error("mpgan_adv_loss_partials: bad argument (n = %d)", n);
    return -1;
  }
  return adv_blocks(n);
}

extern "C" int mpgan_adv_loss(const float* logit, const float* target, int32_t n, int32_t kind, double* partials,
                              float* loss, float* grad, void* stream) {
  MPGAN_CHECK_ARG(n > 0, "mpgan_adv_loss: bad argument (n = %d)", n);
  MPGAN_CHECK_ARG(kind == MPGAN_ADV_BCE_LOGITS || kind == MPGAN_ADV_LSGAN,
                  "mpgan_adv_loss: unknown kind %d (MPGAN_ADV_BCE_LOGITS = 0, MPGAN_ADV_LSGAN = 1)", kind);
  MPGAN_CHECK_ARG(logit && target && partials && loss, "mpgan_adv_loss: bad argument (null pointer)");
  MPGAN_UNSUPPORTED((reinterpret_cast<uintptr_t>(partials) & 7) != 0, "mpgan_adv_loss: partials must be 8-byte aligned");
  const int blocks = adv_blocks(n);
  const bool vec = al16(logit) && al16(target) && (grad == nullptr || al16(grad));
  const bool bce = kind == MPGAN_ADV_BCE_LOGITS;
  auto kern = bce ? (vec ? adv_loss_kernel<MPGAN_ADV_BCE_LOGITS, true> : adv_loss_kernel<MPGAN_ADV_BCE_LOGITS, false>)
                  : (vec ? adv_loss_kernel<MPGAN_ADV_LSGAN, true> : adv_loss_kernel<MPGAN_ADV_LSGAN, false>);
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, (hipStream_t)stream, logit, target, (int)n, partials, loss, grad);
  if (blocks > 1)
    hipLaunchKernelGGL(adv_loss_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                       static_cast<const double*>(partials), blocks, (int)n, loss);
  return check_launch("mpgan_adv_loss");
}
