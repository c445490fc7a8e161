// The optimiser step's optional extras over the flat parameter buffer (include/mpgan_hip.h): the
// gradient's global norm with torch's clip coefficient, an Adam step that reads that coefficient from the device and
// leaves an exponential moving average of the new parameters, and the table-driven EMA of the norm buffers.
//   norm         g_i * grad_scale rounded to fp32 (the value Adam loads), its square and every sum in fp64: per lane
//                its elements in index order, then block_sum4 (reduce.h), one plain store per block; a second,
//                one-block launch adds the block partials by strided_serial_sum256.  No atomics and a grid that
//                depends on numel alone: two runs give the same bits.
//   Adam         adam_kernel's operations (loss_ops.hip) element for element; the coefficient is one scalar
//                load per thread, so clipping needs no host sync.
//   access       16-byte loads and stores when every participating pointer is 16-byte aligned (scalar tail),
//                element by element otherwise.  All HBM-bound, no reuse.
#include "mpgan_common.h"

namespace mpgan {

constexpr int GN_PER_BLOCK = 1024;    // elements per block and sweep: one quad per lane
constexpr int GN_MAX_BLOCKS = 1024;   // beyond 2^20 elements the blocks sweep again (grid-stride)
constexpr int OPT_MAX_BLOCKS = 4096;  // the element-wise kernels: as adam_kernel's launch

static inline int gn_blocks(long numel) {
  long b = (numel + GN_PER_BLOCK - 1) / GN_PER_BLOCK;
  return (int)(b > GN_MAX_BLOCKS ? GN_MAX_BLOCKS : (b < 1 ? 1 : b));
}

static inline int opt_blocks(long work) {
  long b = (work + 255) / 256;
  return (int)(b > OPT_MAX_BLOCKS ? OPT_MAX_BLOCKS : (b < 1 ? 1 : b));
}

__device__ __forceinline__ double gn_sq(float g, float gscale) {
  const double x = (double)(g * gscale);   // the fp32 product, then fp64
  return x * x;
}

// ---- gradient norm -------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const float* __restrict__ g, long numel, float gscale,
                                                                double* __restrict__ partials) {
  __shared__ double sh[4];
  const long gt = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
  double acc = 0.0;
  if (VEC) {
    const long quads = numel >> 2;
    for (long q = gt; q < quads; q += stride) {
      const float4 v = reinterpret_cast<const float4*>(g)[q];
      acc += gn_sq(v.x, gscale);
      acc += gn_sq(v.y, gscale);
      acc += gn_sq(v.z, gscale);
      acc += gn_sq(v.w, gscale);
    }
    if (gt < (numel & 3)) acc += gn_sq(g[quads * 4 + gt], gscale);   // the tail: threads 0..2 of block 0
  } else {
    for (long i = gt; i < numel; i += stride) acc += gn_sq(g[i], gscale);
  }
  acc = block_sum4(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// out2 = (norm, clip coefficient): torch.nn.utils.clip_grad_norm_'s clamp(max_norm / (norm + 1e-6), max=1.0) in fp32;
// a non-finite norm goes through the same expressions
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const double* __restrict__ partials, int blocks,
                                                              float max_norm, float* __restrict__ out2) {
  __shared__ double sh[256];
  const double t = strided_serial_sum256(partials, blocks, sh);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(t);
    out2[0] = norm;
    float coef = 1.f;
    if (max_norm > 0.f) {
      const float c = max_norm / (norm + 1e-6f);
      coef = c > 1.f ? 1.f : c;              // torch.clamp(max=1.0): a NaN stays a NaN
    }
    out2[1] = coef;
  }
}

// ---- Adam with a device clip coefficient and an EMA of the result ------------------------------------------------
struct AdamK {
  float w1, b2, one_minus_b2, step_size, bc2_sqrt, eps, gscale, ema_w;
};

// torch's lerp: start + w*(end-start) for w < 0.5, else end - (end-start)*(1-w), each as one fused multiply-add
__device__ __forceinline__ float lerp_t(float a, float b, float w) {
#pragma clang fp contract(off)
  const float diff = b - a;
  return w < 0.5f ? __builtin_fmaf(w, diff, a) : __builtin_fmaf(-(1.f - w), diff, b);
}

// One element: adam_kernel's statements (loss_ops.hip) in their order, with every rounding spelled out.  adam_kernel
// leaves the fusing of its multiplies and adds to the compiler, and whether a product is fused depends on the code
// around it; its results must be met bit for bit, so the operations here are the ones its gfx950 code performs:
// g*gs is fused into the first-moment difference and into nothing else, both lerp branches and the parameter update
// are one fma each, and the second moment is two rounded products and an add.  gs = grad_scale [* coef] is one fp32
// product made once per thread, so that a coefficient of exactly 1.0f changes no bit whatever grad_scale is.
template <bool EMA>
__device__ __forceinline__ void adam_elem(float& pi, float graw, float& mi, float& vi, float& ei, const AdamK& k,
                                          float gs) {
#pragma clang fp contract(off)
  const float gi = graw * gs;
  // torch: exp_avg.lerp_(grad, 1-beta1)
  const float diff = __builtin_fmaf(graw, gs, -mi);
  mi = k.w1 < 0.5f ? __builtin_fmaf(k.w1, diff, mi) : __builtin_fmaf(-(1.f - k.w1), diff, gi);
  vi = vi * k.b2 + (k.one_minus_b2 * gi) * gi;
  const float denom = sqrtf(vi) / k.bc2_sqrt + k.eps;
  pi = __builtin_fmaf(-k.step_size, mi / denom, pi);
  if (EMA) ei = lerp_t(ei, pi, k.ema_w);
}

template <bool COEF, bool EMA, bool VEC>
__global__ __launch_bounds__(256) void adam_ex_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                      float* __restrict__ m, float* __restrict__ v,
                                                      float* __restrict__ ema, long numel, AdamK k,
                                                      const float* __restrict__ coef_ptr) {
  const float gs = COEF ? k.gscale * coef_ptr[0] : k.gscale;
  const long gt = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
  if (VEC) {
    const long quads = numel >> 2;
    for (long q = gt; q < quads; q += stride) {
      float4 pv = reinterpret_cast<float4*>(p)[q];
      const float4 gv = reinterpret_cast<const float4*>(g)[q];
      float4 mv = reinterpret_cast<float4*>(m)[q];
      float4 vv = reinterpret_cast<float4*>(v)[q];
      float4 ev = make_float4(0.f, 0.f, 0.f, 0.f);
      if (EMA) ev = reinterpret_cast<float4*>(ema)[q];
      adam_elem<EMA>(pv.x, gv.x, mv.x, vv.x, ev.x, k, gs);
      adam_elem<EMA>(pv.y, gv.y, mv.y, vv.y, ev.y, k, gs);
      adam_elem<EMA>(pv.z, gv.z, mv.z, vv.z, ev.z, k, gs);
      adam_elem<EMA>(pv.w, gv.w, mv.w, vv.w, ev.w, k, gs);
      reinterpret_cast<float4*>(p)[q] = pv;
      reinterpret_cast<float4*>(m)[q] = mv;
      reinterpret_cast<float4*>(v)[q] = vv;
      if (EMA) reinterpret_cast<float4*>(ema)[q] = ev;
    }
    if (gt < (numel & 3)) {                        // the tail: threads 0..2 of block 0
      const long i = quads * 4 + gt;
      float pi = p[i], mi = m[i], vi = v[i], ei = EMA ? ema[i] : 0.f;
      adam_elem<EMA>(pi, g[i], mi, vi, ei, k, gs);
      p[i] = pi;
      m[i] = mi;
      v[i] = vi;
      if (EMA) ema[i] = ei;
    }
  } else {
    for (long i = gt; i < numel; i += stride) {
      float pi = p[i], mi = m[i], vi = v[i], ei = EMA ? ema[i] : 0.f;
      adam_elem<EMA>(pi, g[i], mi, vi, ei, k, gs);
      p[i] = pi;
      m[i] = mi;
      v[i] = vi;
      if (EMA) ema[i] = ei;
    }
  }
}

template <bool COEF, bool EMA>
static void launch_adam_ex(bool vec, int blocks, hipStream_t s, float* p, const float* g, float* m, float* v, float* ema,
                           long numel, const AdamK& k, const float* coef) {
  if (vec)
    hipLaunchKernelGGL((adam_ex_kernel<COEF, EMA, true>), dim3(blocks), dim3(256), 0, s, p, g, m, v, ema, numel, k, coef);
  else
    hipLaunchKernelGGL((adam_ex_kernel<COEF, EMA, false>), dim3(blocks), dim3(256), 0, s, p, g, m, v, ema, numel, k, coef);
}

// ---- EMA of the norm buffers (table driven, one launch per network) ----------------------------------------------
// rows [src_ptr, dst_ptr, numel, kind]: kind 0 dst = lerp(dst, src, w) over fp32, kind 1 dst = src over int64
__global__ __launch_bounds__(256) void ema_buffers_kernel(const int64_t* __restrict__ table, float w) {
  const int64_t* e = table + (long)blockIdx.y * 4;
  const long n = e[2];
  const long stride = (long)gridDim.x * blockDim.x;
  if (e[3] == 0) {
    const float* src = reinterpret_cast<const float*>(e[0]);
    float* dst = reinterpret_cast<float*>(e[1]);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = lerp_t(dst[i], src[i], w);
  } else {
    const int64_t* src = reinterpret_cast<const int64_t*>(e[0]);
    int64_t* dst = reinterpret_cast<int64_t*>(e[1]);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[i];
  }
}

}  // namespace mpgan

using namespace mpgan;

static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

extern "C" int64_t mpgan_grad_norm_workspace(int64_t numel) {
  if (numel <= 0) {
    set_error("mpgan_grad_norm_workspace: bad argument (numel = %lld)", (long long)numel);
    return -1;
  }
  return (int64_t)gn_blocks(numel) * (int64_t)sizeof(double);
}

extern "C" int mpgan_grad_norm(const float* g, int64_t numel, float grad_scale, float max_norm, void* ws,
                               int64_t ws_bytes, float* out2, void* stream) {
  MPGAN_CHECK_ARG(numel > 0, "mpgan_grad_norm: bad argument (numel = %lld)", (long long)numel);
  MPGAN_CHECK_ARG(g && ws && out2, "mpgan_grad_norm: bad argument (null pointer)");
  MPGAN_CHECK_ARG(al4(g) && al4(out2) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
                  "mpgan_grad_norm: g / out2 must be 4-byte and the workspace 8-byte aligned");
  const int blocks = gn_blocks(numel);
  MPGAN_CHECK_ARG(ws_bytes >= (int64_t)blocks * (int64_t)sizeof(double),
                  "mpgan_grad_norm: workspace of %lld bytes, needs %lld", (long long)ws_bytes,
                  (long long)blocks * (long long)sizeof(double));
  double* partials = static_cast<double*>(ws);
  if (al16(g))
    hipLaunchKernelGGL(grad_norm_partial_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, (long)numel,
                       grad_scale, partials);
  else
    hipLaunchKernelGGL(grad_norm_partial_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, g, (long)numel,
                       grad_scale, partials);
  hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream,
                     static_cast<const double*>(partials), blocks, max_norm, out2);
  return check_launch("mpgan_grad_norm");
}

extern "C" int mpgan_adam_step_ex(float* p, const float* g, float* m, float* v, int64_t numel, double lr, double b1,
                                  double b2, double eps, int32_t step, float grad_scale, const float* coef, float* ema,
                                  float ema_weight, void* stream) {
  MPGAN_CHECK_ARG(numel > 0 && step > 0, "mpgan_adam_step_ex: bad argument (numel = %lld, step = %d)",
                  (long long)numel, step);
  MPGAN_CHECK_ARG(p && g && m && v, "mpgan_adam_step_ex: bad argument (null pointer)");
  MPGAN_CHECK_ARG(al4(p) && al4(g) && al4(m) && al4(v) && al4(coef) && al4(ema),
                  "mpgan_adam_step_ex: every pointer must be 4-byte aligned");
  MPGAN_CHECK_ARG(!ema || (ema_weight >= 0.f && ema_weight <= 1.f),
                  "mpgan_adam_step_ex: ema_weight %g outside [0, 1]", (double)ema_weight);
  const double bc1 = 1.0 - pow(b1, (double)step);
  const double bc2 = 1.0 - pow(b2, (double)step);
  AdamK k;
  k.w1 = (float)(1.0 - b1);
  k.b2 = (float)b2;
  k.one_minus_b2 = (float)(1.0 - b2);
  k.step_size = (float)(lr / bc1);
  k.bc2_sqrt = (float)sqrt(bc2);
  k.eps = (float)eps;
  k.gscale = grad_scale;
  k.ema_w = ema_weight;
  const bool vec = al16(p) && al16(g) && al16(m) && al16(v) && (ema == nullptr || al16(ema));
  const int blocks = opt_blocks(vec ? (long)((numel + 3) / 4) : (long)numel);
  hipStream_t s = (hipStream_t)stream;
  if (coef && ema) launch_adam_ex<true, true>(vec, blocks, s, p, g, m, v, ema, (long)numel, k, coef);
  else if (coef) launch_adam_ex<true, false>(vec, blocks, s, p, g, m, v, ema, (long)numel, k, coef);
  else if (ema) launch_adam_ex<false, true>(vec, blocks, s, p, g, m, v, ema, (long)numel, k, coef);
  else launch_adam_ex<false, false>(vec, blocks, s, p, g, m, v, ema, (long)numel, k, coef);
  return check_launch("mpgan_adam_step_ex");
}

extern "C" int mpgan_ema_buffers(const int64_t* table, int32_t n_entries, int64_t max_elems, float ema_weight,
                                 void* stream) {
  MPGAN_CHECK_ARG(n_entries >= 0 && n_entries <= 65535, "mpgan_ema_buffers: bad argument (n_entries = %d, 0..65535)",
                  n_entries);
  if (n_entries == 0) return MPGAN_OK;
  MPGAN_CHECK_ARG(table != nullptr, "mpgan_ema_buffers: bad argument (null table)");
  MPGAN_CHECK_ARG(max_elems > 0, "mpgan_ema_buffers: bad argument (max_elems = %lld)", (long long)max_elems);
  MPGAN_CHECK_ARG(ema_weight >= 0.f && ema_weight <= 1.f, "mpgan_ema_buffers: ema_weight %g outside [0, 1]",
                  (double)ema_weight);
  long bx = (max_elems + 255) / 256;
  if (bx > 256) bx = 256;
  hipLaunchKernelGGL(ema_buffers_kernel, dim3((unsigned)bx, (unsigned)n_entries), dim3(256), 0, (hipStream_t)stream,
                     table, ema_weight);
  return check_launch("mpgan_ema_buffers");
}
