// Differentiable augmentation in front of the discriminator (include/mpgan_hip.h): per sample a
// brightness offset and a contrast factor about the sample mean, an integer translation and a cut-out box, forward and
// backward.  Both directions are the same two kernels:
//   sum     (only with MPGAN_DIFFAUG_CONTRAST) the fp64 block partials of a sample's sum: of x in the forward, of
//           g_u (the shifted, masked g_y) in the backward
//   apply   out[q] = inside the valid range and outside the box ? affine(src[q + shift]) : outside value
//           forward:  shift = t,  box = the clipped cut-out box,      affine(v) = c (v - m) + m + b,  outside = fill
//           backward: shift = -t, box = the clipped box moved by t,   affine(v) = v,  outside = 0, then c g_u + k with
//                     k = (1 - c) / N * sum g_u
//   arithmetic   element terms in fp32, every sum in fp64; m and k are rounded to fp32 once
//   sum order    per lane its elements in index order, then block_sum4 (reduce.h); one
//                plain store per block.  The apply kernel adds a sample's partials itself: lane l the partials l, l+64,
//                ... in index order, then wave_sum (every wave of every block does the same additions).
//                No atomics; the grid depends on (n, dhw) alone and no parameter is read on the host: two runs give the
//                same bits.
//   access       16-byte loads and stores when both pointers are 16-byte aligned and W % 4 == 0 (every row of every
//                sample then starts on a 16-byte boundary): a shift that is no multiple of 4 takes the two aligned quads
//                its output quad straddles.  Element by element otherwise.
//   offsets      n * N < 2^31 is required of the caller's geometry, so every element offset fits 32 bits.
#include "mpgan_common.h"

namespace mpgan {

constexpr int DA_THREADS = 256;
constexpr int DA_PER_BLOCK = 1024;        // elements per block and sweep: one quad per lane
constexpr int DA_MAX_BLOCKS = 512;        // blocks per sample; larger samples: the blocks sweep again

static inline int da_blocks(long N) {
  long b = (N + DA_PER_BLOCK - 1) / DA_PER_BLOCK;
  return (int)(b > DA_MAX_BLOCKS ? DA_MAX_BLOCKS : b);
}

constexpr int DA_OPS_ALL = MPGAN_DIFFAUG_BRIGHTNESS | MPGAN_DIFFAUG_CONTRAST | MPGAN_DIFFAUG_TRANSLATION | MPGAN_DIFFAUG_CUTOUT;

struct DaDims {
  int D, H, W;
  FastDiv divH, divW, divWQ;    // row = unit / W (or quad / (W/4)), d = row / H
};

// One sample's gather: out[q] reads src[q + sh] for q in [lo, hi) per axis and outside [blo, bhi); every bound is
// clamped into [0, S], so all coordinate arithmetic stays within int32.
struct DaXform {
  int sh[3], lo[3], hi[3], blo[3], bhi[3];
};

__device__ __forceinline__ int da_clamp(long v, int s) { return (int)(v < 0 ? 0 : (v > s ? s : v)); }

// backward = false: the forward gather; true: the gather that produces g_u.  plain: no shift, no box (the sum of x).
__device__ __forceinline__ DaXform da_xform(const int32_t* __restrict__ geom, int s, const DaDims& dm, int ops,
                                            bool backward, bool plain) {
  DaXform x;
  const int S[3] = {dm.D, dm.H, dm.W};
  const bool tr = !plain && (ops & MPGAN_DIFFAUG_TRANSLATION), cut = !plain && (ops & MPGAN_DIFFAUG_CUTOUT);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    long t = tr ? (long)geom[s * 9 + k] : 0;
    t = t < -(long)S[k] ? -(long)S[k] : (t > S[k] ? S[k] : t);          // |t| > S is all outside too
    const long sh = backward ? -t : t;
    x.sh[k] = (int)sh;
    x.lo[k] = da_clamp(-sh, S[k]);
    x.hi[k] = da_clamp((long)S[k] - sh, S[k]);
    long b0 = 0, b1 = 0;
    if (cut) {
      const long l = geom[s * 9 + 3 + k], z = geom[s * 9 + 6 + k];
      b0 = da_clamp(l, S[k]);
      b1 = da_clamp(l + (z > 0 ? z : 0), S[k]);
      if (backward) { b0 += t; b1 += t; }     // the box is on g_y's coordinates p = q - t
    }
    x.blo[k] = da_clamp(b0, S[k]);
    x.bhi[k] = da_clamp(b1, S[k]);
  }
  return x;
}

__device__ __forceinline__ bool da_in(int v, int lo, int hi) { return v >= lo && v < hi; }

// The gathered values of one unit (VEC: the quad at row `row`, columns w0 .. w0+3; else one element) and their keep
// flags.  src is the sample's base.  Masked lanes of a quad read nothing that lies outside the row.
template <bool VEC>
__device__ __forceinline__ void da_gather(const float* __restrict__ src, const DaDims& dm, const DaXform& x, unsigned unit,
                                          float v[4], bool keep[4]) {
  unsigned row, wu;
  fdivmod(unit, VEC ? dm.divWQ : dm.divW, row, wu);
  unsigned d, h;
  fdivmod(row, dm.divH, d, h);
  const int w0 = VEC ? (int)wu * 4 : (int)wu;
  const bool row_ok = da_in((int)d, x.lo[0], x.hi[0]) && da_in((int)h, x.lo[1], x.hi[1]);
  const bool row_box = da_in((int)d, x.blo[0], x.bhi[0]) && da_in((int)h, x.blo[1], x.bhi[1]);
  constexpr int E = VEC ? 4 : 1;
  bool any = false;
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int w = w0 + k;
    keep[k] = row_ok && da_in(w, x.lo[2], x.hi[2]) && !(row_box && da_in(w, x.blo[2], x.bhi[2]));
    any |= keep[k];
    v[k] = 0.f;
  }
  if (!any) return;
  // row_ok holds: the source row lies inside the sample
  const int srow = ((int)d + x.sh[0]) * dm.H + ((int)h + x.sh[1]);
  const float* __restrict__ sp = src + (long)srow * dm.W;
  if (VEC) {
    const int r = x.sh[2] & 3;                       // the same in every lane of a sample's blocks
    const int a = w0 + x.sh[2] - r;                  // aligned: w0, sh - r are multiples of 4
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f), B = A;
    if (a >= 0 && a + 4 <= dm.W) A = *reinterpret_cast<const float4*>(sp + a);
    if (r != 0 && a + 4 >= 0 && a + 8 <= dm.W) B = *reinterpret_cast<const float4*>(sp + a + 4);
    switch (r) {
      case 0: v[0] = A.x; v[1] = A.y; v[2] = A.z; v[3] = A.w; break;
      case 1: v[0] = A.y; v[1] = A.z; v[2] = A.w; v[3] = B.x; break;
      case 2: v[0] = A.z; v[1] = A.w; v[2] = B.x; v[3] = B.y; break;
      default: v[0] = A.w; v[1] = B.x; v[2] = B.y; v[3] = B.z; break;
    }
  } else {
    v[0] = sp[w0 + x.sh[2]];                         // keep[0]: w0 + sh lies in [0, W)
  }
}

template <bool VEC>
__global__ __launch_bounds__(DA_THREADS) void diffaug_sum_kernel(const float* __restrict__ src, DaDims dm, unsigned units,
                                                                 int bps, int ops, const int32_t* __restrict__ geom,
                                                                 int backward, double* __restrict__ partials) {
  __shared__ double sh[4];
  const int s = blockIdx.x / bps, blk = blockIdx.x - s * bps;
  const DaXform x = da_xform(geom, s, dm, ops, backward != 0, backward == 0);
  const float* __restrict__ base = src + (long)s * ((long)dm.D * dm.H * dm.W);
  double acc = 0.0;
  for (unsigned u = blk * DA_THREADS + threadIdx.x; u < units; u += (unsigned)bps * DA_THREADS) {
    float v[4];
    bool keep[4];
    da_gather<VEC>(base, dm, x, u, v, keep);
#pragma unroll
    for (int k = 0; k < (VEC ? 4 : 1); ++k) acc += keep[k] ? (double)v[k] : 0.0;
  }
  acc = block_sum4(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

template <bool VEC>
__global__ __launch_bounds__(DA_THREADS) void diffaug_apply_kernel(const float* __restrict__ src, DaDims dm, unsigned units,
                                                                   int bps, int ops, const float* __restrict__ color,
                                                                   const int32_t* __restrict__ geom, float fill,
                                                                   int backward, const double* __restrict__ partials,
                                                                   float* __restrict__ dst) {
  const int s = blockIdx.x / bps, blk = blockIdx.x - s * bps;
  const DaXform x = da_xform(geom, s, dm, ops, backward != 0, false);
  const long N = (long)dm.D * dm.H * dm.W;
  const float* __restrict__ base = src + (long)s * N;
  float* __restrict__ out = dst + (long)s * N;
  const bool bright = ops & MPGAN_DIFFAUG_BRIGHTNESS, contrast = ops & MPGAN_DIFFAUG_CONTRAST;
  const float b = bright ? color[s * 2] : 0.f, c = contrast ? color[s * 2 + 1] : 1.f;
  float m = 0.f;                                     // forward: the sample mean; backward: k = (1 - c) / N * sum g_u
  if (contrast) {
    double t = 0.0;
    for (int j = threadIdx.x & 63; j < bps; j += 64) t += partials[s * bps + j];
    t = wave_sum(t);
    m = backward ? (float)((1.0 - (double)c) * t / (double)N) : (float)(t / (double)N);
  }
  const float outside = backward ? 0.f : fill;
  for (unsigned u = blk * DA_THREADS + threadIdx.x; u < units; u += (unsigned)bps * DA_THREADS) {
    float v[4];
    bool keep[4];
    da_gather<VEC>(base, dm, x, u, v, keep);
#pragma unroll
    for (int k = 0; k < (VEC ? 4 : 1); ++k) {
      float r = v[k];
      if (backward) {
        r = keep[k] ? r : 0.f;
        if (contrast) r = c * r + m;
      } else {
        if (contrast) r = c * (r - m) + m + b;
        else if (bright) r = r + b;
        r = keep[k] ? r : outside;
      }
      v[k] = r;
    }
    if (VEC) reinterpret_cast<float4*>(out)[u] = make_float4(v[0], v[1], v[2], v[3]);
    else out[u] = v[0];
  }
}

}  // namespace mpgan

using namespace mpgan;

static inline bool da_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Geometry common to the three entry points: 0 and *N, or -1 with the error set.
static int da_geometry(const char* who, int32_t n, const int32_t* dhw, long* N) {
  MPGAN_CHECK_ARG(dhw != nullptr, "%s: bad argument (null dhw)", who);
  MPGAN_CHECK_ARG(n > 0, "%s: bad argument (n = %d)", who, n);
  return element_count(who, "", n, dhw, N);
}

extern "C" int64_t mpgan_diffaug_workspace(int32_t n, const int32_t* dhw) {
  long N;
  if (da_geometry("mpgan_diffaug_workspace", n, dhw, &N) != MPGAN_OK) return -1;
  return (int64_t)n * da_blocks(N) * (int64_t)sizeof(double);
}

static int da_run(const char* who, const float* src, int32_t n, const int32_t* dhw, int32_t ops, const float* color,
                  const int32_t* geom, float fill, void* ws, int64_t ws_bytes, float* dst, bool backward, void* stream) {
  long N;
  if (int rc = da_geometry(who, n, dhw, &N)) return rc;
  MPGAN_CHECK_ARG((ops & ~DA_OPS_ALL) == 0, "%s: unknown ops bits 0x%x (brightness 1, contrast 2, translation 4, cutout 8)",
                  who, ops);
  MPGAN_CHECK_ARG(src && dst, "%s: bad argument (null pointer)", who);
  MPGAN_CHECK_ARG(!(ops & (MPGAN_DIFFAUG_BRIGHTNESS | MPGAN_DIFFAUG_CONTRAST)) || color,
                  "%s: bad argument (null color with a colour op)", who);
  MPGAN_CHECK_ARG(!(ops & (MPGAN_DIFFAUG_TRANSLATION | MPGAN_DIFFAUG_CUTOUT)) || geom,
                  "%s: bad argument (null geom with a spatial op)", who);
  const int bps = da_blocks(N);
  const bool contrast = ops & MPGAN_DIFFAUG_CONTRAST;
  if (contrast) {
    MPGAN_CHECK_ARG(ws != nullptr, "%s: bad argument (null workspace with contrast)", who);
    MPGAN_CHECK_ARG(ws_bytes >= (int64_t)n * bps * (int64_t)sizeof(double), "%s: workspace of %lld bytes, needs %lld", who,
                    (long long)ws_bytes, (long long)((int64_t)n * bps * (int64_t)sizeof(double)));
    MPGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "%s: workspace must be 8-byte aligned", who);
  }
  DaDims dm;
  dm.D = dhw[0]; dm.H = dhw[1]; dm.W = dhw[2];
  const bool vec = da_al16(src) && da_al16(dst) && (dm.W & 3) == 0;
  dm.divH = make_fastdiv((unsigned)dm.H);
  dm.divW = make_fastdiv((unsigned)dm.W);
  dm.divWQ = make_fastdiv((unsigned)(vec ? dm.W / 4 : 1));
  const unsigned units = (unsigned)(vec ? N / 4 : N);
  const dim3 grid((unsigned)(n * bps)), block(DA_THREADS);     // n * bps <= n * N / 1024 + n < 2^31
  double* partials = static_cast<double*>(ws);
  const int bw = backward ? 1 : 0;
  if (contrast) {
    if (vec)
      hipLaunchKernelGGL(diffaug_sum_kernel<true>, grid, block, 0, (hipStream_t)stream, src, dm, units, bps, (int)ops, geom,
                         bw, partials);
    else
      hipLaunchKernelGGL(diffaug_sum_kernel<false>, grid, block, 0, (hipStream_t)stream, src, dm, units, bps, (int)ops, geom,
                         bw, partials);
  }
  if (vec)
    hipLaunchKernelGGL(diffaug_apply_kernel<true>, grid, block, 0, (hipStream_t)stream, src, dm, units, bps, (int)ops, color,
                       geom, fill, bw, static_cast<const double*>(partials), dst);
  else
    hipLaunchKernelGGL(diffaug_apply_kernel<false>, grid, block, 0, (hipStream_t)stream, src, dm, units, bps, (int)ops, color,
                       geom, fill, bw, static_cast<const double*>(partials), dst);
  return check_launch(who);
}

extern "C" int mpgan_diffaug_forward(const float* x, int32_t n, const int32_t* dhw, int32_t ops, const float* color,
                                     const int32_t* geom, float fill, void* ws, int64_t ws_bytes, float* y, void* stream) {
  return da_run("mpgan_diffaug_forward", x, n, dhw, ops, color, geom, fill, ws, ws_bytes, y, false, stream);
}

extern "C" int mpgan_diffaug_backward(const float* gy, int32_t n, const int32_t* dhw, int32_t ops, const float* color,
                                      const int32_t* geom, void* ws, int64_t ws_bytes, float* gx, void* stream) {
  return da_run("mpgan_diffaug_backward", gy, n, dhw, ops, color, geom, 0.f, ws, ws_bytes, gx, true, stream);
}
