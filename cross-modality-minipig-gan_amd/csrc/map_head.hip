// Markovian (PatchGAN) discriminator head: a last valid convolution C -> 1 (stride 1, no padding) on the
// channels-last fp32 tensor of the last conv layer, read through the optional normalise+activate prologue, and its
// backward.  One output channel: the 32-wide MFMA forms would spend 31/32 of their columns on padding, so these are
// VALU kernels of their own (measured times and what keeps them above the byte floor: DESIGN.md 7c):
//   forward        a wave walks a strip of adjacent map pixels along x with its lanes over channel quads; every loaded
//                  and activated input vector serves kx outputs; the [taps][c] weights sit in LDS, staged once per block
//   backward data  the gather form: a wave walks a strip of input pixels along x, lanes over channel quads
//   backward weight two stages: per-chunk partials [chunk][tap][c] in the caller's workspace, then a finalize that
//                  adds the chunks in index order
// No atomics; every sum has a fixed order, so two runs on the same inputs give the same bits.
#include "mpgan_common.h"

namespace mpgan {

constexpr int MH_STRIP = 8;            // pixels along x per wave strip
constexpr int MH_BATCH = 4;            // input vectors loaded before they are used
constexpr int MH_TAPG = 16;            // taps per weight-gradient block (its accumulators: 16 float4 per lane)
constexpr int MH_LDS_BYTES = 65536;    // the weights' LDS budget: taps * c * 4 bytes

struct MapGeom {
  int n, D, H, W, KD, KH, KW, OD, OH, OW, C, taps;
};

__device__ __forceinline__ float4 mh_act(float4 v, const float sc[4], const float sh[4], int act, float slope) {
  v.x = act_apply(v.x * sc[0] + sh[0], act, slope);
  v.y = act_apply(v.y * sc[1] + sh[1], act, slope);
  v.z = act_apply(v.z * sc[2] + sh[2], act, slope);
  v.w = act_apply(v.w * sc[3] + sh[3], act, slope);
  return v;
}

__device__ __forceinline__ void mh_stage_weights(float* wl, const float* __restrict__ w, int quads) {
  for (int i = threadIdx.x; i < quads; i += 256)
    reinterpret_cast<float4*>(wl)[i] = reinterpret_cast<const float4*>(w)[i];
  __syncthreads();
}

// item = ((n*OD + oz)*xstrips + xs)*OH + oy: the four waves of a block mostly take four adjacent rows of one strip
// column, whose input rows overlap in the CU's vector cache.
// Sum order of one logit: per lane its channel quads (ascending) x taps in index order, then the lanes of the wave.
__global__ __launch_bounds__(256) void maphead_forward_kernel(const float* __restrict__ z, Pro p, MapGeom g,
                                                              const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ logit,
                                                              float* __restrict__ prob, int items, int xstrips) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  mh_stage_weights(wl, w, g.taps * (g.C >> 2));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int CQ = g.C >> 2;
  const float slope = pro_slope(p);
  const float b = bias ? bias[0] : 0.f;
  const long sample = (long)g.D * g.H * g.W * g.C;
  for (int item = blockIdx.x * 4 + wave; item < items; item += gridDim.x * 4) {
    const int oy = item % g.OH;
    int r = item / g.OH;
    const int xs = r % xstrips;
    r /= xstrips;
    const int oz = r % g.OD, n = r / g.OD;
    const int x0 = xs * MH_STRIP;
    const int len = min(MH_STRIP, g.OW - x0);
    const int span = len + g.KW - 1;               // input columns x0 .. x0+span-1 (<= W-1)
    float acc[MH_STRIP];
#pragma unroll
    for (int s = 0; s < MH_STRIP; ++s) acc[s] = 0.f;
    const float* zn = z + (long)n * sample;
    for (int qb = 0; qb < CQ; qb += 64) {
      const bool on = qb + lane < CQ;
      const int q4 = on ? (qb + lane) * 4 : 0;
      float sc[4] = {1.f, 1.f, 1.f, 1.f}, sh[4] = {0.f, 0.f, 0.f, 0.f};
      if (p.scale) {
        const int si = n * p.n_stride + q4;
#pragma unroll
        for (int e = 0; e < 4; ++e) { sc[e] = p.scale[si + e]; sh[e] = p.shift[si + e]; }
      }
      for (int tz = 0; tz < g.KD; ++tz)
        for (int ty = 0; ty < g.KH; ++ty) {
          const float* row = zn + (((long)(oz + tz) * g.H + (oy + ty)) * g.W + x0) * g.C + q4;
          const float* wrow = wl + (long)((tz * g.KH + ty) * g.KW) * g.C + q4;
          for (int i0 = 0; i0 < span; i0 += MH_BATCH) {
            float4 v[MH_BATCH];
#pragma unroll
            for (int j = 0; j < MH_BATCH; ++j) {
              v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
              if (on && i0 + j < span) v[j] = *reinterpret_cast<const float4*>(row + (long)(i0 + j) * g.C);
            }
            if (p.scale) {
#pragma unroll
              for (int j = 0; j < MH_BATCH; ++j)
                if (on && i0 + j < span) v[j] = mh_act(v[j], sc, sh, p.act, slope);
            }
#pragma unroll
            for (int j = 0; j < MH_BATCH; ++j) {
#pragma unroll
              for (int s = 0; s < MH_STRIP; ++s) {
                const int tx = i0 + j - s;         // wave-uniform
                if (tx >= 0 && tx < g.KW && s < len) {
                  const float4 ww = *reinterpret_cast<const float4*>(wrow + tx * g.C);
                  acc[s] = fmaf(v[j].w, ww.w, fmaf(v[j].z, ww.z, fmaf(v[j].y, ww.y, fmaf(v[j].x, ww.x, acc[s]))));
                }
              }
            }
          }
        }
    }
    const long o = (((long)n * g.OD + oz) * g.OH + oy) * g.OW + x0;
#pragma unroll
    for (int s = 0; s < MH_STRIP; ++s) {
      const float t = wave_sum(acc[s]) + b;
      if (lane == 0 && s < len) {
        logit[o + s] = t;
        if (prob) prob[o + s] = 1.f / (1.f + expf(-t));
      }
    }
  }
}

// g_a[n][q][c] = sum_tap dlogit[n][q - tap] * w[tap][c] over the taps that land inside the map, taps in index order.
// item = ((n*D + iz)*xstrips + xs)*H + iy.
__global__ __launch_bounds__(256) void maphead_bwd_data_kernel(MapGeom g, const float* __restrict__ w,
                                                               const float* __restrict__ dlogit,
                                                               float* __restrict__ g_a, int items, int xstrips) {
  extern __shared__ __attribute__((aligned(16))) float wl[];
  mh_stage_weights(wl, w, g.taps * (g.C >> 2));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int CQ = g.C >> 2;
  const long sample = (long)g.D * g.H * g.W * g.C;
  for (int item = blockIdx.x * 4 + wave; item < items; item += gridDim.x * 4) {
    const int iy = item % g.H;
    int r = item / g.H;
    const int xs = r % xstrips;
    r /= xstrips;
    const int iz = r % g.D, n = r / g.D;
    const int x0 = xs * MH_STRIP;
    const int len = min(MH_STRIP, g.W - x0);
    float* out = g_a + (long)n * sample + (((long)iz * g.H + iy) * g.W + x0) * g.C;
    for (int qb = 0; qb < CQ; qb += 64) {
      const bool on = qb + lane < CQ;
      const int q4 = on ? (qb + lane) * 4 : 0;
      float4 acc[MH_STRIP];
#pragma unroll
      for (int s = 0; s < MH_STRIP; ++s) acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int tz = 0; tz < g.KD; ++tz) {
        const int oz = iz - tz;
        if (oz < 0 || oz >= g.OD) continue;
        for (int ty = 0; ty < g.KH; ++ty) {
          const int oy = iy - ty;
          if (oy < 0 || oy >= g.OH) continue;
          const float* drow = dlogit + (((long)n * g.OD + oz) * g.OH + oy) * g.OW;
          for (int tx = 0; tx < g.KW; ++tx) {
            const float4 ww = *reinterpret_cast<const float4*>(wl + (long)((tz * g.KH + ty) * g.KW + tx) * g.C + q4);
#pragma unroll
            for (int s = 0; s < MH_STRIP; ++s) {
              const int ox = x0 + s - tx;          // wave-uniform
              if (s < len && ox >= 0 && ox < g.OW) {
                const float d = drow[ox];
                acc[s].x = fmaf(d, ww.x, acc[s].x);
                acc[s].y = fmaf(d, ww.y, acc[s].y);
                acc[s].z = fmaf(d, ww.z, acc[s].z);
                acc[s].w = fmaf(d, ww.w, acc[s].w);
              }
            }
          }
        }
      }
      if (on) {
#pragma unroll
        for (int s = 0; s < MH_STRIP; ++s)
          if (s < len) *reinterpret_cast<float4*>(out + (long)s * g.C + q4) = acc[s];
      }
    }
  }
}

// Stage 1 of the weight gradient.  Block (chunk, tap group, block of 64 channel quads): the chunk's input rows
// (n, iz, iy) are dealt to the four waves in turn; every wave walks its rows' pixels once, each activated vector
// serving the group's taps:  part[tap][c] += dlogit[n][q - tap] * a[n][q][c].  The four waves' sums are then added in
// wave order through LDS, and the block leaves ws[chunk][tap][c].
__global__ __launch_bounds__(256) void maphead_wgrad_partial_kernel(const float* __restrict__ z, Pro p, MapGeom g,
                                                                    const float* __restrict__ dlogit,
                                                                    float* __restrict__ ws, int rows, int rows_per_chunk) {
  __shared__ __attribute__((aligned(16))) float comb[MH_TAPG * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int CQ = g.C >> 2;
  const int chunk = blockIdx.x, t0 = blockIdx.y * MH_TAPG;
  const bool on = (int)blockIdx.z * 64 + lane < CQ;
  const int q4 = on ? ((int)blockIdx.z * 64 + lane) * 4 : 0;
  const float slope = pro_slope(p);
  int tz[MH_TAPG], ty[MH_TAPG], tx[MH_TAPG];
#pragma unroll
  for (int t = 0; t < MH_TAPG; ++t) {
    const int tap = min(t0 + t, g.taps - 1);
    tx[t] = tap % g.KW;
    ty[t] = (tap / g.KW) % g.KH;
    tz[t] = tap / (g.KW * g.KH);
  }
  float4 acc[MH_TAPG];
#pragma unroll
  for (int t = 0; t < MH_TAPG; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int beg = chunk * rows_per_chunk, end = min(rows, beg + rows_per_chunk);
  for (int r = beg + wave; r < end; r += 4) {
    const int iy = r % g.H;
    const int rr = r / g.H;
    const int iz = rr % g.D, n = rr / g.D;
    float sc[4] = {1.f, 1.f, 1.f, 1.f}, sh[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.scale) {
      const int si = n * p.n_stride + q4;
#pragma unroll
      for (int e = 0; e < 4; ++e) { sc[e] = p.scale[si + e]; sh[e] = p.shift[si + e]; }
    }
    // per tap: is the map row (iz - tz, iy - ty) inside, and where does it start (less tx)
    bool rowok[MH_TAPG];
    int rowbase[MH_TAPG];
#pragma unroll
    for (int t = 0; t < MH_TAPG; ++t) {
      const int oz = iz - tz[t], oy = iy - ty[t];
      rowok[t] = t0 + t < g.taps && oz >= 0 && oz < g.OD && oy >= 0 && oy < g.OH;
      rowbase[t] = ((n * g.OD + oz) * g.OH + oy) * g.OW - tx[t];
    }
    const float* row = z + (long)r * g.W * g.C + q4;
    for (int i0 = 0; i0 < g.W; i0 += MH_BATCH) {
      float4 v[MH_BATCH];
#pragma unroll
      for (int j = 0; j < MH_BATCH; ++j) {
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on && i0 + j < g.W) v[j] = *reinterpret_cast<const float4*>(row + (long)(i0 + j) * g.C);
      }
      if (p.scale) {
#pragma unroll
        for (int j = 0; j < MH_BATCH; ++j)
          if (on && i0 + j < g.W) v[j] = mh_act(v[j], sc, sh, p.act, slope);
      }
#pragma unroll
      for (int j = 0; j < MH_BATCH; ++j) {
        const int ix = i0 + j;
        if (ix < g.W) {
#pragma unroll
          for (int t = 0; t < MH_TAPG; ++t) {
            const int ox = ix - tx[t];             // wave-uniform
            if (rowok[t] && ox >= 0 && ox < g.OW) {
              const float d = dlogit[rowbase[t] + ix];
              acc[t].x = fmaf(d, v[j].x, acc[t].x);
              acc[t].y = fmaf(d, v[j].y, acc[t].y);
              acc[t].z = fmaf(d, v[j].z, acc[t].z);
              acc[t].w = fmaf(d, v[j].w, acc[t].w);
            }
          }
        }
      }
    }
  }
  for (int wv = 0; wv < 4; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int t = 0; t < MH_TAPG; ++t) {
        float4* c = reinterpret_cast<float4*>(comb + t * 256 + lane * 4);
        if (wv == 0) {
          *c = acc[t];
        } else {
          float4 o = *c;
          o.x += acc[t].x; o.y += acc[t].y; o.z += acc[t].z; o.w += acc[t].w;
          *c = o;
        }
      }
    }
    __syncthreads();
  }
  if (on) {
    for (int t = wave; t < MH_TAPG && t0 + t < g.taps; t += 4)
      *reinterpret_cast<float4*>(ws + ((long)chunk * g.taps + t0 + t) * g.C + q4) =
          *reinterpret_cast<const float4*>(comb + t * 256 + lane * 4);
  }
}

// Stage 2: dw (torch order (1, c, kd, kh, kw)) = beta*dw + sum over chunks in index order.
__global__ __launch_bounds__(256) void maphead_wgrad_final_kernel(const float* __restrict__ ws, int chunks, int taps,
                                                                  int C, float* __restrict__ dw, float beta) {
  const int i = blockIdx.x * 256 + threadIdx.x;    // tap*C + c
  if (i >= taps * C) return;
  const long stride = (long)taps * C;
  float s = 0.f;
  for (int k = 0; k < chunks; ++k) s += ws[(long)k * stride + i];
  const int tap = i / C, c = i - tap * C;
  const long o = (long)c * taps + tap;
  dw[o] = beta != 0.f ? beta * dw[o] + s : s;
}

// dbias = beta*dbias + sum dlogit: thread t adds elements t, t+256, ... in order, then block_sum4 (reduce.h).
__global__ __launch_bounds__(256) void maphead_dbias_kernel(const float* __restrict__ dlogit, int total,
                                                            float* __restrict__ dbias, float beta) {
  __shared__ float sh[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < total; i += 256) acc += dlogit[i];
  const float s = block_sum4(acc, sh);
  if (threadIdx.x == 0) {
    *dbias = beta != 0.f ? beta * (*dbias) + s : s;
  }
}

}  // namespace mpgan

using namespace mpgan;

static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Geometry checks shared by the three entry points; `what` names the caller in the error text.
static int mh_geom(const char* what, int32_t n, const int32_t* in_dhw, int32_t c, const int32_t* k_dhw, MapGeom* g) {
  MPGAN_CHECK_ARG(in_dhw && k_dhw && n > 0 && c > 0, "%s: bad argument", what);
  for (int d = 0; d < 3; ++d)
    MPGAN_CHECK_ARG(in_dhw[d] > 0 && k_dhw[d] > 0, "%s: bad argument (in_dhw / k_dhw must be positive)", what);
  MPGAN_UNSUPPORTED(c % 4 != 0, "%s: needs C %% 4 == 0 (got %d)", what, c);
  for (int d = 0; d < 3; ++d)
    MPGAN_UNSUPPORTED(in_dhw[d] < k_dhw[d], "%s: input %dx%dx%d is smaller than the kernel %dx%dx%d", what, in_dhw[0],
                      in_dhw[1], in_dhw[2], k_dhw[0], k_dhw[1], k_dhw[2]);
  const long taps = (long)k_dhw[0] * k_dhw[1] * k_dhw[2];
  MPGAN_UNSUPPORTED(taps * c * 4 > MH_LDS_BYTES, "%s: taps*C = %ld*%d floats exceed the %d-byte LDS budget of the weights",
                    what, taps, c, MH_LDS_BYTES);
  MPGAN_UNSUPPORTED((long)n * in_dhw[0] * in_dhw[1] * in_dhw[2] >= (1L << 31),
                    "%s: too many pixels for 32-bit pixel indices", what);
  g->n = n; g->D = in_dhw[0]; g->H = in_dhw[1]; g->W = in_dhw[2];
  g->KD = k_dhw[0]; g->KH = k_dhw[1]; g->KW = k_dhw[2];
  g->OD = g->D - g->KD + 1; g->OH = g->H - g->KH + 1; g->OW = g->W - g->KW + 1;
  g->C = c; g->taps = (int)taps;
  return MPGAN_OK;
}

// chunks of the weight gradient's first stage and the input rows (n, iz, iy) each takes
static void mh_chunks(const MapGeom& g, int* chunks, int* rows_per_chunk) {
  const int rows = g.n * g.D * g.H;
  const int groups = (g.taps + MH_TAPG - 1) / MH_TAPG;
  int want = 1024 / groups;                         // about four blocks of four waves per CU over all tap groups
  if (want < 64) want = 64;
  const int by4 = (rows + 3) / 4;                   // at least one row per wave
  if (want > by4) want = by4;
  *rows_per_chunk = (rows + want - 1) / want;
  *chunks = (rows + *rows_per_chunk - 1) / *rows_per_chunk;
}

static int mh_strip_grid(int items, int smem) {
  const int per_cu = smem > 40960 ? 2 : (smem > 20480 ? 4 : 8);   // 160 KiB of LDS per CU, at most 32 waves
  const int blocks = (items + 3) / 4, cap = 256 * per_cu;
  return blocks < cap ? blocks : cap;
}

extern "C" int mpgan_maphead_forward(const float* z, const mpgan_prologue* p, int32_t n, const int32_t* in_dhw,
                                     int32_t c, const int32_t* k_dhw, const float* w_perm, const float* bias,
                                     float* logit, float* prob, void* stream) {
  MPGAN_CHECK_ARG(z && w_perm && logit, "maphead_forward: bad argument");
  MapGeom g;
  if (int rc = mh_geom("maphead_forward", n, in_dhw, c, k_dhw, &g)) return rc;
  MPGAN_UNSUPPORTED(!al16(z) || !al16(w_perm), "maphead_forward: needs 16-B aligned z and w_perm");
  if (const int rc = raise_lds_limit<maphead_forward_kernel>(MH_LDS_BYTES, "maphead_forward")) return rc;
  const int xstrips = (g.OW + MH_STRIP - 1) / MH_STRIP;
  const int items = g.n * g.OD * g.OH * xstrips;
  const int smem = g.taps * g.C * 4;
  hipLaunchKernelGGL(maphead_forward_kernel, dim3(mh_strip_grid(items, smem)), dim3(256), smem, (hipStream_t)stream, z,
                     make_pro(p), g, w_perm, bias, logit, prob, items, xstrips);
  return check_launch("maphead_forward");
}

extern "C" int64_t mpgan_maphead_workspace(int32_t n, const int32_t* in_dhw, int32_t c, const int32_t* k_dhw) {
  MapGeom g;
  if (mh_geom("maphead_workspace", n, in_dhw, c, k_dhw, &g)) return -1;
  int chunks, rpc;
  mh_chunks(g, &chunks, &rpc);
  return (int64_t)chunks * g.taps * g.C * 4;
}

extern "C" int mpgan_maphead_backward(const float* z, const mpgan_prologue* p, int32_t n, const int32_t* in_dhw,
                                      int32_t c, const int32_t* k_dhw, const float* w_perm, const float* dlogit,
                                      float* g_a, float* dw, float* dbias, float beta, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
  MPGAN_CHECK_ARG(z && w_perm && dlogit, "maphead_backward: bad argument");
  MapGeom g;
  if (int rc = mh_geom("maphead_backward", n, in_dhw, c, k_dhw, &g)) return rc;
  MPGAN_UNSUPPORTED(!al16(z) || !al16(w_perm) || (g_a && !al16(g_a)) || (dw && !al16(workspace)),
                    "maphead_backward: needs 16-B aligned z, w_perm, g_a and workspace");
  int chunks = 0, rpc = 0;
  if (dw) {
    mh_chunks(g, &chunks, &rpc);
    const int64_t need = (int64_t)chunks * g.taps * g.C * 4;
    MPGAN_CHECK_ARG(workspace && workspace_bytes >= need,
                    "maphead_backward: workspace of %lld bytes is too small (mpgan_maphead_workspace: %lld)",
                    (long long)workspace_bytes, (long long)need);
  }
  hipStream_t s = (hipStream_t)stream;
  if (g_a) {
    if (const int rc = raise_lds_limit<maphead_bwd_data_kernel>(MH_LDS_BYTES, "maphead_backward")) return rc;
    const int xstrips = (g.W + MH_STRIP - 1) / MH_STRIP;
    const int items = g.n * g.D * g.H * xstrips;
    const int smem = g.taps * g.C * 4;
    hipLaunchKernelGGL(maphead_bwd_data_kernel, dim3(mh_strip_grid(items, smem)), dim3(256), smem, s, g, w_perm, dlogit,
                       g_a, items, xstrips);
  }
  if (dw) {
    const int rows = g.n * g.D * g.H;
    const int groups = (g.taps + MH_TAPG - 1) / MH_TAPG, qblocks = (g.C / 4 + 63) / 64;
    hipLaunchKernelGGL(maphead_wgrad_partial_kernel, dim3(chunks, groups, qblocks), dim3(256), 0, s, z, make_pro(p), g,
                       dlogit, static_cast<float*>(workspace), rows, rpc);
    hipLaunchKernelGGL(maphead_wgrad_final_kernel, dim3((g.taps * g.C + 255) / 256), dim3(256), 0, s,
                       static_cast<const float*>(workspace), chunks, g.taps, g.C, dw, beta);
  }
  if (dbias)
    hipLaunchKernelGGL(maphead_dbias_kernel, dim3(1), dim3(256), 0, s, dlogit, g.n * g.OD * g.OH * g.OW, dbias, beta);
  return check_launch("maphead_backward");
}
