// Foreground masks (include/mpgan_hip.h: "foreground masks" states every definition):
//
//   fg_hist_kernel            an item's histogram: a block counts its chunk into 256 LDS counters (image_stats.h: the
//                             joint histogram's bin rule and wave peel) and flushes the non-zero ones with 64-bit
//                             integer atomics.
//   fg_otsu_kernel            Otsu's method over an item's <= 256 counts, one block, in the order the header states.
//   fg_mask_kernel            mask / count / raw box extremes in one pass: per-thread minima and maxima, folded over
//                             the wave and the block, one integer atomic per block, axis and direction.
//   fg_box_init / fg_box_final  the launches around it that initialise box and count and apply margin and clipping.
//   fg_l1_forward_kernel      block partials of num and of the foreground count (fp64, block_tree_sum).
//   fg_l1_item_kernel         an item's partials in slot order + the same tree; den and loss_item.
//   launch_loss_reduce        the reduction over the items (loss_ops.hip).
//   fg_l1_backward_kernel     da and/or db, one factor per item and weight.
//   fg_err_kernel / fg_err_final_kernel   masked MAE / MSE / PSNR / count.
//
// fg_chunks (image_stats.h's planner with this file's constants) is the ONE place the grid of every stream is decided,
// fg_load4 / fg_mask4 the one place a group of four values is read: a thread's values and their order do not depend on
// the pointers' alignment.
#include <limits.h>
#include "image_stats.h"

namespace mpgan {

constexpr long FG_CHUNK_MIN = 4096;             // values a block walks at least: four groups per thread
constexpr int FG_TARGET_BLOCKS = 2048;          // eight 4-wave blocks per CU
constexpr int FG_PEEL_ROUNDS = 2;

static StreamChunks fg_chunks(long n, long items) { return stream_chunks(n, items, FG_CHUNK_MIN, FG_TARGET_BLOCKS); }

// The block's chunk of an item: first value c0, len values (0 when the rounding of per_chunk left none).
struct FgSpan {
  long item, c0, len;
};

__device__ __forceinline__ FgSpan fg_span(long n, long chunks, long per_chunk) {
  FgSpan s;
  s.item = blockIdx.x / chunks;
  s.c0 = (blockIdx.x % chunks) * per_chunk;
  const long rest = n - s.c0;
  s.len = rest < 0 ? 0 : (rest < per_chunk ? rest : per_chunk);
  return s;
}

__device__ __forceinline__ bool fg_aligned(const void* p, unsigned bytes) {
  return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0;
}

// Values e .. e + 3 of the chunk at p (the values past len are 0); returns how many are real.
__device__ __forceinline__ int fg_load4(const float* __restrict__ p, long e, long len, bool vec, float (&v)[4]) {
  const int cnt = len - e < 4 ? (int)(len - e) : 4;
  if (vec && cnt == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p + e);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < cnt ? p[e + k] : 0.f;
  }
  return cnt;
}

__device__ __forceinline__ void fg_mask4(const uint8_t* __restrict__ p, long e, int cnt, bool vec, bool (&m)[4]) {
  if (vec && cnt == 4) {
    const uint32_t q = *reinterpret_cast<const uint32_t*>(p + e);
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = ((q >> (8 * k)) & 0xffu) != 0u;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = k < cnt ? p[e + k] != 0 : false;
  }
}

__device__ __forceinline__ void fg_store4(float* __restrict__ p, long e, int cnt, bool vec, const float (&v)[4]) {
  if (vec && cnt == 4) {
    *reinterpret_cast<float4*>(p + e) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < cnt) p[e + k] = v[k];
  }
}

// ---- Otsu ----------------------------------------------------------------------------------------------------------
struct FgHist {
  const float* x;
  long n, chunks, per_chunk;
  float lo, hi, s;
  int bins;
  unsigned long long* hist;                     // [items][bins]
};

__global__ __launch_bounds__(256) void fg_hist_kernel(FgHist p) {
  __shared__ unsigned lh[256];
  const int tid = threadIdx.x;
  lh[tid] = 0u;
  __syncthreads();
  const FgSpan sp = fg_span(p.n, p.chunks, p.per_chunk);
  const float* x = p.x + sp.item * p.n + sp.c0;
  const bool vec = fg_aligned(x, 16);
  // block-uniform trip count: hist_submit needs every lane of a wave
  for (long g0 = 0; 4 * g0 < sp.len; g0 += 256) {
    const long e = 4 * (g0 + tid);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    const int cnt = e < sp.len ? fg_load4(x, e, sp.len, vec, v) : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = k < cnt && v[k] >= p.lo && v[k] <= p.hi;   // NaN fails both comparisons
      const int j = ok ? hist_bin(v[k], p.lo, p.s, p.bins) : 0;
      hist_submit<FG_PEEL_ROUNDS>(lh, ok, (unsigned)j);
    }
  }
  __syncthreads();
  if (tid < p.bins && lh[tid]) atomicAdd(&p.hist[sp.item * p.bins + tid], (unsigned long long)lh[tid]);
}

// The centres, the products n_j c_j and var_k take one thread per bin (the divisions of fp64 are the cost); the two
// running sums in between are one thread's, in the header's order.  Every var_k has the bits a serial walk would give.
__global__ __launch_bounds__(256) void fg_otsu_kernel(const unsigned long long* __restrict__ hist, int bins, double lo,
                                                      double hi, float* __restrict__ thr) {
#pragma clang fp contract(off)
  __shared__ unsigned long long n[256], w0s[256];
  __shared__ double prod[256], pre[256], var[256];
  __shared__ double suf[257];                   // suf[j] = sum_{i >= j} n_i c_i, added from the top down
  __shared__ unsigned long long total_s;
  __shared__ int occupied_s, last_s;
  const int tid = threadIdx.x;
  const double span = hi - lo, db = (double)bins;
  if (tid < bins) {
    n[tid] = hist[(long)blockIdx.x * bins + tid];
    prod[tid] = (double)n[tid] * (lo + ((double)tid + 0.5) * span / db);
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long w = 0ull;
    int occupied = 0, last = 0;
    double s = 0.0;
    for (int j = 0; j < bins; ++j) {
      w += n[j];
      s += prod[j];
      w0s[j] = w;
      pre[j] = s;
      if (n[j]) { ++occupied; last = j; }
    }
    s = 0.0;
    suf[bins] = 0.0;
    for (int j = bins - 1; j >= 1; --j) {
      s += prod[j];
      suf[j] = s;
    }
    total_s = w; occupied_s = occupied; last_s = last;
  }
  __syncthreads();
  if (tid < bins - 1) {
    const unsigned long long w0 = w0s[tid], w1 = total_s - w0;
    double v = 0.0;
    if (w0 != 0ull && w1 != 0ull) {
      const double d = pre[tid] / (double)w0 - suf[tid + 1] / (double)w1;
      v = ((double)w0 * (double)w1) * (d * d);
    }
    var[tid] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  int k = last_s;                               // one occupied bin: its own centre
  if (occupied_s > 1) {
    double best = -1.0;
    for (int j = 0; j < bins - 1; ++j)
      if (var[j] > best) { best = var[j]; k = j; }     // strictly greater: the first maximum
  }
  thr[blockIdx.x] = total_s == 0ull ? __int_as_float(0x7fc00000) : (float)(lo + ((double)k + 0.5) * span / db);
}

// ---- mask, count, box ------------------------------------------------------------------------------------------------
struct FgMask {
  const float* x;
  const float* thr;
  long n, chunks, per_chunk;
  int D, H, W;
  FastDiv div_w, div_h;                         // n < 2^32: the 32-bit coordinate split
  int narrow;
  uint8_t* mask;
  int* box;                                     // [items][2][3]: raw minima and maxima until fg_box_final
  unsigned long long* count;
};

__global__ void fg_box_init(int* box, unsigned long long* count, int items) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= items) return;
  if (count) count[i] = 0ull;
  if (box) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { box[6 * i + d] = INT_MAX; box[6 * i + 3 + d] = -1; }
  }
}

__global__ void fg_box_final(int* box, int items, int D, int H, int W, int mz, int my, int mx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= items) return;
  const int ext[3] = {D, H, W}, mg[3] = {mz, my, mx};
  const bool empty = box[6 * i + 3] < 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const long lo = (long)box[6 * i + d] - mg[d], hi = (long)box[6 * i + 3 + d] + 1 + mg[d];
    box[6 * i + d] = empty ? 0 : (int)(lo > 0 ? lo : 0);
    box[6 * i + 3 + d] = empty ? 0 : (int)(hi < ext[d] ? hi : ext[d]);
  }
}

template <bool BOX>
__global__ __launch_bounds__(256) void fg_mask_kernel(FgMask p) {
  __shared__ int smin[3][4], smax[3][4];
  __shared__ unsigned scnt[4];
  const int tid = threadIdx.x;
  const FgSpan sp = fg_span(p.n, p.chunks, p.per_chunk);
  const float* x = p.x + sp.item * p.n + sp.c0;
  uint8_t* mk = p.mask ? p.mask + sp.item * p.n + sp.c0 : nullptr;
  const bool vec = fg_aligned(x, 16), mvec = mk && fg_aligned(mk, 4);
  const float t = p.thr[sp.item];
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {-1, -1, -1};
  unsigned cnt_fg = 0;
  for (long e = 4L * tid; e < sp.len; e += 1024) {
    float v[4];
    const int cnt = fg_load4(x, e, sp.len, vec, v);
    bool m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = k < cnt && v[k] > t;          // false for a NaN on either side
    if (mk) {
      if (mvec && cnt == 4) {
        *reinterpret_cast<uint32_t*>(mk + e) = (unsigned)m[0] | ((unsigned)m[1] << 8) | ((unsigned)m[2] << 16) |
                                               ((unsigned)m[3] << 24);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (k < cnt) mk[e + k] = (uint8_t)m[k];
      }
    }
    const int any = (int)m[0] + (int)m[1] + (int)m[2] + (int)m[3];
    cnt_fg += (unsigned)any;
    if (BOX && any) {
      // (z, y, x) of the group's first voxel, then a carry per step
      const long idx = sp.c0 + e;
      int cz, cy, cx;
      if (p.narrow) {
        const unsigned row = fdiv((unsigned)idx, p.div_w);
        cx = (int)((unsigned)idx - row * (unsigned)p.W);
        const unsigned z = fdiv(row, p.div_h);
        cy = (int)(row - z * (unsigned)p.H);
        cz = (int)z;
      } else {
        const long row = idx / p.W;
        cx = (int)(idx - row * p.W);
        cz = (int)(row / p.H);
        cy = (int)(row - (long)cz * p.H);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (m[k]) {
          lo[0] = min(lo[0], cz); hi[0] = max(hi[0], cz);
          lo[1] = min(lo[1], cy); hi[1] = max(hi[1], cy);
          lo[2] = min(lo[2], cx); hi[2] = max(hi[2], cx);
        }
        if (++cx == p.W) {
          cx = 0;
          if (++cy == p.H) { cy = 0; ++cz; }
        }
      }
    }
  }
  // the wave, then the block; integer minima, maxima and sums: no order to fix
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    cnt_fg += __shfl_xor(cnt_fg, off, 64);
    if (BOX) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        lo[d] = min(lo[d], __shfl_xor(lo[d], off, 64));
        hi[d] = max(hi[d], __shfl_xor(hi[d], off, 64));
      }
    }
  }
  const int lane = tid & 63, w = tid >> 6;
  if (lane == 0) {
    scnt[w] = cnt_fg;
    if (BOX) {
#pragma unroll
      for (int d = 0; d < 3; ++d) { smin[d][w] = lo[d]; smax[d][w] = hi[d]; }
    }
  }
  __syncthreads();
  if (tid == 0) {
    const unsigned long long c = (unsigned long long)scnt[0] + scnt[1] + scnt[2] + scnt[3];
    if (c != 0ull) {
      if (p.count) atomicAdd(&p.count[sp.item], c);
      if (BOX) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          atomicMin(&p.box[6 * sp.item + d], min(min(smin[d][0], smin[d][1]), min(smin[d][2], smin[d][3])));
          atomicMax(&p.box[6 * sp.item + 3 + d], max(max(smax[d][0], smax[d][1]), max(smax[d][2], smax[d][3])));
        }
      }
    }
  }
}

// ---- mask-weighted L1 ------------------------------------------------------------------------------------------------
struct FgL1 {
  const float* a;
  const float* b;
  const uint8_t* mask;                          // one of mask, thr
  const float* thr;
  long n, chunks, per_chunk;
  double w_fg, w_bg;
  double* partials;                             // forward: num[items][chunks] | n_fg[items][chunks]
  const double* den;                            // backward
  const float* upstream;
  int up_stride, channels;
  double scale;
  float* da;
  float* db;
};

template <bool EXPLICIT>
__global__ __launch_bounds__(256) void fg_l1_forward_kernel(FgL1 p) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const FgSpan sp = fg_span(p.n, p.chunks, p.per_chunk);
  const long base = sp.item * p.n + sp.c0;
  const float* a = p.a + base;
  const float* b = p.b + base;
  const uint8_t* mk = EXPLICIT ? p.mask + base : nullptr;
  const bool veca = fg_aligned(a, 16), vecb = fg_aligned(b, 16), vecm = EXPLICIT && fg_aligned(mk, 4);
  const float t = EXPLICIT ? 0.f : p.thr[sp.item];
  double num = 0.0;
  unsigned nfg = 0;
  for (long e = 4L * tid; e < sp.len; e += 1024) {
    float va[4], vb[4];
    const int cnt = fg_load4(a, e, sp.len, veca, va);
    fg_load4(b, e, sp.len, vecb, vb);
    bool m[4];
    if (EXPLICIT) {
      fg_mask4(mk, e, cnt, vecm, m);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = k < cnt && vb[k] > t;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < cnt) {
        const double d = fabs((double)va[k] - (double)vb[k]);
        num += (m[k] ? p.w_fg : p.w_bg) * d;
        nfg += (unsigned)m[k];
      }
    }
  }
  num = block_tree_sum<256>(num, red);
  const double cnt_fg = block_tree_sum<256, true>((double)nfg, red);   // integers below 2^53: exact in any order
  if (tid == 0) {
    p.partials[blockIdx.x] = num;
    p.partials[(long)gridDim.x + blockIdx.x] = cnt_fg;          // the grid is items x chunks
  }
}

// item[i] = loss_item, den[i] = den_item
__global__ __launch_bounds__(256) void fg_l1_item_kernel(const double* __restrict__ partials, long chunks, long items,
                                                         long n, double w_fg, double w_bg, double* __restrict__ item,
                                                         double* __restrict__ den) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const double* pn = partials + (long)blockIdx.x * chunks;
  const double* pc = partials + items * chunks + (long)blockIdx.x * chunks;
  double s = 0.0, c = 0.0;
  for (long i = threadIdx.x; i < chunks; i += 256) { s += pn[i]; c += pc[i]; }
  s = block_tree_sum<256>(s, red);
  c = block_tree_sum<256, true>(c, red);
  if (threadIdx.x == 0) {
    const double d = w_fg * c + w_bg * ((double)n - c);
    den[blockIdx.x] = d;
    item[blockIdx.x] = d > 0.0 ? s / d : 0.0;
  }
}

template <bool EXPLICIT>
__global__ __launch_bounds__(256) void fg_l1_backward_kernel(FgL1 p) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const FgSpan sp = fg_span(p.n, p.chunks, p.per_chunk);
  const long base = sp.item * p.n + sp.c0;
  const float* a = p.a + base;
  const float* b = p.b + base;
  const uint8_t* mk = EXPLICIT ? p.mask + base : nullptr;
  float* da = p.da ? p.da + base : nullptr;
  float* db = p.db ? p.db + base : nullptr;
  const bool veca = fg_aligned(a, 16), vecb = fg_aligned(b, 16), vecm = EXPLICIT && fg_aligned(mk, 4);
  const bool vda = da && fg_aligned(da, 16), vdb = db && fg_aligned(db, 16);
  const float t = EXPLICIT ? 0.f : p.thr[sp.item];
  const double den = p.den[sp.item];
  float c_fg = 0.f, c_bg = 0.f;
  if (den > 0.0) {
    const double up = (double)p.upstream[(sp.item / p.channels) * p.up_stride] * p.scale;
    c_fg = (float)(up * p.w_fg / den);
    c_bg = (float)(up * p.w_bg / den);
  }
  for (long e = 4L * tid; e < sp.len; e += 1024) {
    float va[4], vb[4], ga[4], gb[4];
    const int cnt = fg_load4(a, e, sp.len, veca, va);
    fg_load4(b, e, sp.len, vecb, vb);
    bool m[4];
    if (EXPLICIT) {
      fg_mask4(mk, e, cnt, vecm, m);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = k < cnt && vb[k] > t;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float c = m[k] ? c_fg : c_bg;
      ga[k] = (va[k] > vb[k] ? c : (va[k] < vb[k] ? -c : 0.f)) + 0.f;   // + 0: a weight of 0 leaves +0, never -0
      gb[k] = -ga[k];                                                   // the negation itself: db == -da in every bit
    }
    if (da) fg_store4(da, e, cnt, vda, ga);
    if (db) fg_store4(db, e, cnt, vdb, gb);
  }
}

// ---- masked errors ---------------------------------------------------------------------------------------------------
// partials[3][chunks]: sum |a - b|, sum (a - b)^2, count
__global__ __launch_bounds__(256) void fg_err_kernel(const float* __restrict__ a0, const float* __restrict__ b0,
                                                     const uint8_t* __restrict__ m0, long n, long chunks,
                                                     long per_chunk, double* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const FgSpan sp = fg_span(n, chunks, per_chunk);
  const float* a = a0 + sp.c0;
  const float* b = b0 + sp.c0;
  const uint8_t* mk = m0 + sp.c0;
  const bool veca = fg_aligned(a, 16), vecb = fg_aligned(b, 16), vecm = fg_aligned(mk, 4);
  double ae = 0.0, se = 0.0;
  unsigned cnt_m = 0;
  for (long e = 4L * tid; e < sp.len; e += 1024) {
    float va[4], vb[4];
    const int cnt = fg_load4(a, e, sp.len, veca, va);
    fg_load4(b, e, sp.len, vecb, vb);
    bool m[4];
    fg_mask4(mk, e, cnt, vecm, m);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (m[k]) {
        const double d = (double)va[k] - (double)vb[k];
        ae += fabs(d);
        se += d * d;
        ++cnt_m;
      }
    }
  }
  ae = block_tree_sum<256>(ae, red);
  se = block_tree_sum<256, true>(se, red);
  const double c = block_tree_sum<256, true>((double)cnt_m, red);
  if (tid == 0) {
    partials[blockIdx.x] = ae;
    partials[chunks + blockIdx.x] = se;
    partials[2 * chunks + blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(256) void fg_err_final_kernel(const double* __restrict__ partials, long chunks,
                                                           double data_range, double* __restrict__ out4) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  double ae = 0.0, se = 0.0, c = 0.0;
  for (long i = threadIdx.x; i < chunks; i += 256) {
    ae += partials[i];
    se += partials[chunks + i];
    c += partials[2 * chunks + i];
  }
  ae = block_tree_sum<256>(ae, red);
  se = block_tree_sum<256, true>(se, red);
  c = block_tree_sum<256, true>(c, red);
  if (threadIdx.x == 0) {
    if (c == 0.0) {
      const double qnan = __longlong_as_double(0x7ff8000000000000LL);
      out4[0] = out4[1] = out4[2] = qnan;
    } else {
      const double mse = se / c;
      out4[0] = ae / c;
      out4[1] = mse;
      out4[2] = mse > 0.0 ? 10.0 * log10(data_range * data_range / mse) : (double)INFINITY;
    }
    out4[3] = c;
  }
}

// The checks the two masked-L1 entry points share.  Status as the entry points return it.
static int fg_l1_args(const char* who, const float* a, const float* b, int64_t n, int32_t items, int32_t channels,
                      const uint8_t* mask, const float* thr, double w_fg, double w_bg, StreamChunks* c) {
  MPGAN_CHECK_ARG(a && b, "%s: null input", who);
  MPGAN_CHECK_ARG(items >= 1, "%s: items %d < 1", who, items);
  MPGAN_CHECK_ARG(n >= 1, "%s: numel_per_item %ld < 1", who, (long)n);
  if (int rc = check_items(who, items, channels)) return rc;
  MPGAN_CHECK_ARG((mask != nullptr) != (thr != nullptr), "%s: exactly one of mask and thr must be given (got %s)", who,
                  mask ? "both" : "neither");
  MPGAN_CHECK_ARG(is_finite(w_fg) && is_finite(w_bg) && w_fg >= 0.0 && w_bg >= 0.0,
                  "%s: weights must be finite and >= 0", who);
  *c = fg_chunks(n, items);
  MPGAN_CHECK_ARG(c->chunks * (long)items < (1L << 31), "%s: too many blocks", who);
  return MPGAN_OK;
}

}  // namespace mpgan

using namespace mpgan;

extern "C" int64_t mpgan_otsu_workspace(int32_t items, int32_t bins) {
  if (items < 1 || bins < 2 || bins > 256) return -1;
  return (int64_t)items * bins * (int64_t)sizeof(int64_t);
}

extern "C" int mpgan_otsu_threshold(const float* x, int64_t numel_per_item, int32_t items, float lo, float hi,
                                    int32_t bins, void* workspace, float* thr, void* stream) {
  MPGAN_CHECK_ARG(x && workspace && thr, "otsu_threshold: null pointer");
  MPGAN_CHECK_ARG(bins >= 2 && bins <= 256, "otsu_threshold: bins %d outside [2, 256]", bins);
  MPGAN_CHECK_ARG(items >= 1, "otsu_threshold: items %d < 1", items);
  MPGAN_CHECK_ARG(numel_per_item >= 1, "otsu_threshold: numel_per_item %ld < 1", (long)numel_per_item);
  float s;
  if (int rc = check_bin_range("otsu_threshold", lo, hi, bins, &s)) return rc;
  MPGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "otsu_threshold: workspace must be 8-byte aligned");
  const StreamChunks c = fg_chunks(numel_per_item, items);
  MPGAN_CHECK_ARG(c.chunks * (long)items < (1L << 31), "otsu_threshold: too many blocks");
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(workspace, 0, (size_t)mpgan_otsu_workspace(items, bins), st);
  if (e != hipSuccess) { set_error("otsu_threshold: hipMemsetAsync: %s", hipGetErrorString(e)); return MPGAN_ERR_HIP; }
  FgHist p;
  p.x = x; p.n = numel_per_item; p.chunks = c.chunks; p.per_chunk = c.per_chunk;
  p.lo = lo; p.hi = hi; p.s = s; p.bins = bins;
  p.hist = static_cast<unsigned long long*>(workspace);
  hipLaunchKernelGGL(fg_hist_kernel, dim3((unsigned)(c.chunks * items)), dim3(256), 0, st, p);
  hipLaunchKernelGGL(fg_otsu_kernel, dim3((unsigned)items), dim3(256), 0, st, (const unsigned long long*)p.hist,
                     (int)bins, (double)lo, (double)hi, thr);
  return check_launch("otsu_threshold");
}

extern "C" int mpgan_foreground_mask(const float* x, const int32_t* dhw, int32_t items, const float* thr,
                                     const int32_t* margin, uint8_t* mask, int32_t* box, int64_t* count, void* stream) {
  MPGAN_CHECK_ARG(x && dhw && thr, "foreground_mask: null pointer");
  MPGAN_CHECK_ARG(mask || box || count, "foreground_mask: no output asked for");
  MPGAN_CHECK_ARG(items >= 1, "foreground_mask: items %d < 1", items);
  MPGAN_CHECK_ARG(dhw[0] >= 1 && dhw[1] >= 1 && dhw[2] >= 1, "foreground_mask: empty extents (%d, %d, %d)", dhw[0],
                  dhw[1], dhw[2]);
  int mg[3] = {0, 0, 0};
  if (margin)
    for (int d = 0; d < 3; ++d) {
      MPGAN_CHECK_ARG(margin[d] >= 0, "foreground_mask: negative margin %d on axis %d", margin[d], d);
      mg[d] = margin[d];
    }
  const long n = (long)dhw[0] * dhw[1] * dhw[2];
  const StreamChunks c = fg_chunks(n, items);
  MPGAN_CHECK_ARG(c.chunks * (long)items < (1L << 31), "foreground_mask: too many blocks");
  FgMask p;
  p.x = x; p.thr = thr; p.n = n; p.chunks = c.chunks; p.per_chunk = c.per_chunk;
  p.D = dhw[0]; p.H = dhw[1]; p.W = dhw[2];
  p.narrow = n < (1L << 32);
  p.div_w = make_fastdiv((unsigned)dhw[2]); p.div_h = make_fastdiv((unsigned)dhw[1]);
  p.mask = mask; p.box = box; p.count = reinterpret_cast<unsigned long long*>(count);
  hipStream_t st = (hipStream_t)stream;
  const dim3 small((unsigned)((items + 255) / 256));
  if (box || count) hipLaunchKernelGGL(fg_box_init, small, dim3(256), 0, st, p.box, p.count, (int)items);
  const dim3 grid((unsigned)(c.chunks * items));
  if (box) {
    hipLaunchKernelGGL(fg_mask_kernel<true>, grid, dim3(256), 0, st, p);
    hipLaunchKernelGGL(fg_box_final, small, dim3(256), 0, st, p.box, (int)items, p.D, p.H, p.W, mg[0], mg[1], mg[2]);
  } else {
    hipLaunchKernelGGL(fg_mask_kernel<false>, grid, dim3(256), 0, st, p);
  }
  return check_launch("foreground_mask");
}

extern "C" int64_t mpgan_masked_l1_workspace(int64_t numel_per_item, int32_t items) {
  if (numel_per_item < 1 || items < 1) return -1;
  const StreamChunks c = fg_chunks(numel_per_item, items);
  return (2 * c.chunks * (int64_t)items + items) * (int64_t)sizeof(double);
}

extern "C" int mpgan_masked_l1_forward(const float* a, const float* b, int64_t numel_per_item, int32_t items,
                                       int32_t channels, const uint8_t* mask, const float* thr, double w_fg,
                                       double w_bg, void* workspace, int64_t workspace_bytes, double* den,
                                       int32_t reduction, float* loss, void* stream) {
  StreamChunks c;
  if (int rc = fg_l1_args("masked_l1_forward", a, b, numel_per_item, items, channels, mask, thr, w_fg, w_bg, &c))
    return rc;
  MPGAN_CHECK_ARG(den && loss, "masked_l1_forward: null pointer");
  if (int rc = check_reduction("masked_l1_forward", reduction)) return rc;
  if (int rc = check_workspace("masked_l1_forward", workspace, workspace_bytes,
                               mpgan_masked_l1_workspace(numel_per_item, items)))
    return rc;
  MPGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(den) & 7) == 0, "masked_l1_forward: den must be 8-byte aligned");
  FgL1 p;
  p.a = a; p.b = b; p.mask = mask; p.thr = thr;
  p.n = numel_per_item; p.chunks = c.chunks; p.per_chunk = c.per_chunk;
  p.w_fg = w_fg; p.w_bg = w_bg;
  p.partials = static_cast<double*>(workspace);
  p.den = nullptr; p.upstream = nullptr; p.up_stride = 0; p.channels = channels; p.scale = 0.0;
  p.da = nullptr; p.db = nullptr;
  double* item = p.partials + 2 * c.chunks * (long)items;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(c.chunks * items));
  if (mask) {
    hipLaunchKernelGGL(fg_l1_forward_kernel<true>, grid, dim3(256), 0, st, p);
  } else {
    hipLaunchKernelGGL(fg_l1_forward_kernel<false>, grid, dim3(256), 0, st, p);
  }
  hipLaunchKernelGGL(fg_l1_item_kernel, dim3((unsigned)items), dim3(256), 0, st, (const double*)p.partials, c.chunks,
                     (long)items, (long)numel_per_item, w_fg, w_bg, item, den);
  launch_loss_reduce(item, items, channels, reduction, false, loss, st);
  return check_launch("masked_l1_forward");
}

extern "C" int mpgan_masked_l1_backward(const float* a, const float* b, int64_t numel_per_item, int32_t items,
                                        int32_t channels, const uint8_t* mask, const float* thr, double w_fg,
                                        double w_bg, const double* den, const float* upstream,
                                        int32_t upstream_stride, double scale, float* da, float* db, void* stream) {
  StreamChunks c;
  if (int rc = fg_l1_args("masked_l1_backward", a, b, numel_per_item, items, channels, mask, thr, w_fg, w_bg, &c))
    return rc;
  MPGAN_CHECK_ARG(den && upstream, "masked_l1_backward: null pointer");
  MPGAN_CHECK_ARG(da || db, "masked_l1_backward: no gradient asked for");
  if (int rc = check_upstream_stride("masked_l1_backward", upstream_stride)) return rc;
  if (int rc = check_scale("masked_l1_backward", scale)) return rc;
  FgL1 p;
  p.a = a; p.b = b; p.mask = mask; p.thr = thr;
  p.n = numel_per_item; p.chunks = c.chunks; p.per_chunk = c.per_chunk;
  p.w_fg = w_fg; p.w_bg = w_bg;
  p.partials = nullptr; p.den = den; p.upstream = upstream; p.up_stride = upstream_stride; p.channels = channels;
  p.scale = scale; p.da = da; p.db = db;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(c.chunks * items));
  if (mask) {
    hipLaunchKernelGGL(fg_l1_backward_kernel<true>, grid, dim3(256), 0, st, p);
  } else {
    hipLaunchKernelGGL(fg_l1_backward_kernel<false>, grid, dim3(256), 0, st, p);
  }
  return check_launch("masked_l1_backward");
}

extern "C" int64_t mpgan_masked_errors_partials(int64_t numel) {
  if (numel < 1) return -1;
  return 3 * fg_chunks(numel, 1).chunks;
}

extern "C" int mpgan_masked_image_errors(const float* a, const float* b, const uint8_t* mask, int64_t numel,
                                         float data_range, double* partials, double* out4, void* stream) {
  MPGAN_CHECK_ARG(a && b && mask && partials && out4, "masked_image_errors: null pointer");
  MPGAN_CHECK_ARG(numel >= 1, "masked_image_errors: numel %ld < 1", (long)numel);
  MPGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(partials) & 7) == 0 && (reinterpret_cast<uintptr_t>(out4) & 7) == 0,
                  "masked_image_errors: partials and out4 must be 8-byte aligned");
  const StreamChunks c = fg_chunks(numel, 1);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(fg_err_kernel, dim3((unsigned)c.chunks), dim3(256), 0, st, a, b, mask, (long)numel, c.chunks,
                     c.per_chunk, partials);
  hipLaunchKernelGGL(fg_err_final_kernel, dim3(1), dim3(256), 0, st, (const double*)partials, c.chunks,
                     (double)data_range, out4);
  return check_launch("masked_image_errors");
}
