// Sliding-window inference around a predictor (MONAI 0.4.0 sliding_window_inference, the call that
// code/GAN/minipig_inference.py:110-114 holds commented out): window gather with on-the-fly constant padding,
// the count map, the importance-weighted blend and the final division.  The predictor does the arithmetic;
// these kernels move bytes.  Every thread owns the elements it writes and visits windows in global order, so the
// result is bit-identical to MONAI's sequential `out[win] += imp * pred; count[win] += imp` with no float
// atomics.  One rounded product and one rounded add per window: contraction into an FMA is switched off below
// (HIP's __fmul_rn / __fadd_rn are plain operators in a system header compiled with contraction on, so the
// helpers here are this file's own).
#include "mpgan_common.h"

#pragma clang fp contract(off)

namespace mpgan {

// Device view of mpgan_sw_geom (the start table stays in device memory: GatherConv-style by-value tables are
// bounded by the 4 KiB kernel-argument limit, the number of windows is not).
struct SwGeom {
  const int32_t* starts;  // z starts, then y, then x
  int D, H, W;
  int pz, py, px;
  int Dp, Hp, Wp;
  int rz, ry, rx;
  int nz, ny, nx;
  int nwin;
};

__device__ __forceinline__ void sw_window(const SwGeom& g, int gi, int& b, int& sz, int& sy, int& sx) {
  b = gi / g.nwin;
  const int w = gi - b * g.nwin;
  const int t = w / g.nx;
  const int ix = w - t * g.nx;
  const int iz = t / g.ny;
  const int iy = t - iz * g.ny;
  sz = g.starts[iz];
  sy = g.starts[g.nz + iy];
  sx = g.starts[g.nz + g.ny + ix];
}

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// One thread per 4 consecutive x of a window row.  grid: (ceil(quads / 256), cin, n).  VEC: rx % 4 == 0 (16-byte
// stores); ALIGNED_IN: the input base is 16-byte aligned (16-byte loads where the row offset allows).
template <bool VEC, bool ALIGNED_IN>
__global__ __launch_bounds__(256) void sw_gather_kernel(const float* __restrict__ in, SwGeom g, int cin, int first,
                                                        float cval, FastDiv fq, FastDiv fy, unsigned quads,
                                                        float* __restrict__ win) {
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  if (q >= quads) return;
  const int c = blockIdx.y, k = blockIdx.z;
  int b, sz, sy, sx;
  sw_window(g, first + k, b, sz, sy, sx);
  unsigned row, xq, z, y;
  fdivmod(q, fq, row, xq);
  fdivmod(row, fy, z, y);
  const int x0 = (int)xq * 4;
  const long long rvol = (long long)g.rz * g.ry * g.rx;
  float* dst = win + ((long long)k * cin + c) * rvol + ((long long)z * g.ry + y) * g.rx + x0;
  const int iz = sz + (int)z - g.pz, iy = sy + (int)y - g.py, ix = sx + x0 - g.px;
  const bool row_ok = (unsigned)iz < (unsigned)g.D && (unsigned)iy < (unsigned)g.H;
  const long long off = row_ok ? ((((long long)b * cin + c) * g.D + iz) * g.H + iy) * g.W + ix : 0;
  float v[4];
  if (ALIGNED_IN && row_ok && ix >= 0 && ix + 4 <= g.W && (off & 3) == 0) {
    const float4 t = ld4(in + off);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (row_ok && (unsigned)(ix + j) < (unsigned)g.W) ? in[off + j] : cval;
  }
  if (VEC) {
    st4(dst, make_float4(v[0], v[1], v[2], v[3]));
  } else {
    const int cnt = min(4, g.rx - x0);
    for (int j = 0; j < cnt; ++j) dst[j] = v[j];
  }
}

// Sum of imp over the windows of one image that cover a padded voxel, in window order (z, then y, then x start:
// the nested loops visit the covering windows lexicographically, which is the global order).  VEC: rx, Wp and every
// x start are multiples of 4, so a quad lies wholly inside or wholly outside each window.
template <bool VEC, bool CONST_IMP>
__global__ __launch_bounds__(256) void sw_count_kernel(SwGeom g, const float* __restrict__ imp, FastDiv fq,
                                                       FastDiv fy, unsigned units, float* __restrict__ count) {
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  if (q >= units) return;
  unsigned row, xq, z, y;
  fdivmod(q, fq, row, xq);
  fdivmod(row, fy, z, y);
  const int x = VEC ? (int)xq * 4 : (int)xq;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  const int* sy_t = g.starts + g.nz;
  const int* sx_t = g.starts + g.nz + g.ny;
  for (int iz = 0; iz < g.nz; ++iz) {
    const int dz = (int)z - g.starts[iz];
    if ((unsigned)dz >= (unsigned)g.rz) continue;
    for (int iy = 0; iy < g.ny; ++iy) {
      const int dy = (int)y - sy_t[iy];
      if ((unsigned)dy >= (unsigned)g.ry) continue;
      for (int ix = 0; ix < g.nx; ++ix) {
        const int dx = x - sx_t[ix];
        if ((unsigned)dx >= (unsigned)g.rx) continue;
        const long long l = ((long long)dz * g.ry + dy) * g.rx + dx;
        if (VEC) {
          const float4 t = CONST_IMP ? make_float4(1.f, 1.f, 1.f, 1.f) : ld4(imp + l);
          a[0] = add_rn(a[0], t.x); a[1] = add_rn(a[1], t.y);
          a[2] = add_rn(a[2], t.z); a[3] = add_rn(a[3], t.w);
        } else {
          a[0] = add_rn(a[0], CONST_IMP ? 1.f : imp[l]);
        }
      }
    }
  }
  const long long o = ((long long)z * g.Hp + y) * g.Wp + x;
  if (VEC) st4(count + o, make_float4(a[0], a[1], a[2], a[3]));
  else count[o] = a[0];
}

// Blend of one predictor call.  A thread owns one voxel (VEC: 4 consecutive x) of acc[b][c] inside the call's
// bounding box, reads it once, adds imp * pred of each of the call's windows that covers it in order, and writes
// it once when any did.  grid: (ceil(box units / 256), cout, images spanned by the call).
template <bool VEC, bool CONST_IMP>
__global__ __launch_bounds__(256) void sw_blend_kernel(SwGeom g, const float* __restrict__ pred, int cout, int first,
                                                       int n, const float* __restrict__ imp, int b0, int bz0, int by0,
                                                       int bx0, FastDiv fq, FastDiv fy, unsigned units,
                                                       float* __restrict__ acc) {
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  if (q >= units) return;
  const int c = blockIdx.y, b = b0 + (int)blockIdx.z;
  unsigned row, xq, zz, yy;
  fdivmod(q, fq, row, xq);
  fdivmod(row, fy, zz, yy);
  const int z = bz0 + (int)zz, y = by0 + (int)yy, x = bx0 + (VEC ? (int)xq * 4 : (int)xq);
  const long long rvol = (long long)g.rz * g.ry * g.rx;
  const long long o = (((long long)b * cout + c) * g.Dp + z) * g.Hp * (long long)g.Wp + (long long)y * g.Wp + x;
  float a[4];
  bool touched = false;
  for (int k = 0; k < n; ++k) {
    int wb, sz, sy, sx;
    sw_window(g, first + k, wb, sz, sy, sx);
    const int dz = z - sz, dy = y - sy, dx = x - sx;
    if (wb != b || (unsigned)dz >= (unsigned)g.rz || (unsigned)dy >= (unsigned)g.ry || (unsigned)dx >= (unsigned)g.rx)
      continue;
    if (!touched) {
      if (VEC) {
        const float4 t = ld4(acc + o);
        a[0] = t.x; a[1] = t.y; a[2] = t.z; a[3] = t.w;
      } else {
        a[0] = acc[o];
      }
      touched = true;
    }
    const long long l = ((long long)dz * g.ry + dy) * g.rx + dx;
    const float* p = pred + ((long long)k * cout + c) * rvol + l;
    if (VEC) {
      const float4 pv = ld4(p);
      const float4 w = CONST_IMP ? make_float4(1.f, 1.f, 1.f, 1.f) : ld4(imp + l);
      a[0] = add_rn(a[0], mul_rn(w.x, pv.x)); a[1] = add_rn(a[1], mul_rn(w.y, pv.y));
      a[2] = add_rn(a[2], mul_rn(w.z, pv.z)); a[3] = add_rn(a[3], mul_rn(w.w, pv.w));
    } else {
      a[0] = add_rn(a[0], mul_rn(CONST_IMP ? 1.f : imp[l], *p));
    }
  }
  if (!touched) return;
  if (VEC) st4(acc + o, make_float4(a[0], a[1], a[2], a[3]));
  else acc[o] = a[0];
}

// out[b][c] = acc / count over the unpadded region.  grid: (ceil(units / 256), cout, B).  VEC: W, Wp and the
// x padding are multiples of 4.
template <bool VEC>
__global__ __launch_bounds__(256) void sw_finalize_kernel(SwGeom g, const float* __restrict__ acc, int cout,
                                                          const float* __restrict__ count, FastDiv fq, FastDiv fy,
                                                          unsigned units, float* __restrict__ out) {
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  if (q >= units) return;
  const int c = blockIdx.y, b = blockIdx.z;
  unsigned row, xq, z, y;
  fdivmod(q, fq, row, xq);
  fdivmod(row, fy, z, y);
  const int x = VEC ? (int)xq * 4 : (int)xq;
  const long long ps = ((long long)(z + g.pz) * g.Hp + (y + g.py)) * g.Wp + (x + g.px);
  const long long pvol = (long long)g.Dp * g.Hp * g.Wp;
  const long long ao = ((long long)b * cout + c) * pvol + ps;
  const long long oo = ((long long)b * cout + c) * ((long long)g.D * g.H * g.W) + ((long long)z * g.H + y) * g.W + x;
  if (VEC) {
    const float4 s = ld4(acc + ao), n = ld4(count + ps);
    st4(out + oo, make_float4(s.x / n.x, s.y / n.y, s.z / n.z, s.w / n.w));
  } else {
    out[oo] = acc[ao] / count[ps];
  }
}

}  // namespace mpgan

using namespace mpgan;

namespace {

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

unsigned blocks_for(long long units) { return (unsigned)((units + 255) / 256); }

// Host validation of the geometry and its start table; fills the device view.
int sw_check(const mpgan_sw_geom* h, SwGeom& g, const char* what) {
  MPGAN_CHECK_ARG(h && h->starts_dev && h->starts_host, "%s: null geometry or start table", what);
  MPGAN_CHECK_ARG(h->batch > 0, "%s: batch must be positive", what);
  for (int d = 0; d < 3; ++d) {
    MPGAN_CHECK_ARG(h->dhw[d] > 0 && h->roi[d] > 0 && h->pad_lo[d] >= 0 && h->num[d] > 0,
                    "%s: bad extent/roi/padding/window count in dim %d", what, d);
    MPGAN_CHECK_ARG(h->padded[d] >= h->roi[d] && (long long)h->padded[d] >= (long long)h->dhw[d] + h->pad_lo[d],
                    "%s: padded extent %d of dim %d must hold the roi and the padded image", what, h->padded[d], d);
  }
  long long nwin = 1;
  int base = 0;
  for (int d = 0; d < 3; ++d) {
    for (int i = 0; i < h->num[d]; ++i) {
      const int s = h->starts_host[base + i];
      MPGAN_CHECK_ARG(s >= 0 && s <= h->padded[d] - h->roi[d], "%s: window start %d of dim %d outside [0, %d]", what, s,
                      d, h->padded[d] - h->roi[d]);
    }
    base += h->num[d];
    nwin *= h->num[d];
  }
  MPGAN_UNSUPPORTED(nwin * h->batch >= (1ll << 31), "%s: %lld windows exceed the int32 window index", what,
                    nwin * h->batch);
  const long long pplane = (long long)h->padded[0] * h->padded[1] * h->padded[2];
  MPGAN_UNSUPPORTED(pplane >= (1ll << 32) - 4, "%s: padded extent exceeds 2^32 voxels per channel", what);
  g.starts = h->starts_dev;
  g.D = h->dhw[0]; g.H = h->dhw[1]; g.W = h->dhw[2];
  g.pz = h->pad_lo[0]; g.py = h->pad_lo[1]; g.px = h->pad_lo[2];
  g.Dp = h->padded[0]; g.Hp = h->padded[1]; g.Wp = h->padded[2];
  g.rz = h->roi[0]; g.ry = h->roi[1]; g.rx = h->roi[2];
  g.nz = h->num[0]; g.ny = h->num[1]; g.nx = h->num[2];
  g.nwin = (int)nwin;
  return MPGAN_OK;
}

// Count and blend may use quads when no window boundary splits one.
bool sw_quads(const mpgan_sw_geom* h) {
  if (h->roi[2] % 4 || h->padded[2] % 4) return false;
  const int* sx = h->starts_host + h->num[0] + h->num[1];
  for (int i = 0; i < h->num[2]; ++i)
    if (sx[i] % 4) return false;
  return true;
}

int check_channels_calls(int32_t ch, int32_t first, int32_t n, const SwGeom& g, int32_t batch, const char* what) {
  MPGAN_CHECK_ARG(ch > 0 && ch <= 65535, "%s: channel count %d outside [1, 65535]", what, ch);
  MPGAN_CHECK_ARG(n > 0 && n <= 65535 && first >= 0 && (long long)first + n <= (long long)g.nwin * batch,
                  "%s: windows [%d, %d) outside the %lld of the batch (at most 65535 per call)", what, first,
                  first + n, (long long)g.nwin * batch);
  return MPGAN_OK;
}

// ---- the form of each launch: decided in ONE function per launch, which the launch and the label both read ------
// Gather: VEC when the roi's x extent is a multiple of 4 (the window batch must then be 16-byte aligned: refused
// otherwise), ALIGNED_IN from the input base.
struct SwGatherChoice { bool vec, aligned_in; };
int choose_sw_gather(const SwGeom& g, const void* in, const void* win, SwGatherChoice& c) {
  MPGAN_CHECK_ARG(in && win, "sw_gather: null pointer");
  c.vec = g.rx % 4 == 0;
  c.aligned_in = al16(in);
  MPGAN_UNSUPPORTED(c.vec && !al16(win), "sw_gather: the window batch must be 16-byte aligned");
  return MPGAN_OK;
}

// Count: quads when no window boundary splits one and count (and imp, when given) are 16-byte aligned.
struct SwWeightedChoice { bool vec, const_imp; };
int choose_sw_count(const mpgan_sw_geom* h, const void* imp, const void* count, SwWeightedChoice& c) {
  MPGAN_CHECK_ARG(count, "sw_count: null pointer");
  c.const_imp = imp == nullptr;
  c.vec = sw_quads(h) && al16(count) && (imp == nullptr || al16(imp));
  return MPGAN_OK;
}

// Blend: as the count, with pred and acc in place of count.
int choose_sw_blend(const mpgan_sw_geom* h, const void* pred, const void* imp, const void* acc, SwWeightedChoice& c) {
  MPGAN_CHECK_ARG(pred && acc, "sw_blend: null pointer");
  c.const_imp = imp == nullptr;
  c.vec = sw_quads(h) && al16(pred) && al16(acc) && (imp == nullptr || al16(imp));
  return MPGAN_OK;
}

// Finalize: quads when W, the padded W and the x padding are multiples of 4 and all three buffers are aligned.
struct SwFinalizeChoice { bool vec; };
int choose_sw_finalize(const SwGeom& g, const void* acc, const void* count, const void* out, SwFinalizeChoice& c) {
  MPGAN_CHECK_ARG(acc && count && out, "sw_finalize: null pointer");
  c.vec = g.W % 4 == 0 && g.Wp % 4 == 0 && g.px % 4 == 0 && al16(acc) && al16(count) && al16(out);
  return MPGAN_OK;
}

}  // namespace

extern "C" int mpgan_sw_gather(const mpgan_sw_geom* h, const float* in, int32_t cin, int32_t first, int32_t n,
                               float cval, float* win, void* stream) {
  SwGeom g;
  int rc = sw_check(h, g, "sw_gather");
  if (rc) return rc;
  rc = check_channels_calls(cin, first, n, g, h->batch, "sw_gather");
  if (rc) return rc;
  SwGatherChoice c;
  rc = choose_sw_gather(g, in, win, c);
  if (rc) return rc;
  const unsigned rx4 = (unsigned)(g.rx + 3) / 4;
  const long long quads = (long long)g.rz * g.ry * rx4;
  MPGAN_UNSUPPORTED(quads >= (1ll << 31), "sw_gather: roi too large");
  const dim3 grid(blocks_for(quads), cin, n);
  const FastDiv fq = make_fastdiv(rx4), fy = make_fastdiv(g.ry);
  hipStream_t s = (hipStream_t)stream;
#define MPGAN_SW_GATHER_(V, A)                                                                                       \
  hipLaunchKernelGGL((sw_gather_kernel<V, A>), grid, dim3(256), 0, s, in, g, cin, first, cval, fq, fy, (unsigned)quads, \
                     win)
  if (c.vec && c.aligned_in) MPGAN_SW_GATHER_(true, true);
  else if (c.vec) MPGAN_SW_GATHER_(true, false);
  else if (c.aligned_in) MPGAN_SW_GATHER_(false, true);
  else MPGAN_SW_GATHER_(false, false);
#undef MPGAN_SW_GATHER_
  return check_launch("sw_gather");
}

extern "C" int mpgan_sw_count(const mpgan_sw_geom* h, const float* imp, float* count, void* stream) {
  SwGeom g;
  int rc = sw_check(h, g, "sw_count");
  if (rc) return rc;
  SwWeightedChoice c;
  rc = choose_sw_count(h, imp, count, c);
  if (rc) return rc;
  const unsigned xu = c.vec ? (unsigned)g.Wp / 4 : (unsigned)g.Wp;
  const long long units = (long long)g.Dp * g.Hp * xu;
  const dim3 grid(blocks_for(units));
  const FastDiv fq = make_fastdiv(xu), fy = make_fastdiv(g.Hp);
  hipStream_t s = (hipStream_t)stream;
#define MPGAN_SW_COUNT_(V, CI) \
  hipLaunchKernelGGL((sw_count_kernel<V, CI>), grid, dim3(256), 0, s, g, imp, fq, fy, (unsigned)units, count)
  if (c.vec && !c.const_imp) MPGAN_SW_COUNT_(true, false);
  else if (c.vec) MPGAN_SW_COUNT_(true, true);
  else if (!c.const_imp) MPGAN_SW_COUNT_(false, false);
  else MPGAN_SW_COUNT_(false, true);
#undef MPGAN_SW_COUNT_
  return check_launch("sw_count");
}

extern "C" int mpgan_sw_blend(const mpgan_sw_geom* h, const float* pred, int32_t cout, int32_t first, int32_t n,
                              const float* imp, float* acc, void* stream) {
  SwGeom g;
  int rc = sw_check(h, g, "sw_blend");
  if (rc) return rc;
  rc = check_channels_calls(cout, first, n, g, h->batch, "sw_blend");
  if (rc) return rc;
  SwWeightedChoice c;
  rc = choose_sw_blend(h, pred, imp, acc, c);
  if (rc) return rc;
  // bounding box of the call's windows (padded coordinates) and the images they belong to
  int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {0, 0, 0};
  const int* sz = h->starts_host;
  const int* sy = sz + g.nz;
  const int* sx = sy + g.ny;
  for (int k = 0; k < n; ++k) {
    const int w = (first + k) % g.nwin;
    const int st[3] = {sz[w / (g.nx * g.ny)], sy[(w / g.nx) % g.ny], sx[w % g.nx]};
    for (int d = 0; d < 3; ++d) {
      lo[d] = st[d] < lo[d] ? st[d] : lo[d];
      hi[d] = st[d] + h->roi[d] > hi[d] ? st[d] + h->roi[d] : hi[d];
    }
  }
  const int b0 = first / g.nwin, b1 = (first + n - 1) / g.nwin;
  const unsigned xu = c.vec ? (unsigned)(hi[2] - lo[2]) / 4 : (unsigned)(hi[2] - lo[2]);
  const long long units = (long long)(hi[0] - lo[0]) * (hi[1] - lo[1]) * xu;
  const dim3 grid(blocks_for(units), cout, b1 - b0 + 1);
  const FastDiv fq = make_fastdiv(xu), fy = make_fastdiv(hi[1] - lo[1]);
  hipStream_t s = (hipStream_t)stream;
#define MPGAN_SW_BLEND_(V, CI)                                                                                        \
  hipLaunchKernelGGL((sw_blend_kernel<V, CI>), grid, dim3(256), 0, s, g, pred, cout, first, n, imp, b0, lo[0], lo[1], \
                     lo[2], fq, fy, (unsigned)units, acc)
  if (c.vec && !c.const_imp) MPGAN_SW_BLEND_(true, false);
  else if (c.vec) MPGAN_SW_BLEND_(true, true);
  else if (!c.const_imp) MPGAN_SW_BLEND_(false, false);
  else MPGAN_SW_BLEND_(false, true);
#undef MPGAN_SW_BLEND_
  return check_launch("sw_blend");
}

extern "C" int mpgan_sw_finalize(const mpgan_sw_geom* h, const float* acc, int32_t cout, const float* count,
                                 float* out, void* stream) {
  SwGeom g;
  int rc = sw_check(h, g, "sw_finalize");
  if (rc) return rc;
  SwFinalizeChoice c;
  rc = choose_sw_finalize(g, acc, count, out, c);
  if (rc) return rc;
  MPGAN_CHECK_ARG(cout > 0 && cout <= 65535 && h->batch <= 65535, "sw_finalize: channels / batch outside [1, 65535]");
  const unsigned xu = c.vec ? (unsigned)g.W / 4 : (unsigned)g.W;
  const long long units = (long long)g.D * g.H * xu;
  const dim3 grid(blocks_for(units), cout, h->batch);
  const FastDiv fq = make_fastdiv(xu), fy = make_fastdiv(g.H);
  hipStream_t s = (hipStream_t)stream;
  if (c.vec)
    hipLaunchKernelGGL((sw_finalize_kernel<true>), grid, dim3(256), 0, s, g, acc, cout, count, fq, fy,
                       (unsigned)units, out);
  else
    hipLaunchKernelGGL((sw_finalize_kernel<false>), grid, dim3(256), 0, s, g, acc, cout, count, fq, fy,
                       (unsigned)units, out);
  return check_launch("sw_finalize");
}

// The label of the instance a launch runs, formatted from the launch's own choice.
extern "C" int mpgan_sw_kernel_name(int32_t launch, const mpgan_sw_geom* h, const void* p0, const void* p1,
                                    const void* p2, char* buf, int32_t len) {
  MPGAN_CHECK_ARG(buf && len > 0, "sw_kernel_name: no buffer");
  MPGAN_CHECK_ARG(launch >= MPGAN_SW_GATHER && launch <= MPGAN_SW_FINALIZE, "sw_kernel_name: unknown launch %d", launch);
  static const char* const what[4] = {"sw_gather", "sw_count", "sw_blend", "sw_finalize"};
  static const char* const b[2] = {"false", "true"};
  SwGeom g;
  int rc = sw_check(h, g, what[launch]);
  if (rc) return rc;
  int n = 0;
  if (launch == MPGAN_SW_GATHER) {
    SwGatherChoice c;
    if ((rc = choose_sw_gather(g, p0, p1, c))) return rc;
    n = snprintf(buf, len, "sw_gather_kernel<%s, %s>", b[c.vec], b[c.aligned_in]);
  } else if (launch == MPGAN_SW_COUNT) {
    SwWeightedChoice c;
    if ((rc = choose_sw_count(h, p0, p1, c))) return rc;
    n = snprintf(buf, len, "sw_count_kernel<%s, %s>", b[c.vec], b[c.const_imp]);
  } else if (launch == MPGAN_SW_BLEND) {
    SwWeightedChoice c;
    if ((rc = choose_sw_blend(h, p0, p1, p2, c))) return rc;
    n = snprintf(buf, len, "sw_blend_kernel<%s, %s>", b[c.vec], b[c.const_imp]);
  } else {
    SwFinalizeChoice c;
    if ((rc = choose_sw_finalize(g, p0, p1, p2, c))) return rc;
    n = snprintf(buf, len, "sw_finalize_kernel<%s>", b[c.vec]);
  }
  MPGAN_CHECK_ARG(n < len, "sw_kernel_name: the name needs %d bytes", n + 1);
  return MPGAN_OK;
}
