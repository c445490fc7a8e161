// Paired affine augmentation of a (T1, T2) batch (include/mpgan_hip.h): one gather kernel.
//   map        output voxel p = (d, h, w) of sample s reads the input at c = A p + t, (A | t) = theta[s], a row-major
//              3 x 4 of doubles read on the device (block-uniform: scalar loads)
//   value      trilinear over floor(c) + {0,1}^3.  CONSTANT: a corner outside the input is `fill`; c is first clamped
//              to [-1, S] per axis, beyond which every corner of that axis is outside anyway (and the base index stays
//              an int whatever theta holds).  BORDER: c is clamped to [0, S - 1].  A NaN coordinate takes the lower
//              clamp.  A corner of weight exactly 0 (frac == 0) is not read: its index falls back on the base corner.
//   arithmetic c, the fractions and the seven lerps in fp64, + (double)sigma * noise in fp64 when the plane has noise
//              and sigma != 0, one rounding to fp32.  Integer-valued (A | t) give integer c exactly: copies are exact.
//   launch     one thread per output voxel and D-iteration; a block of 256 threads covers a TD x TH x TW tile of one
//              sample's output (W fastest: a wave's stores are whole 128-byte rows), so that under a rotation the
//              block's reads fall into a compact box of the input.  Coordinates and weights are computed once and used
//              for both planes.  No atomics, no grid cap (n * N_out < 2^31 bounds the tile count): two runs give the
//              same bits.
//   offsets    n * N_in, n * N_out < 2^31 are required, so every element offset fits 32 bits.
#include "mpgan_common.h"

namespace mpgan {

// Threads BD x BH x BW = 256, each walks ID steps of BD along d: the tile is (BD * ID) x BH x BW.
template <int BD_, int BH_, int BW_, int ID_>
struct WarpTile {
  static constexpr int BD = BD_, BH = BH_, BW = BW_, ID = ID_;
  static constexpr int TD = BD_ * ID_, TH = BH_, TW = BW_;
  static_assert(BD_ * BH_ * BW_ == 256, "256 threads");
};
using WarpTile3d = WarpTile<1, 8, 32, 4>;      // 4 x 8 x 32: volumes
using WarpTile2d = WarpTile<1, 8, 32, 1>;      // 1 x 8 x 32: images (D = 1)
#ifdef MPGAN_DEV_SWITCHES
// what else was measured: MPGAN_DBG_WARP_TILE = 0 .. 8 of the development build selects a tile
using WarpTileRow = WarpTile<1, 1, 256, 1>;    // 256 consecutive w
using WarpTileSq = WarpTile<1, 16, 16, 1>;
using WarpTileCube = WarpTile<4, 8, 8, 1>;
using WarpTileDeep = WarpTile<2, 4, 32, 4>;    // 8 x 4 x 32
using WarpTileWave = WarpTile<1, 4, 64, 1>;    // a wave per row of 64 w
using WarpTileWave4 = WarpTile<1, 4, 64, 4>;   // 4 x 4 x 64
using WarpTileHalf = WarpTile<1, 2, 128, 1>;
#endif

struct WarpDims {
  int in[3], out[3];
  FastDiv divTW, divTH, divTD;     // tile index -> (sample, tile d, tile h, tile w)
};

struct WarpAxis {
  int i0, i1;      // element indices of the two corners along this axis (i1 == i0 when the far corner has weight 0)
  bool ok0, ok1;   // CONSTANT: the corner lies inside the input
  double f;
};

template <bool BORDER>
__device__ __forceinline__ WarpAxis warp_axis(double c, int S) {
  WarpAxis a;
  const double lo = BORDER ? 0.0 : -1.0, hi = BORDER ? (double)(S - 1) : (double)S;
  c = !(c >= lo) ? lo : (c > hi ? hi : c);          // NaN -> lo
  const double fl = floor(c);
  const int b = (int)fl;                            // in [lo, hi]
  a.f = c - fl;
  const int b1 = a.f > 0.0 ? b + 1 : b;             // frac > 0 implies b < hi, so b1 <= hi
  a.ok0 = b >= 0 && b < S;
  a.ok1 = b1 >= 0 && b1 < S;
  a.i0 = a.ok0 ? b : 0;                             // an outside corner is never read; its index stays in range
  a.i1 = a.ok1 ? b1 : 0;
  return a;
}

template <bool BORDER>
__device__ __forceinline__ double warp_value(const float* __restrict__ x, const WarpAxis& ad, const WarpAxis& ah,
                                             const WarpAxis& aw, int sH, int sD, double fill) {
  const int r00 = ad.i0 * sD + ah.i0 * sH, r01 = ad.i0 * sD + ah.i1 * sH;
  const int r10 = ad.i1 * sD + ah.i0 * sH, r11 = ad.i1 * sD + ah.i1 * sH;
  auto at = [&](int row, bool okr, int i, bool okw) -> double {
    if (BORDER) return (double)x[row + i];
    return okr && okw ? (double)x[row + i] : fill;
  };
  const bool k00 = ad.ok0 && ah.ok0, k01 = ad.ok0 && ah.ok1, k10 = ad.ok1 && ah.ok0, k11 = ad.ok1 && ah.ok1;
  const double v000 = at(r00, k00, aw.i0, aw.ok0), v001 = at(r00, k00, aw.i1, aw.ok1);
  const double v010 = at(r01, k01, aw.i0, aw.ok0), v011 = at(r01, k01, aw.i1, aw.ok1);
  const double v100 = at(r10, k10, aw.i0, aw.ok0), v101 = at(r10, k10, aw.i1, aw.ok1);
  const double v110 = at(r11, k11, aw.i0, aw.ok0), v111 = at(r11, k11, aw.i1, aw.ok1);
  const double w00 = v000 + aw.f * (v001 - v000), w01 = v010 + aw.f * (v011 - v010);
  const double w10 = v100 + aw.f * (v101 - v100), w11 = v110 + aw.f * (v111 - v110);
  const double h0 = w00 + ah.f * (w01 - w00), h1 = w10 + ah.f * (w11 - w10);
  return h0 + ad.f * (h1 - h0);
}

template <class T, bool BORDER>
__global__ __launch_bounds__(256) void affine_warp_kernel(const float* __restrict__ x0, const float* __restrict__ x1,
                                                          WarpDims dm, const double* __restrict__ theta, float fill0,
                                                          float fill1, const float* __restrict__ noise0,
                                                          const float* __restrict__ noise1,
                                                          const float* __restrict__ sigma, float* __restrict__ y0,
                                                          float* __restrict__ y1) {
  unsigned q, tw, th, td, s;
  fdivmod(blockIdx.x, dm.divTW, q, tw);
  fdivmod(q, dm.divTH, q, th);
  fdivmod(q, dm.divTD, s, td);
  const int lw = threadIdx.x % T::BW, lh = (threadIdx.x / T::BW) % T::BH, ld = threadIdx.x / (T::BW * T::BH);
  const int w = (int)tw * T::TW + lw, h = (int)th * T::TH + lh;
  if (w >= dm.out[2] || h >= dm.out[1]) return;
  const double* __restrict__ th12 = theta + (size_t)s * 12;
  double A[3][4];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int j = 0; j < 4; ++j) A[k][j] = th12[k * 4 + j];
  const int Nin = dm.in[0] * dm.in[1] * dm.in[2], Nout = dm.out[0] * dm.out[1] * dm.out[2];
  const int sH = dm.in[2], sD = dm.in[1] * dm.in[2];
  const float* __restrict__ p0 = x0 + (size_t)s * Nin;
  const float* __restrict__ p1 = x1 ? x1 + (size_t)s * Nin : nullptr;
  const double sg0 = noise0 ? (double)sigma[s * 2] : 0.0, sg1 = noise1 ? (double)sigma[s * 2 + 1] : 0.0;
  double base[3];                                   // A p + t without the d term
#pragma unroll
  for (int k = 0; k < 3; ++k) base[k] = A[k][1] * (double)h + A[k][2] * (double)w + A[k][3];
#pragma unroll
  for (int i = 0; i < T::ID; ++i) {
    const int d = (int)td * T::TD + i * T::BD + ld;
    if (d >= dm.out[0]) break;
    const WarpAxis ad = warp_axis<BORDER>(A[0][0] * (double)d + base[0], dm.in[0]);
    const WarpAxis ah = warp_axis<BORDER>(A[1][0] * (double)d + base[1], dm.in[1]);
    const WarpAxis aw = warp_axis<BORDER>(A[2][0] * (double)d + base[2], dm.in[2]);
    const int o = (d * dm.out[1] + h) * dm.out[2] + w;
    const size_t go = (size_t)s * Nout + o;
    double v = warp_value<BORDER>(p0, ad, ah, aw, sH, sD, (double)fill0);
    if (sg0 != 0.0) v += sg0 * (double)noise0[go];
    y0[go] = (float)v;
    if (p1) {
      double u = warp_value<BORDER>(p1, ad, ah, aw, sH, sD, (double)fill1);
      if (sg1 != 0.0) u += sg1 * (double)noise1[go];
      y1[go] = (float)u;
    }
  }
}

}  // namespace mpgan

using namespace mpgan;

// n * D * H * W of one side: 0 and *N, or -1 with the error set.
static int warp_count(const char* side, int32_t n, const int32_t* dhw, long* N) {
  MPGAN_CHECK_ARG(dhw[0] >= 1 && dhw[1] >= 1 && dhw[2] >= 1, "mpgan_affine_warp: bad argument (%s extent %d x %d x %d)",
                  side, dhw[0], dhw[1], dhw[2]);
  const long cap = 0x7fffffffL;
  long e = n;
  for (int k = 0; k < 3; ++k) {
    MPGAN_CHECK_ARG(e <= cap / dhw[k], "mpgan_affine_warp: %s n * D * H * W = %d * %d * %d * %d exceeds the 32-bit element count",
                    side, n, dhw[0], dhw[1], dhw[2]);
    e *= dhw[k];
  }
  *N = e / n;
  return MPGAN_OK;
}

template <class T>
static int warp_launch(const float* x0, const float* x1, int32_t n, const int32_t* in_dhw, const int32_t* out_dhw,
                       const double* theta, int32_t mode, float fill0, float fill1, const float* noise0,
                       const float* noise1, const float* sigma, float* y0, float* y1, void* stream) {
  WarpDims dm;
  for (int k = 0; k < 3; ++k) { dm.in[k] = in_dhw[k]; dm.out[k] = out_dhw[k]; }
  const long tW = (out_dhw[2] + T::TW - 1) / T::TW, tH = (out_dhw[1] + T::TH - 1) / T::TH,
             tD = (out_dhw[0] + T::TD - 1) / T::TD;
  dm.divTW = make_fastdiv((unsigned)tW);
  dm.divTH = make_fastdiv((unsigned)tH);
  dm.divTD = make_fastdiv((unsigned)tD);
  const long tiles = (long)n * tD * tH * tW;        // every tile holds an output voxel of its own: <= n * N_out < 2^31
  const dim3 grid((unsigned)tiles), block(256);
  if (mode == MPGAN_WARP_BORDER)
    hipLaunchKernelGGL((affine_warp_kernel<T, true>), grid, block, 0, (hipStream_t)stream, x0, x1, dm, theta, fill0, fill1,
                       noise0, noise1, sigma, y0, y1);
  else
    hipLaunchKernelGGL((affine_warp_kernel<T, false>), grid, block, 0, (hipStream_t)stream, x0, x1, dm, theta, fill0, fill1,
                       noise0, noise1, sigma, y0, y1);
  return check_launch("mpgan_affine_warp");
}

extern "C" int mpgan_affine_warp(const float* x0, const float* x1, int32_t n, const int32_t* in_dhw,
                                 const int32_t* out_dhw, const double* theta, int32_t mode, float fill0, float fill1,
                                 const float* noise0, const float* noise1, const float* sigma, float* y0, float* y1,
                                 void* stream) {
  MPGAN_CHECK_ARG(x0 && y0 && theta && in_dhw && out_dhw, "mpgan_affine_warp: bad argument (null x0 / y0 / theta / in_dhw / out_dhw)");
  MPGAN_CHECK_ARG((x1 != nullptr) == (y1 != nullptr), "mpgan_affine_warp: bad argument (x1 and y1 go together: %s alone)",
                  x1 ? "x1" : "y1");
  MPGAN_CHECK_ARG(n > 0, "mpgan_affine_warp: bad argument (n = %d)", n);
  MPGAN_CHECK_ARG(mode == MPGAN_WARP_CONSTANT || mode == MPGAN_WARP_BORDER, "mpgan_affine_warp: unknown mode %d (constant 0, border 1)", mode);
  MPGAN_CHECK_ARG(!(noise0 || noise1) || sigma, "mpgan_affine_warp: bad argument (noise without sigma)");
  MPGAN_CHECK_ARG(!sigma || noise0 || noise1, "mpgan_affine_warp: bad argument (sigma without noise)");
  MPGAN_CHECK_ARG(!noise1 || x1, "mpgan_affine_warp: bad argument (noise1 without the second plane)");
  long Nin, Nout;
  if (int rc = warp_count("input", n, in_dhw, &Nin)) return rc;
  if (int rc = warp_count("output", n, out_dhw, &Nout)) return rc;
  int tile = out_dhw[0] > 1 ? 0 : 1;
  if (const char* e = dev_env("MPGAN_DBG_WARP_TILE")) tile = atoi(e);
#define MPGAN_WARP_GO(T) return warp_launch<T>(x0, x1, n, in_dhw, out_dhw, theta, mode, fill0, fill1, noise0, noise1, sigma, y0, y1, stream)
  switch (tile) {
    case 0: MPGAN_WARP_GO(WarpTile3d);
    case 1: MPGAN_WARP_GO(WarpTile2d);
#ifdef MPGAN_DEV_SWITCHES
    case 2: MPGAN_WARP_GO(WarpTileRow);
    case 3: MPGAN_WARP_GO(WarpTileSq);
    case 4: MPGAN_WARP_GO(WarpTileCube);
    case 5: MPGAN_WARP_GO(WarpTileDeep);
    case 6: MPGAN_WARP_GO(WarpTileWave);
    case 7: MPGAN_WARP_GO(WarpTileWave4);
    case 8: MPGAN_WARP_GO(WarpTileHalf);
#endif
  }
#undef MPGAN_WARP_GO
  set_error("mpgan_affine_warp: unknown tile %d", tile);
  return MPGAN_ERR_INVALID;
}
