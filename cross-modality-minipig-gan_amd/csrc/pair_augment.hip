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
//
// Elastic deformation and intensity augmentation of the same pair (mpgan_deform_warp): a second kernel on the
// same tiles, the same warp_axis / warp_value and the same expression for A p + t.
//   map        c = (A p + t) + u(p), u a cubic B-spline free-form deformation over the OUTPUT extent from a per-sample
//              lattice of control displacements; the lattice coordinate of an axis depends on that axis's index alone
//   value      as above, then on the planes of gain_planes v += (v - lo) * expm1(b(p)) (b: a B-spline of a log-gain
//              lattice; skipped where expm1(b) == 0), then v = lo + R * pow(max(v - lo, 0) / R, gamma) (skipped where
//              gamma == 1), then the noise term as above.  Zero lattices and gamma 1 give the affine kernel's bits.
//   row lattices  a block covers a 1 x 8 x 32 tile whatever the depth (one d, BH rows of h).  It first reduces the d and h
//              sums of both lattices once per row into LDS: BH rows x (3 + 1) channels x g_w doubles (<= 16 KiB, static).
//              After one barrier a voxel adds 4 terms per channel with the weights of its w.  Every sum has a fixed
//              order; no atomics.
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

// c_k = A p + t along one axis, Ak = row k of (A | t): the one expression every kernel of this file evaluates the map
// with (the backward's weights are the forward's only if both round alike): the (h, w) part first, the d term added to it.
__device__ __forceinline__ double warp_base(const double* Ak, int h, int w) {
  return Ak[1] * (double)h + Ak[2] * (double)w + Ak[3];
}
__device__ __forceinline__ double warp_coord(const double* Ak, int d, double base) { return Ak[0] * (double)d + base; }

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
  for (int k = 0; k < 3; ++k) base[k] = warp_base(A[k], h, w);
#pragma unroll
  for (int i = 0; i < T::ID; ++i) {
    const int d = (int)td * T::TD + i * T::BD + ld;
    if (d >= dm.out[0]) break;
    const WarpAxis ad = warp_axis<BORDER>(warp_coord(A[0], d, base[0]), dm.in[0]);
    const WarpAxis ah = warp_axis<BORDER>(warp_coord(A[1], d, base[1]), dm.in[1]);
    const WarpAxis aw = warp_axis<BORDER>(warp_coord(A[2], d, base[2]), dm.in[2]);
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

// ---- mpgan_affine_warp_backward ------------------------------------------------------------------------------------------
// The adjoint of the CONSTANT kernel above in x, as a gather: one thread per INPUT voxel q on the forward's tiles (of
// the input extent this time), no atomics, every sum in increasing linear order of p.
//   weights    g_x[q] = sum_p g_y[p] tent(c_d(p) - q_d) tent(c_h(p) - q_h) tent(c_w(p) - q_w), c by warp_base / warp_coord
//   candidates a contributor has |c(p) - q| < 1 on every axis, so p = p* + A^-1 e with p* = A^-1 (q - t), |e_j| < 1:
//              |p_k - p*_k| < r_k = sum_j |A^-1[k][j]|.  The box is walked over (p_d, p_h); along w the three
//              conditions are linear in p_w and cut the box's row down to one interval.  Box and interval only prune
//              (both are widened by kWarpSlack against their own rounding): the tents decide, and a weight of exactly
//              0 is neither read nor added.
//   bound      a sample with det A not finite, det A == 0 or an r_k > MPGAN_WARP_REACH_MAX gets NaN everywhere and no
//              loop at all, so a thread visits at most 9 x 9 rows of at most 9 voxels whatever theta holds.
constexpr double kWarpSlack = 1e-6;

__device__ __forceinline__ double warp_tent(double u) {
  const double a = fabs(u);
  return a < 1.0 ? 1.0 - a : 0.0;                   // NaN -> 0
}

// [lo, hi] = the integers of [x - r, x + r] inside [0, S - 1]; empty (hi < lo) for a NaN.  r <= MPGAN_WARP_REACH_MAX, so
// at most 9 of them.
__device__ __forceinline__ void warp_reach(double x, double r, int S, int& lo, int& hi) {
  const double l = ceil(x - r - kWarpSlack), u = floor(x + r + kWarpSlack);
  lo = l > 0.0 ? (l > (double)S ? S : (int)l) : 0;
  hi = !(u >= -1.0) ? -1 : (u < (double)(S - 1) ? (int)u : S - 1);
}

// Cut [w0, w1] down to the p_w with |b + a p_w| < 1 (ia = 1 / a).  A bound that is NaN cuts nothing.
__device__ __forceinline__ void warp_cut(double b, double a, double ia, int& w0, int& w1) {
  if (a == 0.0) {
    if (!(fabs(b) < 1.0 + kWarpSlack)) w1 = w0 - 1;
    return;
  }
  const double x0 = (-1.0 - b) * ia, x1 = (1.0 - b) * ia;       // (a small |a| makes both large: the slack is relative)
  const double xl = a > 0.0 ? x0 : x1, xu = a > 0.0 ? x1 : x0;
  const double l = ceil(xl - kWarpSlack * (1.0 + fabs(xl))), u = floor(xu + kWarpSlack * (1.0 + fabs(xu)));
  if (l > (double)w0) w0 = l > (double)w1 ? w1 + 1 : (int)l;
  if (u < (double)w1) w1 = u < (double)w0 ? w0 - 1 : (int)u;
}

// dm.in: the extent of g_y (what is read: the forward's output), dm.out: the extent of g_x (what is written and tiled).
template <class T>
__global__ __launch_bounds__(256) void affine_warp_backward_kernel(const float* __restrict__ gy, WarpDims dm,
                                                                   const double* __restrict__ theta,
                                                                   float* __restrict__ gx) {
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
  // A^-1 = adj(A) / det A, its row sums r_k, and 1 / A[k][2] for the cuts along w: once per thread, block-uniform
  double Ai[3][3];
  Ai[0][0] = A[1][1] * A[2][2] - A[1][2] * A[2][1];
  Ai[0][1] = A[0][2] * A[2][1] - A[0][1] * A[2][2];
  Ai[0][2] = A[0][1] * A[1][2] - A[0][2] * A[1][1];
  Ai[1][0] = A[1][2] * A[2][0] - A[1][0] * A[2][2];
  Ai[1][1] = A[0][0] * A[2][2] - A[0][2] * A[2][0];
  Ai[1][2] = A[0][2] * A[1][0] - A[0][0] * A[1][2];
  Ai[2][0] = A[1][0] * A[2][1] - A[1][1] * A[2][0];
  Ai[2][1] = A[0][1] * A[2][0] - A[0][0] * A[2][1];
  Ai[2][2] = A[0][0] * A[1][1] - A[0][1] * A[1][0];
  const double det = A[0][0] * Ai[0][0] + A[0][1] * Ai[1][0] + A[0][2] * Ai[2][0];
  const double idet = 1.0 / det;
  double r[3], ia[3];
  bool ok = det != 0.0 && fabs(det) < HUGE_VAL;     // (a NaN fails the second test)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int j = 0; j < 3; ++j) Ai[k][j] *= idet;
    r[k] = fabs(Ai[k][0]) + fabs(Ai[k][1]) + fabs(Ai[k][2]);
    ok = ok && r[k] <= MPGAN_WARP_REACH_MAX;        // (a NaN fails)
    ia[k] = 1.0 / A[k][2];
  }
  const int Ngy = dm.in[0] * dm.in[1] * dm.in[2], Ngx = dm.out[0] * dm.out[1] * dm.out[2];
  const float* __restrict__ g = gy + (size_t)s * Ngy;
  float* __restrict__ o = gx + (size_t)s * Ngx;
#pragma unroll 1
  for (int i = 0; i < T::ID; ++i) {
    const int d = (int)td * T::TD + i * T::BD + ld;
    if (d >= dm.out[0]) break;
    const int at = (d * dm.out[1] + h) * dm.out[2] + w;
    if (!ok) {
      o[at] = __builtin_nanf("");
      continue;
    }
    const double e0 = (double)d - A[0][3], e1 = (double)h - A[1][3], e2 = (double)w - A[2][3];
    int lo[3], hi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
      warp_reach(Ai[k][0] * e0 + Ai[k][1] * e1 + Ai[k][2] * e2, r[k], dm.in[k], lo[k], hi[k]);
    double acc = 0.0;
    if (lo[2] <= hi[2]) {
      for (int pd = lo[0]; pd <= hi[0]; ++pd) {
        for (int ph = lo[1]; ph <= hi[1]; ++ph) {
          double base[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) base[k] = A[k][0] * (double)pd + A[k][1] * (double)ph + A[k][3];
          int w0 = lo[2], w1 = hi[2];
          warp_cut(base[0] - (double)d, A[0][2], ia[0], w0, w1);
          warp_cut(base[1] - (double)h, A[1][2], ia[1], w0, w1);
          warp_cut(base[2] - (double)w, A[2][2], ia[2], w0, w1);
          const int row = (pd * dm.in[1] + ph) * dm.in[2];
          for (int pw = w0; pw <= w1; ++pw) {
            const double wd = warp_tent(warp_coord(A[0], pd, warp_base(A[0], ph, pw)) - (double)d);
            const double wh = warp_tent(warp_coord(A[1], pd, warp_base(A[1], ph, pw)) - (double)h);
            const double ww = warp_tent(warp_coord(A[2], pd, warp_base(A[2], ph, pw)) - (double)w);
            if (wd == 0.0 || wh == 0.0 || ww == 0.0) continue;
            acc += (double)g[row + pw] * wd * wh * ww;
          }
        }
      }
    }
    o[at] = (float)acc;
  }
}

// ---- mpgan_affine_warp_backward_theta ------------------------------------------------------------------------------------
// The derivative of the CONSTANT kernel in theta (include/mpgan_hip.h): y is trilinear in c and c_k is linear
// in row k of theta, so g_theta[k][j] = sum_p (sum_planes g_y[p] dy/dc_k(p)) P_j(p), P = (d, h, w, 1).
//   voxel      c by warp_base / warp_coord; dead (any c_k NaN or outside [-1, S_k]: nothing read, nothing added); else
//              b = floor(c), f = c - b and ALL eight corners b + {0,1}^3, `fill` outside the input: the forward skips a
//              corner of weight 0, but the derivative along an axis is the difference across it whatever f is.  At an
//              integer c this is the right-hand derivative, on the cell [b, b + 1].
//   launch 1   the forward's tiles of the output, one thread per (h, w) walking the tile's d steps: 12 sums per thread in
//              increasing d, block_sum_n (reduce.h) over the 12 entries, 12 doubles to ws[sample][tile][12]
//   launch 2   one block per (sample, entry): thread t adds tiles t, t + 256, .. in order, then block_tree_sum<256>
// No atomics; grid and orders depend on (n, out_dhw) alone.  Cell and fractions are computed once for both planes.
struct WarpCell {
  int i[3][2];      // element index of the two corners along each axis (0 where the corner is outside: never read)
  bool ok[3][2];
  double f[3];
};

// The eight corners of one plane -> dy/dc_d, dy/dc_h, dy/dc_w.
__device__ __forceinline__ void warp_slopes(const float* __restrict__ x, const WarpCell& c, int sH, int sD, double fill,
                                            double& dd, double& dh, double& dw) {
  double v[2][2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int row = c.i[0][a] * sD + c.i[1][b] * sH;
      const bool okr = c.ok[0][a] && c.ok[1][b];
#pragma unroll
      for (int e = 0; e < 2; ++e) v[a][b][e] = okr && c.ok[2][e] ? (double)x[row + c.i[2][e]] : fill;
    }
  auto lerp = [](double p, double q, double f) { return p + f * (q - p); };
  const double fd = c.f[0], fh = c.f[1], fw = c.f[2];
  dd = lerp(lerp(v[1][0][0] - v[0][0][0], v[1][0][1] - v[0][0][1], fw),
            lerp(v[1][1][0] - v[0][1][0], v[1][1][1] - v[0][1][1], fw), fh);
  dh = lerp(lerp(v[0][1][0] - v[0][0][0], v[0][1][1] - v[0][0][1], fw),
            lerp(v[1][1][0] - v[1][0][0], v[1][1][1] - v[1][0][1], fw), fd);
  dw = lerp(lerp(v[0][0][1] - v[0][0][0], v[0][1][1] - v[0][1][0], fh),
            lerp(v[1][0][1] - v[1][0][0], v[1][1][1] - v[1][1][0], fh), fd);
}

template <class T>
__global__ __launch_bounds__(256) void affine_warp_theta_tile_kernel(const float* __restrict__ x0,
                                                                     const float* __restrict__ x1,
                                                                     const float* __restrict__ gy0,
                                                                     const float* __restrict__ gy1, WarpDims dm,
                                                                     const double* __restrict__ theta, float fill0,
                                                                     float fill1, double* __restrict__ ws) {
  static_assert(T::BD == 1, "one thread per (h, w)");
  __shared__ double sh[12 * 256];
  unsigned q, tw, th, td, s;
  fdivmod(blockIdx.x, dm.divTW, q, tw);
  fdivmod(q, dm.divTH, q, th);
  fdivmod(q, dm.divTD, s, td);
  const int lw = threadIdx.x % T::BW, lh = threadIdx.x / T::BW;
  const int w = (int)tw * T::TW + lw, h = (int)th * T::TH + lh;
  double acc[12];                                     // [k][j], row-major like theta
#pragma unroll
  for (int e = 0; e < 12; ++e) acc[e] = 0.0;
  if (w < dm.out[2] && h < dm.out[1]) {               // (a thread outside the output stays for the block sums)
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
    double base[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) base[k] = warp_base(A[k], h, w);
#pragma unroll
    for (int i = 0; i < T::ID; ++i) {
      const int d = (int)td * T::TD + i;
      if (d >= dm.out[0]) break;
      WarpCell cell;
      bool alive = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double c = warp_coord(A[k], d, base[k]);
        alive = alive && c >= -1.0 && c <= (double)dm.in[k];       // a NaN fails
        const double fl = floor(alive ? c : 0.0);
        const int b = (int)fl;                                     // in [-1, S]
        cell.f[k] = (alive ? c : 0.0) - fl;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          cell.ok[k][e] = b + e >= 0 && b + e < dm.in[k];
          cell.i[k][e] = cell.ok[k][e] ? b + e : 0;
        }
      }
      if (!alive) continue;
      const size_t go = (size_t)s * Nout + (size_t)((d * dm.out[1] + h) * dm.out[2] + w);
      double dd, dh, dw;
      warp_slopes(p0, cell, sH, sD, (double)fill0, dd, dh, dw);
      const double g0 = (double)gy0[go];
      double G[3] = {g0 * dd, g0 * dh, g0 * dw};
      if (p1) {
        warp_slopes(p1, cell, sH, sD, (double)fill1, dd, dh, dw);
        const double g1 = (double)gy1[go];
        G[0] += g1 * dd;
        G[1] += g1 * dh;
        G[2] += g1 * dw;
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        acc[k * 4 + 0] += G[k] * (double)d;
        acc[k * 4 + 1] += G[k] * (double)h;
        acc[k * 4 + 2] += G[k] * (double)w;
        acc[k * 4 + 3] += G[k];
      }
    }
  }
  const double t = block_sum_n<12>(acc, sh);                        // entry threadIdx.x / 16 in the threads < 192
  if (threadIdx.x < 192 && (threadIdx.x & 15) == 0)
    ws[(size_t)blockIdx.x * 12 + (threadIdx.x >> 4)] = t;            // blockIdx.x = sample * tiles + tile
}

// g_theta[s][e] = the sum over the sample's tiles of ws[s][tile][e], one block per (sample, entry): thread t takes tiles
// t, t + 256, .. in order, then block_tree_sum<256> (loss_item_kernel's scheme; a block per entry instead of twelve trees
// in a row in one block: the same order per entry, a twelfth of the barriers in a row).
__global__ __launch_bounds__(256) void affine_warp_theta_sum_kernel(const double* __restrict__ ws, int tiles,
                                                                    double* __restrict__ gtheta) {
  __shared__ double red[256];
  const unsigned s = blockIdx.x / 12, e = blockIdx.x % 12;
  const double* __restrict__ p = ws + (size_t)s * tiles * 12 + e;
  double acc = 0.0;
  for (int i = threadIdx.x; i < tiles; i += 256) acc += p[(size_t)i * 12];
  acc = block_tree_sum<256>(acc, red);
  if (threadIdx.x == 0) gtheta[blockIdx.x] = acc;
}

// ---- mpgan_deform_warp ---------------------------------------------------------------------------------------------------
constexpr int kLatticeMax = 64;                   // the largest lattice extent per axis (the LDS rows are sized by it)

struct DeformArgs {
  const double* ctrl;      // [n][3][cg0][cg1][cg2] control displacements in input voxels, or null
  const double* gain;      // [n][gg0][gg1][gg2] log-gain control values, or null
  const double* gamma;     // [n][2], or null
  int cg[3], gg[3];
  int gain_planes;
  double lo, hi;
};

// One axis of the lattice rule: the four entries min(i0 + a, g - 1), a = 0..3, with the weights B[a].  An axis of
// output extent 1 has the lattice extent 1 and the single weight 1 (the other three weights are 0 on entry 0).
struct SplineAxis {
  int i0;
  double B[4];
};

__device__ __forceinline__ SplineAxis spline_axis(int p, int S, int g) {
  SplineAxis a;
  if (g < 4) {
    a.i0 = 0;
    a.B[0] = 1.0; a.B[1] = 0.0; a.B[2] = 0.0; a.B[3] = 0.0;
    return a;
  }
  const double xi = 1.0 + ((double)p * (double)(g - 3)) / (double)(S - 1);      // g >= 4 implies S > 1 (host check)
  int i = (int)floor(xi);
  i = i < 1 ? 1 : (i > g - 3 ? g - 3 : i);         // xi in [1, g - 2]: the clamp keeps every index inside whatever p is
  const double f = xi - (double)i, f2 = f * f, f3 = f2 * f, m = 1.0 - f;
  a.i0 = i - 1;
  a.B[0] = m * m * m / 6.0;
  a.B[1] = (3.0 * f3 - 6.0 * f2 + 4.0) / 6.0;
  a.B[2] = (-3.0 * f3 + 3.0 * f2 + 3.0 * f + 1.0) / 6.0;
  a.B[3] = f3 / 6.0;
  return a;
}

// rows[(r * NCH + k) * g[2] + j] = sum over a, b of Bd[a] Bh[b] L[k][id + a][ih + b][j] for the ROWS rows h0 + r of the
// tile at depth weights `ad` (L: one sample's lattice [NCH][g0][g1][g2]).  A row beyond the output takes the last
// row's weights; nobody reads it.
template <int ROWS, int NCH>
__device__ __forceinline__ void spline_rows(double* __restrict__ rows, const double* __restrict__ L, const int* g,
                                            const SplineAxis& ad, int h0, int outH) {
  const int gw = g[2], total = ROWS * NCH * gw;
  for (int e = threadIdx.x; e < total; e += 256) {
    const int j = e % gw, q = e / gw, k = q % NCH, r = q / NCH;
    const int h = h0 + r < outH ? h0 + r : outH - 1;
    const SplineAxis ah = spline_axis(h, outH, g[1]);
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int id = ad.i0 + a < g[0] ? ad.i0 + a : g[0] - 1;
      double row = 0.0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int ih = ah.i0 + b < g[1] ? ah.i0 + b : g[1] - 1;
        row += ah.B[b] * L[((size_t)(k * g[0] + id) * g[1] + ih) * gw + j];
      }
      acc += ad.B[a] * row;
    }
    rows[e] = acc;
  }
}

__device__ __forceinline__ double spline_row_value(const double* __restrict__ row, const SplineAxis& aw, int gw) {
  double acc = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) acc += aw.B[c] * row[aw.i0 + c < gw ? aw.i0 + c : gw - 1];
  return acc;
}

#ifdef MPGAN_DEV_SWITCHES
// what else was measured: the literal 64-term sum per voxel and channel, straight from the lattice
template <int NCH>
__device__ __forceinline__ void spline_voxel(double* __restrict__ out, const double* __restrict__ L, const int* g,
                                             const SplineAxis& ad, const SplineAxis& ah, const SplineAxis& aw) {
  for (int k = 0; k < NCH; ++k) {
    double acc = 0.0;
    for (int a = 0; a < 4; ++a) {
      const int id = ad.i0 + a < g[0] ? ad.i0 + a : g[0] - 1;
      for (int b = 0; b < 4; ++b) {
        const int ih = ah.i0 + b < g[1] ? ah.i0 + b : g[1] - 1;
        const double* row = L + ((size_t)(k * g[0] + id) * g[1] + ih) * g[2];
        double t = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) t += aw.B[c] * row[aw.i0 + c < g[2] ? aw.i0 + c : g[2] - 1];
        acc += ad.B[a] * ah.B[b] * t;
      }
    }
    out[k] = acc;
  }
}
#endif

// gain (e = expm1 of the log-gain, 0 on a plane without gain) and gamma around lo; a value of exactly lo stays lo
__device__ __forceinline__ double warp_intensity(double v, double e, double gam, double lo, double R) {
  if (e != 0.0) v += (v - lo) * e;
  if (gam != 1.0) v = lo + R * pow(fmax(v - lo, 0.0) / R, gam);
  return v;
}

template <class T, bool BORDER, bool ROWS = true>
__global__ __launch_bounds__(256) void deform_warp_kernel(const float* __restrict__ x0, const float* __restrict__ x1,
                                                          WarpDims dm, const double* __restrict__ theta, DeformArgs df,
                                                          float fill0, float fill1, const float* __restrict__ noise0,
                                                          const float* __restrict__ noise1,
                                                          const float* __restrict__ sigma, float* __restrict__ y0,
                                                          float* __restrict__ y1) {
  static_assert(T::BD == 1, "the row lattices are per d step: every thread of the block has the same d");
  __shared__ double s_ctrl[ROWS ? T::BH * 3 * kLatticeMax : 1];
  __shared__ double s_gain[ROWS ? T::BH * kLatticeMax : 1];
  unsigned q, tw, th, td, s;
  fdivmod(blockIdx.x, dm.divTW, q, tw);
  fdivmod(q, dm.divTH, q, th);
  fdivmod(q, dm.divTD, s, td);
  const int lw = threadIdx.x % T::BW, lh = threadIdx.x / T::BW;
  const int w = (int)tw * T::TW + lw, h = (int)th * T::TH + lh;
  const bool active = w < dm.out[2] && h < dm.out[1];        // (no early return: the block meets at barriers)
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
  const double* __restrict__ cl = df.ctrl ? df.ctrl + (size_t)s * 3 * df.cg[0] * df.cg[1] * df.cg[2] : nullptr;
  const double* __restrict__ gl = df.gain ? df.gain + (size_t)s * df.gg[0] * df.gg[1] * df.gg[2] : nullptr;
  const double gam0 = df.gamma ? df.gamma[s * 2] : 1.0, gam1 = df.gamma ? df.gamma[s * 2 + 1] : 1.0;
  const double R = df.hi - df.lo;
  const int wc = w < dm.out[2] ? w : dm.out[2] - 1;
  SplineAxis cw, gw;                                // this thread's w weights: the same at every d step
  if (cl) cw = spline_axis(wc, dm.out[2], df.cg[2]);
  if (gl) gw = spline_axis(wc, dm.out[2], df.gg[2]);
  double base[3];                                   // A p + t without the d term
#pragma unroll
  for (int k = 0; k < 3; ++k) base[k] = warp_base(A[k], h, w);
#pragma unroll 1
  for (int i = 0; i < T::ID; ++i) {                 // (ID == 1 in the product: one d step per block)
    const int d = (int)td * T::TD + i;
    if (d >= dm.out[0]) break;                      // the same for every thread of the block
    if (ROWS) {
      if (i) __syncthreads();                       // the last step's reads are done
      if (cl) spline_rows<T::BH, 3>(s_ctrl, cl, df.cg, spline_axis(d, dm.out[0], df.cg[0]), (int)th * T::TH, dm.out[1]);
      if (gl) spline_rows<T::BH, 1>(s_gain, gl, df.gg, spline_axis(d, dm.out[0], df.gg[0]), (int)th * T::TH, dm.out[1]);
      __syncthreads();
    }
    if (!active) continue;
    double c0 = warp_coord(A[0], d, base[0]);
    double c1 = warp_coord(A[1], d, base[1]);
    double c2 = warp_coord(A[2], d, base[2]);
    double b = 0.0;                                 // the log-gain
    if (cl) {                                       // an axis of extent 1 has no displacement
      double u[3];
      if (ROWS) {
        const double* row = s_ctrl + lh * 3 * df.cg[2];
        u[0] = spline_row_value(row, cw, df.cg[2]);
        u[1] = spline_row_value(row + df.cg[2], cw, df.cg[2]);
        u[2] = spline_row_value(row + 2 * df.cg[2], cw, df.cg[2]);
      }
#ifdef MPGAN_DEV_SWITCHES
      else
        spline_voxel<3>(u, cl, df.cg, spline_axis(d, dm.out[0], df.cg[0]), spline_axis(h, dm.out[1], df.cg[1]), cw);
#endif
      c0 += dm.out[0] > 1 ? u[0] : 0.0;
      c1 += dm.out[1] > 1 ? u[1] : 0.0;
      c2 += dm.out[2] > 1 ? u[2] : 0.0;
    }
    if (gl) {
      if (ROWS) b = spline_row_value(s_gain + lh * df.gg[2], gw, df.gg[2]);
#ifdef MPGAN_DEV_SWITCHES
      else
        spline_voxel<1>(&b, gl, df.gg, spline_axis(d, dm.out[0], df.gg[0]), spline_axis(h, dm.out[1], df.gg[1]), gw);
#endif
    }
    const double e = gl ? expm1(b) : 0.0;
    const WarpAxis ad = warp_axis<BORDER>(c0, dm.in[0]);
    const WarpAxis ah = warp_axis<BORDER>(c1, dm.in[1]);
    const WarpAxis aw = warp_axis<BORDER>(c2, dm.in[2]);
    const int o = (d * dm.out[1] + h) * dm.out[2] + w;
    const size_t go = (size_t)s * Nout + o;
    double v = warp_value<BORDER>(p0, ad, ah, aw, sH, sD, (double)fill0);
    v = warp_intensity(v, (df.gain_planes & 1) ? e : 0.0, gam0, df.lo, R);
    if (sg0 != 0.0) v += sg0 * (double)noise0[go];
    y0[go] = (float)v;
    if (p1) {
      double u = warp_value<BORDER>(p1, ad, ah, aw, sH, sD, (double)fill1);
      u = warp_intensity(u, (df.gain_planes & 2) ? e : 0.0, gam1, df.lo, R);
      if (sg1 != 0.0) u += sg1 * (double)noise1[go];
      y1[go] = (float)u;
    }
  }
}

}  // namespace mpgan

using namespace mpgan;

// What every warp entry point refuses: a null required pointer (`given`: the entry point's own, spelled out in `names`),
// n, the mode, and an extent or element count of either side.  An entry point without a border mode passes what the
// border mode lacks there and why as `constant_only`; null: both modes are taken.
static int warp_check(const char* fn, bool given, const char* names, int32_t n, const int32_t* in_dhw,
                      const int32_t* out_dhw, int32_t mode, const char* constant_only) {
  MPGAN_CHECK_ARG(given && in_dhw && out_dhw, "%s: bad argument (null %s / in_dhw / out_dhw)", fn, names);
  MPGAN_CHECK_ARG(n > 0, "%s: bad argument (n = %d)", fn, n);
  MPGAN_CHECK_ARG(mode == MPGAN_WARP_CONSTANT || mode == MPGAN_WARP_BORDER, "%s: unknown mode %d (constant 0%s)", fn, mode,
                  constant_only ? "" : ", border 1");
  MPGAN_CHECK_ARG(!constant_only || mode != MPGAN_WARP_BORDER, "%s: the border mode has no %s; constant 0 only", fn,
                  constant_only);
  long N;
  if (int rc = element_count(fn, "input ", n, in_dhw, &N)) return rc;
  return element_count(fn, "output ", n, out_dhw, &N);
}

// The second plane's two pointers (a, b: their names) are both given or both null.
#define MPGAN_WARP_PAIR(fn, a, b) \
  MPGAN_CHECK_ARG((a != nullptr) == (b != nullptr), "%s: bad argument (" #a " and " #b " go together: %s alone)", fn, a ? #a : #b)

// What both forward entry points refuse.
static int warp_forward_check(const char* fn, const float* x0, const float* x1, int32_t n, const int32_t* in_dhw,
                              const int32_t* out_dhw, const double* theta, int32_t mode, const float* noise0,
                              const float* noise1, const float* sigma, const float* y0, const float* y1) {
  if (int rc = warp_check(fn, x0 && y0 && theta, "x0 / y0 / theta", n, in_dhw, out_dhw, mode, nullptr)) return rc;
  MPGAN_WARP_PAIR(fn, x1, y1);
  MPGAN_CHECK_ARG(!(noise0 || noise1) || sigma, "%s: bad argument (noise without sigma)", fn);
  MPGAN_CHECK_ARG(!sigma || noise0 || noise1, "%s: bad argument (sigma without noise)", fn);
  MPGAN_CHECK_ARG(!noise1 || x1, "%s: bad argument (noise1 without the second plane)", fn);
  return MPGAN_OK;
}

// The tile of a launch over an extent of this depth, the forward's choice by measurement: 4 x 8 x 32 for
// volumes, 1 x 8 x 32 for depth 1.  go(T{}) launches with the tile T.
template <class Go>
static int warp_tile(int32_t depth, Go&& go) {
  if (depth > 1) return go(WarpTile3d{});
  return go(WarpTile2d{});
}

// The tiling of the output: dm and the number of tiles (= blocks).
template <class T>
static long warp_dims(int32_t n, const int32_t* in_dhw, const int32_t* out_dhw, WarpDims* dm) {
  for (int k = 0; k < 3; ++k) { dm->in[k] = in_dhw[k]; dm->out[k] = out_dhw[k]; }
  const long tW = (out_dhw[2] + T::TW - 1) / T::TW, tH = (out_dhw[1] + T::TH - 1) / T::TH,
             tD = (out_dhw[0] + T::TD - 1) / T::TD;
  dm->divTW = make_fastdiv((unsigned)tW);
  dm->divTH = make_fastdiv((unsigned)tH);
  dm->divTD = make_fastdiv((unsigned)tD);
  return (long)n * tD * tH * tW;                    // every tile holds an output voxel of its own: <= n * N_out < 2^31
}

extern "C" int mpgan_affine_warp(const float* x0, const float* x1, int32_t n, const int32_t* in_dhw,
                                 const int32_t* out_dhw, const double* theta, int32_t mode, float fill0, float fill1,
                                 const float* noise0, const float* noise1, const float* sigma, float* y0, float* y1,
                                 void* stream) {
  if (int rc = warp_forward_check("mpgan_affine_warp", x0, x1, n, in_dhw, out_dhw, theta, mode, noise0, noise1, sigma, y0, y1)) return rc;
  auto go = [&](auto tile) {
    using T = decltype(tile);
    WarpDims dm;
    const dim3 grid((unsigned)warp_dims<T>(n, in_dhw, out_dhw, &dm)), block(256);
    if (mode == MPGAN_WARP_BORDER)
      hipLaunchKernelGGL((affine_warp_kernel<T, true>), grid, block, 0, (hipStream_t)stream, x0, x1, dm, theta, fill0, fill1,
                         noise0, noise1, sigma, y0, y1);
    else
      hipLaunchKernelGGL((affine_warp_kernel<T, false>), grid, block, 0, (hipStream_t)stream, x0, x1, dm, theta, fill0, fill1,
                         noise0, noise1, sigma, y0, y1);
    return check_launch("mpgan_affine_warp");
  };
#ifdef MPGAN_DEV_SWITCHES
  if (const char* e = dev_env("MPGAN_DBG_WARP_TILE")) {
    switch (atoi(e)) {
      case 0: return go(WarpTile3d{});
      case 1: return go(WarpTile2d{});
      case 2: return go(WarpTileRow{});
      case 3: return go(WarpTileSq{});
      case 4: return go(WarpTileCube{});
      case 5: return go(WarpTileDeep{});
      case 6: return go(WarpTileWave{});
      case 7: return go(WarpTileWave4{});
      case 8: return go(WarpTileHalf{});
    }
    set_error("mpgan_affine_warp: unknown tile %s", e);
    return MPGAN_ERR_INVALID;
  }
#endif
  return warp_tile(out_dhw[0], go);
}

extern "C" int mpgan_affine_warp_backward(const float* gy, int32_t n, const int32_t* in_dhw, const int32_t* out_dhw,
                                          const double* theta, int32_t mode, float* gx, void* stream) {
  if (int rc = warp_check("mpgan_affine_warp_backward", gy && gx && theta, "gy / gx / theta", n, in_dhw, out_dhw, mode,
                          "backward (a clamped coordinate sends gradient from arbitrarily far away to the faces)"))
    return rc;
  return warp_tile(in_dhw[0], [&](auto tile) {
    WarpDims dm;                                    // the kernel reads the forward's output extent and tiles its input extent
    const dim3 grid((unsigned)warp_dims<decltype(tile)>(n, out_dhw, in_dhw, &dm)), block(256);
    hipLaunchKernelGGL((affine_warp_backward_kernel<decltype(tile)>), grid, block, 0, (hipStream_t)stream, gy, dm, theta, gx);
    return check_launch("mpgan_affine_warp_backward");
  });
}

// Bytes of the theta gradient's workspace: 12 doubles per forward tile (warp_tile's) of the n samples' outputs.
static int64_t warp_theta_bytes(int32_t n, const int32_t* out_dhw) {
  const long td = out_dhw[0] > 1 ? WarpTile3d::TD : WarpTile2d::TD;
  const long tiles = ((out_dhw[0] + td - 1) / td) * ((out_dhw[1] + WarpTile3d::TH - 1) / WarpTile3d::TH) *
                     ((out_dhw[2] + WarpTile3d::TW - 1) / WarpTile3d::TW);
  return (int64_t)n * tiles * 12 * (int64_t)sizeof(double);
}
static_assert(WarpTile3d::TH == WarpTile2d::TH && WarpTile3d::TW == WarpTile2d::TW, "one (h, w) tiling");

extern "C" int64_t mpgan_affine_warp_theta_workspace(int32_t n, const int32_t* out_dhw) {
  const char* fn = "mpgan_affine_warp_theta_workspace";
  long Nout;
  if (!out_dhw || n <= 0) {
    set_error("%s: bad argument (null out_dhw or n = %d)", fn, n);
    return -1;
  }
  if (element_count(fn, "output ", n, out_dhw, &Nout) != MPGAN_OK) return -1;
  return warp_theta_bytes(n, out_dhw);
}

extern "C" int mpgan_affine_warp_backward_theta(const float* x0, const float* x1, const float* gy0, const float* gy1,
                                                int32_t n, const int32_t* in_dhw, const int32_t* out_dhw,
                                                const double* theta, int32_t mode, float fill0, float fill1, void* ws,
                                                int64_t ws_bytes, double* gtheta, void* stream) {
  const char* fn = "mpgan_affine_warp_backward_theta";
  if (int rc = warp_check(fn, x0 && gy0 && theta && gtheta, "x0 / gy0 / theta / gtheta", n, in_dhw, out_dhw, mode,
                          "gradient in theta here (the clamp makes it a different function of c: not built)"))
    return rc;
  MPGAN_WARP_PAIR(fn, x1, gy1);
  const int64_t need = warp_theta_bytes(n, out_dhw);
  MPGAN_CHECK_ARG(ws != nullptr, "%s: bad argument (null workspace)", fn);
  MPGAN_CHECK_ARG(ws_bytes >= need, "%s: workspace of %lld bytes, needs %lld", fn, (long long)ws_bytes, (long long)need);
  MPGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "%s: workspace must be 8-byte aligned", fn);
  return warp_tile(out_dhw[0], [&](auto tile) {
    WarpDims dm;
    const long blocks = warp_dims<decltype(tile)>(n, in_dhw, out_dhw, &dm);
    hipLaunchKernelGGL((affine_warp_theta_tile_kernel<decltype(tile)>), dim3((unsigned)blocks), dim3(256), 0,
                       (hipStream_t)stream, x0, x1, gy0, gy1, dm, theta, fill0, fill1, static_cast<double*>(ws));
    if (int rc = check_launch(fn)) return rc;
    hipLaunchKernelGGL(affine_warp_theta_sum_kernel, dim3((unsigned)n * 12), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const double*>(ws), (int)(blocks / n), gtheta);
    return check_launch(fn);
  });
}

// The lattice rule of include/mpgan_hip.h over the output extent: extent 1 on an axis of extent 1, else 4 .. 64.
static int lattice_check(const char* what, const double* lattice, const int32_t* g, const int32_t* out_dhw) {
  if (!lattice) return MPGAN_OK;
  MPGAN_CHECK_ARG(g, "mpgan_deform_warp: bad argument (%s without its size triple)", what);
  for (int k = 0; k < 3; ++k) {
    if (out_dhw[k] == 1)
      MPGAN_CHECK_ARG(g[k] == 1, "mpgan_deform_warp: %s lattice %d x %d x %d: axis %d has output extent 1 and must have lattice extent 1",
                      what, g[0], g[1], g[2], k);
    else
      MPGAN_CHECK_ARG(g[k] >= 4 && g[k] <= kLatticeMax, "mpgan_deform_warp: %s lattice %d x %d x %d: axis %d must have an extent in [4, %d]",
                      what, g[0], g[1], g[2], k, kLatticeMax);
  }
  return MPGAN_OK;
}

template <class T, bool ROWS = true>
static int deform_launch(const float* x0, const float* x1, int32_t n, const int32_t* in_dhw, const int32_t* out_dhw,
                         const double* theta, const DeformArgs& df, int32_t mode, float fill0, float fill1,
                         const float* noise0, const float* noise1, const float* sigma, float* y0, float* y1,
                         void* stream) {
  WarpDims dm;
  const dim3 grid((unsigned)warp_dims<T>(n, in_dhw, out_dhw, &dm)), block(256);
  if (mode == MPGAN_WARP_BORDER)
    hipLaunchKernelGGL((deform_warp_kernel<T, true, ROWS>), grid, block, 0, (hipStream_t)stream, x0, x1, dm, theta, df, fill0,
                       fill1, noise0, noise1, sigma, y0, y1);
  else
    hipLaunchKernelGGL((deform_warp_kernel<T, false, ROWS>), grid, block, 0, (hipStream_t)stream, x0, x1, dm, theta, df, fill0,
                       fill1, noise0, noise1, sigma, y0, y1);
  return check_launch("mpgan_deform_warp");
}

extern "C" int mpgan_deform_warp(const float* x0, const float* x1, int32_t n, const int32_t* in_dhw,
                                 const int32_t* out_dhw, const double* theta, const double* ctrl,
                                 const int32_t* ctrl_dhw, const double* gain, const int32_t* gain_dhw,
                                 int32_t gain_planes, const double* gamma, double lo, double hi, int32_t mode,
                                 float fill0, float fill1, const float* noise0, const float* noise1,
                                 const float* sigma, float* y0, float* y1, void* stream) {
  if (int rc = warp_forward_check("mpgan_deform_warp", x0, x1, n, in_dhw, out_dhw, theta, mode, noise0, noise1, sigma, y0, y1)) return rc;
  if (int rc = lattice_check("ctrl", ctrl, ctrl_dhw, out_dhw)) return rc;
  if (int rc = lattice_check("gain", gain, gain_dhw, out_dhw)) return rc;
  MPGAN_CHECK_ARG(!(gain_planes & ~3), "mpgan_deform_warp: unknown gain_planes bits %#x (1 = plane 0, 2 = plane 1)", gain_planes);
  MPGAN_CHECK_ARG(!gain || gain_planes, "mpgan_deform_warp: bad argument (gain with gain_planes == 0)");
  MPGAN_CHECK_ARG(!(gain_planes & 2) || x1, "mpgan_deform_warp: bad argument (gain_planes names plane 1 without the second plane)");
  MPGAN_CHECK_ARG(!(gain || gamma) || hi > lo, "mpgan_deform_warp: bad argument (value range [%g, %g]: hi must exceed lo)", lo, hi);
  DeformArgs df;
  df.ctrl = ctrl;
  df.gain = gain;
  df.gamma = gamma;
  for (int k = 0; k < 3; ++k) { df.cg[k] = ctrl ? ctrl_dhw[k] : 1; df.gg[k] = gain ? gain_dhw[k] : 1; }
  df.gain_planes = gain ? gain_planes : 0;
  df.lo = lo;
  df.hi = hi;
  // a 1 x 8 x 32 tile whatever the depth: one d step per block needs no loop around the row lattices (the loop of the
  // 4 x 8 x 32 tile keeps the constants of pow and expm1 in registers across its barrier: 181 VGPRs against 70)
#ifdef MPGAN_DEV_SWITCHES
  // what else was measured: MPGAN_DBG_DEFORM_TILE=0 the 4 x 8 x 32 tile, MPGAN_DBG_DEFORM_FORM=1 the
  // 64-term sum per voxel instead of the row lattices
  if (const char* e = dev_env("MPGAN_DBG_DEFORM_TILE"))
    if (atoi(e) == 0)
      return deform_launch<WarpTile3d>(x0, x1, n, in_dhw, out_dhw, theta, df, mode, fill0, fill1, noise0, noise1, sigma, y0, y1, stream);
  if (const char* e = dev_env("MPGAN_DBG_DEFORM_FORM"))
    if (atoi(e) == 1)
      return deform_launch<WarpTile2d, false>(x0, x1, n, in_dhw, out_dhw, theta, df, mode, fill0, fill1, noise0, noise1, sigma, y0, y1, stream);
#endif
  return deform_launch<WarpTile2d>(x0, x1, n, in_dhw, out_dhw, theta, df, mode, fill0, fill1, noise0, noise1, sigma, y0, y1, stream);
}
