// SSIM, the metric and the differentiable loss (include/mpgan_hip.h: "SSIM loss" states the definition and the
// closed-form gradient; the metric is skimage.metrics.structural_similarity as psnr_ssim_metric.py:91-92 calls it:
// 7-wide uniform window, 7x7 for a slice and 7x7x7 for a volume, K1 = 0.01, K2 = 0.03, sample covariance NP/(NP-1),
// mean of S over the interior that excludes the 3 border samples per windowed axis).  Two kernels of its own, the
// metric's one-block tail and the shared loss tail, no floating-point atomics, no scatter; every sum is taken in a fixed order in fp64 (reduce.h):
//
//   sl_forward_kernel   THE SSIM forward, of the metric too: a block stages the (TZ+WZ-1) x 14 x 38 region of both
//                       images of ONE item in LDS, a thread owns one (y, x) column of the 8 x 32 tile, forms the 7x7
//                       plane sums of (a, b, a^2, b^2, ab) of every staged z once in double (sums of 343 products of
//                       0..255 values would cost fp32 its variance digits) and adds them to the windows that hold the
//                       plane (the z slide).  The sums are taken over the raw samples and shifted by `lo` once per
//                       window, in double (exactly what a per-sample x - lo in double gives, to 1e-14; with lo = 0,
//                       the metric, the shift adds and subtracts exact zeros).  When a gradient is wanted the same pass
//                       writes the per-window coefficient maps Q, R and P of each differentiated image, as doubles
//                       (see "storage" below).  Block partial -> workspace slot.
//   ssim_final_kernel   mpgan_ssim's tail: one block adds the one item's tile partials in slot order + a fixed tree
//                       and rounds the mean to fp32.
//   launch_loss_tail    (loss_ops.hip) loss_item_kernel, one block per item: its tiles' partials in slot order + a fixed
//                       tree -> ssim_item (double); loss_reduce_kernel<true>: loss = 1 - ssim over the items in item
//                       order: mean, sum, or per batch entry over its channels.
//   sl_backward_kernel  a gather: an output voxel box-sums each map over the windows that contain it (the map is zero
//                       outside the M valid corners).  One map at a time goes through one LDS buffer with a 6-sample
//                       halo in front of the tile on every windowed axis; per staged z a thread forms the 7x7 plane
//                       sum once and slides the z window, then folds the map in: g = sum P + a_p sum Q + b_p sum R.
//
// Storage of the maps: P holds -ux Q - uy R, so sum P + a_p sum Q + b_p sum R cancels wherever a voxel sits at its
// windows' means (flat regions: |sum Q (a_p - ux)| is zero while |a_p sum Q| is ~1e5 at data range 2).  With fp32 maps
// the rounding of P (2^-24 * 1e5) would be the gradient's error, three orders above what fp32 arithmetic on the
// centred product costs.  The maps are therefore doubles: 24 B per window and image for one gradient, 32 B for both
// (about 200 MB at 4 x 1 x 128^3), and the backward's box sums run in double too; only the final product with the
// upstream gradient is rounded to fp32.
//
// The foreground-weighted form (include/mpgan_hip.h: "masked SSIM") is the same two kernels under one more
// template parameter: a valid window carries a weight w in {0, 1} read at its centre voxel -- a byte of the mask
// (SL_MASK), or the staged b against the item's threshold, out of LDS (SL_THR).  The forward adds w S to the block's
// partial and w to a second, integer partial, stores w Q, w R, w P (exact: zero or the value, so the backward's box
// sums are those of the plain form) and can write S itself as an fp32 map; launch_counted_loss_tail (loss_ops.hip) turns
// the two partial sets into stats[item] = (ssim_item, n_item) and the loss; the backward reads its per-item factor
// scale / (n n_item) from stats on the device.  SL_PLAIN is the code of the plain entry points, bit for bit: the
// weighted fields live in a derived parameter struct that the plain instances never see.
#include "mpgan_common.h"

namespace mpgan {

constexpr int SL_W = 7, SL_TY = 8, SL_TX = 32, SL_RY = SL_TY + SL_W - 1, SL_RX = SL_TX + SL_W - 1;
constexpr int SL_TZ3 = 4;                       // z tile of the 3-D forms (forward: window corners, backward: voxels)
constexpr int SL_PLANE = SL_RY * SL_RX;

constexpr int SL_PLAIN = 0, SL_MASK = 1, SL_THR = 2;      // where a window's weight comes from

struct SlFwd {
  const float* a;
  const float* b;
  int D, H, W, tiles_x, tiles_y;
  long tiles;                                   // per item
  double lo, c1, c2;
  double* partials;                             // [items][tiles]
  double* q;                                    // [items][M] each, or null
  double* r;
  double* pa;
  double* pb;
};

struct SlFwdW : SlFwd {                         // the weighted instances' additions
  const uint8_t* mask;                          // SL_MASK: [items][D][H][W], or null for w = 1 everywhere
  const float* thr;                             // SL_THR: [items]
  long long* counts;                            // [items][tiles]: the block's number of weighted windows
  float* smap;                                  // [items][M]: S of every valid window, or null
};

// The parameter struct of an instance, by specialisation: the kernels' mangled names then hold the template arguments
// alone (an expression over a constant in the signature is mangled with the constant's type and name, and the host
// and the device pass number an unnamed type differently -- the runtime then finds no such kernel).
template <int MODE> struct SlFwdOf { using type = SlFwdW; };
template <> struct SlFwdOf<SL_PLAIN> { using type = SlFwd; };

template <int WZ, int TZ, int MODE>
__global__ __launch_bounds__(256) void sl_forward_kernel(typename SlFwdOf<MODE>::type p) {
  constexpr int RZ = TZ + WZ - 1;
  extern __shared__ float sl_sm[];              // [2][RZ][SL_RY][SL_RX]
  __shared__ double red[256];
  float* sa = sl_sm;
  float* sb = sl_sm + RZ * SL_PLANE;
  const int tid = threadIdx.x;
  const long item = blockIdx.y;
  const long vox = (long)p.D * p.H * p.W;
  const float* a = p.a + item * vox;
  const float* b = p.b + item * vox;
  const int bx = blockIdx.x % p.tiles_x;
  const int by = (blockIdx.x / p.tiles_x) % p.tiles_y;
  const int bz = blockIdx.x / (p.tiles_x * p.tiles_y);
  const int z0 = bz * TZ, y0 = by * SL_TY, x0 = bx * SL_TX;   // origin of the tile = first window corner
  for (int i = tid; i < RZ * SL_PLANE; i += 256) {
    const int rx = i % SL_RX, ry = (i / SL_RX) % SL_RY, rz = i / SL_PLANE;
    const int z = z0 + rz, y = y0 + ry, x = x0 + rx;
    const bool ok = z < p.D && y < p.H && x < p.W;
    const long off = ((long)z * p.H + y) * p.W + x;
    sa[i] = ok ? a[off] : 0.f;
    sb[i] = ok ? b[off] : 0.f;
  }
  __syncthreads();
  const int tx = tid % SL_TX, ty = tid / SL_TX;
  const int OD = p.D - WZ + 1, OH = p.H - SL_W + 1, OW = p.W - SL_W + 1;   // window corners
  // the weights of this column's TZ windows as one bit each, read at the centre voxel (corner + 3 on every windowed
  // axis) ahead of the plane sums, which hide the mask bytes' latency; the scheduling barrier keeps the plane loop below
  // what it is in the plain form
  unsigned wbits = 0;
  if constexpr (MODE != SL_PLAIN) {
    constexpr int CZ = WZ / 2, CYX = SL_W / 2;
    float thr = 0.f;
    if constexpr (MODE == SL_THR) thr = p.thr[item];
#pragma unroll
    for (int zo = 0; zo < TZ; ++zo) {
      const int cz = z0 + zo, cy = y0 + ty, cx = x0 + tx;
      bool w = cz < OD && cy < OH && cx < OW;
      if constexpr (MODE == SL_MASK) {
        if (w && p.mask) w = p.mask[item * vox + ((long)(cz + CZ) * p.H + cy + CYX) * p.W + cx + CYX] != 0;
      } else {                                  // the staged b: strict, in fp32, false for a NaN on either side
        w = w && sb[((zo + CZ) * SL_RY + ty + CYX) * SL_RX + tx + CYX] > thr;
      }
      wbits |= (unsigned)w << zo;
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  // window sums of the TZ corners of this column; a plane's five sums are formed once and added to every window
  // that holds the plane (in plane order), so that only 5 TZ doubles stay live across the planes
  double wa[TZ], wb[TZ], waa[TZ], wbb[TZ], wab[TZ];
#pragma unroll
  for (int zo = 0; zo < TZ; ++zo) wa[zo] = wb[zo] = waa[zo] = wbb[zo] = wab[zo] = 0.0;
#pragma unroll 1                                // a rolled loop: unrolled, the planes' LDS reads are hoisted and spill
  for (int rz = 0; rz < RZ; ++rz) {
    double s_a = 0, s_b = 0, s_aa = 0, s_bb = 0, s_ab = 0;
    for (int dy = 0; dy < SL_W; ++dy) {
      const float* ra = sa + (rz * SL_RY + ty + dy) * SL_RX + tx;
      const float* rb = sb + (rz * SL_RY + ty + dy) * SL_RX + tx;
#pragma unroll
      for (int dx = 0; dx < SL_W; ++dx) {
        const double u = (double)ra[dx], v = (double)rb[dx];
        s_a += u; s_b += v;
        s_aa = fma(u, u, s_aa); s_bb = fma(v, v, s_bb); s_ab = fma(u, v, s_ab);
      }
    }
#pragma unroll
    for (int zo = 0; zo < TZ; ++zo) {
      const bool in = zo <= rz && rz < zo + WZ;
      wa[zo] += in ? s_a : 0.0; wb[zo] += in ? s_b : 0.0;
      waa[zo] += in ? s_aa : 0.0; wbb[zo] += in ? s_bb : 0.0; wab[zo] += in ? s_ab : 0.0;
    }
  }
  constexpr double NP = (double)(WZ * SL_W * SL_W);
  constexpr double cn = NP / (NP - 1.0);
  const double lo = p.lo, klo = NP * lo * lo;
  const long M = (long)OD * OH * OW;
  double local = 0.0;
#pragma unroll
  for (int zo = 0; zo < TZ; ++zo) {
    const int cz = z0 + zo, cy = y0 + ty, cx = x0 + tx;
    if (cz >= OD || cy >= OH || cx >= OW) continue;
    const bool w = MODE == SL_PLAIN || ((wbits >> zo) & 1u);
    double s_a = wa[zo], s_b = wb[zo], s_aa = waa[zo], s_bb = wbb[zo], s_ab = wab[zo];
    // sums of the shifted samples x - lo from the sums of the raw ones (the three second moments by one expression,
    // so that identical images keep vx == vy == vxy bit for bit)
    s_aa = s_aa - lo * (s_a + s_a) + klo;
    s_bb = s_bb - lo * (s_b + s_b) + klo;
    s_ab = s_ab - lo * (s_a + s_b) + klo;
    s_a -= NP * lo;
    s_b -= NP * lo;
    const double ux = s_a / NP, uy = s_b / NP;
    const double vx = cn * (s_aa / NP - ux * ux), vy = cn * (s_bb / NP - uy * uy);
    const double vxy = cn * (s_ab / NP - ux * uy);
    const double A1 = 2.0 * ux * uy + p.c1, A2 = 2.0 * vxy + p.c2;
    const double B1 = ux * ux + uy * uy + p.c1, B2 = vx + vy + p.c2;
    const double S = (A1 * A2) / (B1 * B2);
    if constexpr (MODE == SL_PLAIN) {
      local += S;
    } else {
      local += w ? S : 0.0;
      if (p.smap) p.smap[item * M + ((long)cz * OH + cy) * OW + cx] = (float)S;
    }
    if (p.q) {
      const double inv = 1.0 / (B1 * B2);       // 1/B1 = B2 inv, 1/B2 = B1 inv
      const double Q = -2.0 * cn * S * (B1 * inv);
      const double R = 2.0 * cn * A1 * inv;
      const long o = item * M + ((long)cz * OH + cy) * OW + cx;
      p.q[o] = w ? Q : 0.0;                     // w is the constant true in the plain form
      p.r[o] = w ? R : 0.0;
      if (p.pa) p.pa[o] = w ? 2.0 * uy * A2 * inv - 2.0 * ux * S * (B2 * inv) - ux * Q - uy * R : 0.0;
      if (p.pb) p.pb[o] = w ? 2.0 * ux * A2 * inv - 2.0 * uy * S * (B2 * inv) - uy * Q - ux * R : 0.0;
    }
    __builtin_amdgcn_sched_barrier(0);          // one window's divisions at a time
  }
  local = block_tree_sum<256>(local, red);      // block sum in a fixed order
  if (tid == 0) p.partials[item * p.tiles + blockIdx.x] = local;
  if constexpr (MODE != SL_PLAIN) {
    __shared__ unsigned cnt4[4];
    const unsigned c = block_sum4((unsigned)__popc(wbits), cnt4);      // integers: no order to fix
    if (tid == 0) p.counts[item * p.tiles + blockIdx.x] = (long long)c;
  }
}

struct SlBwd {
  const float* x;                               // the image the gradient is for
  const float* y;                               // the other image
  int D, H, W, OD, OH, OW, tiles_x, tiles_y;
  const double* p;                              // [items][M]: P of the differentiated image, Q, R
  const double* q;
  const double* r;
  double lo, scale;                             // scale = reduction factor / (n M)
  const float* upstream;
  int up_stride, channels;
  float* grad;
};

struct SlBwdW : SlBwd {                         // weighted: scale = reduction factor / n, the item's divisor from stats
  const double* stats;                          // [items][2] = (ssim_item, n_item)
};

template <bool WEIGHTED> struct SlBwdOf { using type = SlBwdW; };
template <> struct SlBwdOf<false> { using type = SlBwd; };

template <int WZ, int TZ, bool WEIGHTED>
__global__ __launch_bounds__(256) void sl_backward_kernel(typename SlBwdOf<WEIGHTED>::type p) {
  constexpr int RZ = TZ + WZ - 1;
  extern __shared__ double sl_sd[];             // [RZ][SL_RY][SL_RX]: one map's corners, zero outside the valid ones
  const int tid = threadIdx.x;
  const long item = blockIdx.y;
  const long vox = (long)p.D * p.H * p.W, M = (long)p.OD * p.OH * p.OW;
  const int bx = blockIdx.x % p.tiles_x;
  const int by = (blockIdx.x / p.tiles_x) % p.tiles_y;
  const int bz = blockIdx.x / (p.tiles_x * p.tiles_y);
  const int z0 = bz * TZ, y0 = by * SL_TY, x0 = bx * SL_TX;   // origin of the tile = first output voxel
  const int tx = tid % SL_TX, ty = tid / SL_TX;
  const int vy = y0 + ty, vx = x0 + tx;
  const bool col_ok = vy < p.H && vx < p.W;
  const float* x = p.x + item * vox;
  const float* y = p.y + item * vox;
  double item_scale = p.scale;
  if constexpr (WEIGHTED) {
    const double n_item = p.stats[2 * item + 1];
    if (!(n_item > 0.0)) {                      // an empty item: exactly zero, whatever the upstream (block-uniform)
      float* out = p.grad + item * vox;
      for (int zo = 0; zo < TZ; ++zo)
        if (col_ok && z0 + zo < p.D) out[((long)(z0 + zo) * p.H + vy) * p.W + vx] = 0.f;
      return;
    }
    item_scale = p.scale / n_item;
  }
  double xv[TZ], yv[TZ], acc[TZ];
#pragma unroll
  for (int zo = 0; zo < TZ; ++zo) {
    const bool ok = col_ok && z0 + zo < p.D;
    const long off = ((long)(z0 + zo) * p.H + vy) * p.W + vx;
    xv[zo] = ok ? (double)x[off] - p.lo : 0.0;
    yv[zo] = ok ? (double)y[off] - p.lo : 0.0;
    acc[zo] = 0.0;
  }
#pragma unroll 1
  for (int m = 0; m < 3; ++m) {
    const double* src = (m == 0 ? p.p : (m == 1 ? p.q : p.r)) + item * M;
    if (m) __syncthreads();
    for (int i = tid; i < RZ * SL_PLANE; i += 256) {
      const int rx = i % SL_RX, ry = (i / SL_RX) % SL_RY, rz = i / SL_PLANE;
      const int cz = z0 - (WZ - 1) + rz, cy = y0 - (SL_W - 1) + ry, cx = x0 - (SL_W - 1) + rx;
      const bool ok = cz >= 0 && cz < p.OD && cy >= 0 && cy < p.OH && cx >= 0 && cx < p.OW;
      sl_sd[i] = ok ? src[((long)cz * p.OH + cy) * p.OW + cx] : 0.0;
    }
    __syncthreads();
    double ps[RZ];
#pragma unroll
    for (int rz = 0; rz < RZ; ++rz) {
      double s = 0.0;
      for (int dy = 0; dy < SL_W; ++dy) {
        const double* row = sl_sd + (rz * SL_RY + ty + dy) * SL_RX + tx;
#pragma unroll
        for (int dx = 0; dx < SL_W; ++dx) s += row[dx];
      }
      ps[rz] = s;
    }
#pragma unroll
    for (int zo = 0; zo < TZ; ++zo) {
      double g = 0.0;
#pragma unroll
      for (int dz = 0; dz < WZ; ++dz) g += ps[zo + dz];
      acc[zo] = m == 0 ? g : fma(m == 1 ? xv[zo] : yv[zo], g, acc[zo]);
    }
  }
  const double up = (double)p.upstream[(item / p.channels) * p.up_stride] * item_scale;
  float* out = p.grad + item * vox;
#pragma unroll
  for (int zo = 0; zo < TZ; ++zo) {
    if (!col_ok || z0 + zo >= p.D) continue;
    out[((long)(z0 + zo) * p.H + vy) * p.W + vx] = (float)(up * acc[zo]);
  }
}

struct SlGeom {
  bool vol;
  int D, H, W, OD, OH, OW;
  long M, vox;
  long fwd_tiles, bwd_tiles;
  int fwd_tx, fwd_ty, bwd_tx, bwd_ty;
};

// The ONE place the tiling of both launches is decided: extents (D >= 1, H and W >= 7) -> *g.  A depth below 7 tiles as
// that many slices (which is what mpgan_ssim_workspace sizes a depth of 2..6 by; the launches refuse it).
static void sl_tiling(const int32_t* dhw, SlGeom* g) {
  g->vol = dhw[0] >= SL_W;
  g->D = dhw[0]; g->H = dhw[1]; g->W = dhw[2];
  g->OD = g->vol ? g->D - SL_W + 1 : g->D; g->OH = g->H - SL_W + 1; g->OW = g->W - SL_W + 1;
  g->M = (long)g->OD * g->OH * g->OW;
  g->vox = (long)g->D * g->H * g->W;
  const int tz = g->vol ? SL_TZ3 : 1;
  g->fwd_tx = (g->OW + SL_TX - 1) / SL_TX; g->fwd_ty = (g->OH + SL_TY - 1) / SL_TY;
  g->fwd_tiles = (long)((g->OD + tz - 1) / tz) * g->fwd_ty * g->fwd_tx;
  g->bwd_tx = (g->W + SL_TX - 1) / SL_TX; g->bwd_ty = (g->H + SL_TY - 1) / SL_TY;
  g->bwd_tiles = (long)((g->D + tz - 1) / tz) * g->bwd_ty * g->bwd_tx;
}

static bool sl_extents_ok(const int32_t* dhw) { return dhw && dhw[0] >= 1 && dhw[1] >= SL_W && dhw[2] >= SL_W; }

// Every launch's geometry checks, then the tiling.  Status as the entry points return it; *g is valid on MPGAN_OK alone.
static int sl_geometry(const char* who, const int32_t* dhw, int32_t items, SlGeom* g) {
  MPGAN_CHECK_ARG(dhw != nullptr, "%s: null dhw", who);
  MPGAN_CHECK_ARG(items >= 1 && items <= 65535, "%s: %d items outside [1, 65535]", who, items);
  MPGAN_CHECK_ARG(sl_extents_ok(dhw), "%s: extents (%d, %d, %d) below the 7-wide window", who, dhw[0], dhw[1], dhw[2]);
  MPGAN_UNSUPPORTED(dhw[0] > 1 && dhw[0] < SL_W, "%s: depth %d is neither a slice (1) nor >= 7", who, dhw[0]);
  sl_tiling(dhw, g);
  MPGAN_CHECK_ARG(g->fwd_tiles < (1L << 31) && g->bwd_tiles < (1L << 31), "%s: too many tiles", who);
  return MPGAN_OK;
}

static int sl_maps(int grad_mask) { return grad_mask == 0 ? 0 : (grad_mask == 3 ? 4 : 3); }

// What a weighted call has beyond a plain one (the plain entry points pass null).
struct SlWeights {
  const uint8_t* mask;
  const float* thr;
  double* stats;                                // [items][2]
  float* smap;                                  // nullable
};

// Workspace: [items][tiles] partials, then (weighted) [items][tiles] int64 counts, then [items] of the loss tail.
static int64_t sl_workspace(const char* who, const int32_t* dhw, int32_t items, int32_t grad_mask, bool weighted,
                            int64_t* coef_bytes) {
  SlGeom g;
  if (grad_mask < 0 || grad_mask > 3 || sl_geometry(who, dhw, items, &g) != MPGAN_OK) return -1;
  if (coef_bytes) *coef_bytes = (int64_t)sl_maps(grad_mask) * items * g.M * (int64_t)sizeof(double);
  return ((int64_t)items * g.fwd_tiles * (weighted ? 2 : 1) + items) * (int64_t)sizeof(double);
}

template <int MODE, typename P>
static void sl_launch_forward(const SlGeom& g, int32_t items, const P& p, hipStream_t st) {
  const dim3 grid((unsigned)g.fwd_tiles, (unsigned)items);
  if (g.vol) {
    const size_t smem = 2ul * (SL_TZ3 + SL_W - 1) * SL_PLANE * sizeof(float);
    hipLaunchKernelGGL((sl_forward_kernel<SL_W, SL_TZ3, MODE>), grid, dim3(256), smem, st, p);
  } else {
    const size_t smem = 2ul * SL_PLANE * sizeof(float);
    hipLaunchKernelGGL((sl_forward_kernel<1, 1, MODE>), grid, dim3(256), smem, st, p);
  }
}

template <bool WEIGHTED, typename P>
static void sl_launch_backward(const SlGeom& g, int32_t items, const P& p, hipStream_t st) {
  const dim3 grid((unsigned)g.bwd_tiles, (unsigned)items);
  if (g.vol) {
    const size_t smem = (size_t)(SL_TZ3 + SL_W - 1) * SL_PLANE * sizeof(double);
    hipLaunchKernelGGL((sl_backward_kernel<SL_W, SL_TZ3, WEIGHTED>), grid, dim3(256), smem, st, p);
  } else {
    const size_t smem = (size_t)SL_PLANE * sizeof(double);
    hipLaunchKernelGGL((sl_backward_kernel<1, 1, WEIGHTED>), grid, dim3(256), smem, st, p);
  }
}

// What every forward launch reads: the images, the tiling, lo and the two constants of the data range L; no maps.
static void sl_forward_params(SlFwd* p, const float* a, const float* b, const SlGeom& g, double lo, double L,
                              void* workspace) {
  p->a = a; p->b = b; p->D = g.D; p->H = g.H; p->W = g.W;
  p->tiles_x = g.fwd_tx; p->tiles_y = g.fwd_ty; p->tiles = g.fwd_tiles;
  p->lo = lo; p->c1 = (0.01 * L) * (0.01 * L); p->c2 = (0.03 * L) * (0.03 * L);
  p->partials = static_cast<double*>(workspace);
  p->q = p->r = p->pa = p->pb = nullptr;
}

// Both forward entry points of the loss: every check, then the launches.  wt == null is the plain form.
static int sl_forward(const char* who, const float* a, const float* b, const int32_t* dhw, int32_t items,
                      int32_t channels, double lo, double hi, int32_t grad_mask, void* workspace,
                      int64_t workspace_bytes, void* coef, int64_t coef_bytes, int32_t reduction, float* loss,
                      void* stream, const SlWeights* wt) {
  MPGAN_CHECK_ARG(a && b && loss && (!wt || wt->stats), "%s: null pointer", who);
  MPGAN_CHECK_ARG(!wt || !(wt->mask && wt->thr), "%s: at most one of mask and thr may be given (got both)", who);
  SlGeom g;
  if (int rc = sl_geometry(who, dhw, items, &g)) return rc;
  if (int rc = check_items(who, items, channels)) return rc;
  MPGAN_CHECK_ARG(hi - lo > 0.0 && is_finite(hi - lo), "%s: value range needs finite hi > lo", who);
  MPGAN_CHECK_ARG(grad_mask >= 0 && grad_mask <= 3, "%s: grad_mask %d outside [0, 3]", who, grad_mask);
  if (int rc = check_reduction(who, reduction)) return rc;
  int64_t need_coef = 0;
  if (int rc = check_workspace(who, workspace, workspace_bytes,
                               sl_workspace(who, dhw, items, grad_mask, wt != nullptr, &need_coef)))
    return rc;
  MPGAN_CHECK_ARG(grad_mask == 0 || (coef && coef_bytes >= need_coef), "%s: coef missing or too small", who);
  MPGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(coef) & 7) == 0, "%s: coef must be 8-byte aligned", who);
  MPGAN_CHECK_ARG(!wt || ((reinterpret_cast<uintptr_t>(wt->stats) & 7) == 0 &&
                          (reinterpret_cast<uintptr_t>(wt->smap) & 3) == 0),
                  "%s: stats must be 8-byte and smap 4-byte aligned", who);
  SlFwdW p;
  sl_forward_params(&p, a, b, g, lo, hi - lo, workspace);
  const long slots = (long)items * g.fwd_tiles;
  double* ssim_item = p.partials + slots * (wt ? 2 : 1);
  double* maps = static_cast<double*>(coef);
  const long per_map = (long)items * g.M;
  p.q = grad_mask ? maps : nullptr;
  p.r = grad_mask ? maps + per_map : nullptr;
  p.pa = (grad_mask & 1) ? maps + 2 * per_map : nullptr;
  p.pb = (grad_mask & 2) ? maps + (grad_mask == 3 ? 3 : 2) * per_map : nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (!wt) {
    sl_launch_forward<SL_PLAIN>(g, items, static_cast<const SlFwd&>(p), st);
    // ssim_item = (sum of the item's tile partials) / M; loss = 1 - ssim over the items
    launch_loss_tail(p.partials, g.fwd_tiles, 1.0 / (double)g.M, ssim_item, items, channels, reduction, true, loss, st);
    return check_launch(who);
  }
  p.mask = wt->mask; p.thr = wt->thr; p.smap = wt->smap;
  p.counts = reinterpret_cast<long long*>(p.partials + slots);
  if (wt->thr) sl_launch_forward<SL_THR>(g, items, p, st);
  else sl_launch_forward<SL_MASK>(g, items, p, st);       // a null mask: every window weighs 1
  // stats[item] = (sum w S / n_item, n_item); loss = 1 - ssim over the items, an empty item adding 0
  launch_counted_loss_tail(p.partials, p.counts, g.fwd_tiles, ssim_item, wt->stats, items, channels, reduction, loss, st);
  return check_launch(who);
}

// Both backward entry points; stats == null is the plain form.
static int sl_backward(const char* who, const float* a, const float* b, const int32_t* dhw, int32_t items,
                       int32_t channels, double lo, int32_t grad_mask, const void* coef, int64_t coef_bytes,
                       const double* stats, const float* upstream, int32_t upstream_stride, double scale, int32_t wrt,
                       float* grad, void* stream) {
  MPGAN_CHECK_ARG(a && b && coef && upstream && grad, "%s: null pointer", who);
  SlGeom g;
  if (int rc = sl_geometry(who, dhw, items, &g)) return rc;
  if (int rc = check_items(who, items, channels)) return rc;
  if (int rc = check_wrt(who, wrt)) return rc;
  if (int rc = check_upstream_stride(who, upstream_stride)) return rc;
  if (int rc = check_scale(who, scale)) return rc;
  MPGAN_CHECK_ARG(is_finite(lo), "%s: non-finite lo", who);
  MPGAN_CHECK_ARG(grad_mask >= 1 && grad_mask <= 3 && ((grad_mask >> wrt) & 1),
                  "%s: the forward's grad_mask %d holds no maps for wrt %d", who, grad_mask, wrt);
  const long per_map = (long)items * g.M;
  MPGAN_CHECK_ARG(coef_bytes >= (int64_t)sl_maps(grad_mask) * per_map * (int64_t)sizeof(double), "%s: coef too small",
                  who);
  MPGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(coef) & 7) == 0 && (reinterpret_cast<uintptr_t>(stats) & 7) == 0,
                  "%s: coef must be 8-byte aligned", who);
  const double* maps = static_cast<const double*>(coef);
  SlBwdW p;
  p.x = wrt == 0 ? a : b;
  p.y = wrt == 0 ? b : a;
  p.D = g.D; p.H = g.H; p.W = g.W; p.OD = g.OD; p.OH = g.OH; p.OW = g.OW;
  p.tiles_x = g.bwd_tx; p.tiles_y = g.bwd_ty;
  p.q = maps;
  p.r = maps + per_map;
  p.p = maps + (wrt == 1 && grad_mask == 3 ? 3 : 2) * per_map;
  const double np = g.vol ? 343.0 : 49.0;
  p.lo = lo; p.scale = stats ? scale / np : scale / (np * (double)g.M);
  p.upstream = upstream; p.up_stride = upstream_stride; p.channels = channels;
  p.grad = grad;
  p.stats = stats;
  hipStream_t st = (hipStream_t)stream;
  if (stats) sl_launch_backward<true>(g, items, p, st);
  else sl_launch_backward<false>(g, items, static_cast<const SlBwd&>(p), st);
  return check_launch(who);
}

// The metric's tail: the mean of S over the one item's windows, rounded to fp32.
__global__ __launch_bounds__(256) void ssim_final_kernel(const double* __restrict__ partials, int nb, double inv_count,
                                                         float* __restrict__ out1) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) s += partials[i];
  s = block_tree_sum<256>(s, red);
  if (threadIdx.x == 0) out1[0] = (float)(s * inv_count);
}

}  // namespace mpgan

using namespace mpgan;

// One double per tile of the forward; a query: it leaves the last error alone.
extern "C" int64_t mpgan_ssim_workspace(const int32_t* dhw) {
  if (!sl_extents_ok(dhw)) return -1;
  SlGeom g;
  sl_tiling(dhw, &g);
  return g.fwd_tiles * (int64_t)sizeof(double);
}

// The plain forward over one item with lo = 0 and hi = data_range, no maps, then the metric's own tail.
extern "C" int mpgan_ssim(const float* a, const float* b, const int32_t* dhw, float data_range, void* workspace,
                          int64_t workspace_bytes, float* out1, void* stream) {
  MPGAN_CHECK_ARG(a && b && workspace && out1, "ssim: null pointer");
  SlGeom g;
  if (int rc = sl_geometry("ssim", dhw, 1, &g)) return rc;
  MPGAN_CHECK_ARG(workspace_bytes >= g.fwd_tiles * (int64_t)sizeof(double), "ssim: workspace too small");
  SlFwd p;
  sl_forward_params(&p, a, b, g, 0.0, (double)data_range, workspace);
  hipStream_t st = (hipStream_t)stream;
  sl_launch_forward<SL_PLAIN>(g, 1, p, st);
  hipLaunchKernelGGL(ssim_final_kernel, dim3(1), dim3(256), 0, st, (const double*)p.partials, (int)g.fwd_tiles,
                     1.0 / (double)g.M, out1);
  return check_launch("ssim");
}

extern "C" int64_t mpgan_ssim_loss_workspace(const int32_t* dhw, int32_t items, int32_t grad_mask,
                                             int64_t* coef_bytes) {
  return sl_workspace("ssim_loss_workspace", dhw, items, grad_mask, false, coef_bytes);
}

extern "C" int mpgan_ssim_loss_forward(const float* a, const float* b, const int32_t* dhw, int32_t items,
                                       int32_t channels, double lo, double hi, int32_t grad_mask, void* workspace,
                                       int64_t workspace_bytes, void* coef, int64_t coef_bytes, int32_t reduction,
                                       float* loss, void* stream) {
  return sl_forward("ssim_loss_forward", a, b, dhw, items, channels, lo, hi, grad_mask, workspace, workspace_bytes, coef,
                    coef_bytes, reduction, loss, stream, nullptr);
}

extern "C" int mpgan_ssim_loss_backward(const float* a, const float* b, const int32_t* dhw, int32_t items,
                                        int32_t channels, double lo, int32_t grad_mask, const void* coef,
                                        int64_t coef_bytes, const float* upstream, int32_t upstream_stride,
                                        double scale, int32_t wrt, float* grad, void* stream) {
  return sl_backward("ssim_loss_backward", a, b, dhw, items, channels, lo, grad_mask, coef, coef_bytes, nullptr,
                     upstream, upstream_stride, scale, wrt, grad, stream);
}

extern "C" int64_t mpgan_masked_ssim_loss_workspace(const int32_t* dhw, int32_t items, int32_t grad_mask,
                                                    int64_t* coef_bytes) {
  return sl_workspace("masked_ssim_loss_workspace", dhw, items, grad_mask, true, coef_bytes);
}

extern "C" int mpgan_masked_ssim_loss_forward(const float* a, const float* b, const int32_t* dhw, int32_t items,
                                              int32_t channels, double lo, double hi, const uint8_t* mask,
                                              const float* thr, int32_t grad_mask, void* workspace,
                                              int64_t workspace_bytes, void* coef, int64_t coef_bytes, double* stats,
                                              float* smap, int32_t reduction, float* loss, void* stream) {
  const SlWeights wt = {mask, thr, stats, smap};
  return sl_forward("masked_ssim_loss_forward", a, b, dhw, items, channels, lo, hi, grad_mask, workspace,
                    workspace_bytes, coef, coef_bytes, reduction, loss, stream, &wt);
}

extern "C" int mpgan_masked_ssim_loss_backward(const float* a, const float* b, const int32_t* dhw, int32_t items,
                                               int32_t channels, double lo, int32_t grad_mask, const void* coef,
                                               int64_t coef_bytes, const double* stats, const float* upstream,
                                               int32_t upstream_stride, double scale, int32_t wrt, float* grad,
                                               void* stream) {
  MPGAN_CHECK_ARG(stats, "masked_ssim_loss_backward: null pointer");
  return sl_backward("masked_ssim_loss_backward", a, b, dhw, items, channels, lo, grad_mask, coef, coef_bytes, stats,
                     upstream, upstream_stride, scale, wrt, grad, stream);
}
