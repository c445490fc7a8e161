// Differentiable SSIM loss (include/mpgan_hip.h: "SSIM loss" states the definition and the closed-form gradient).
// Two kernels of its own and the shared loss tail, no floating-point atomics, no scatter; every sum is taken in a
// fixed order in fp64 (reduce.h):
//
//   sl_forward_kernel   the pattern of ssim_partial_kernel (metric_ops.hip): a block stages the (TZ+WZ-1) x 14 x 38
//                       region of both images of ONE item in LDS, a thread owns one (y, x) column of the 8 x 32 tile,
//                       forms the 7x7 plane sums of (a, b, a^2, b^2, ab) of every staged z once in double and adds
//                       them to the windows that hold the plane (the z slide).  The sums are taken over the raw samples and shifted by `lo` once per
//                       window, in double (exactly what a per-sample x - lo in double gives, to 1e-14).  When a
//                       gradient is wanted the same pass writes the per-window coefficient maps Q, R and P of each
//                       differentiated image, as doubles (see "storage" below).  Block partial -> workspace slot.
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
#include "mpgan_common.h"

namespace mpgan {

constexpr int SL_W = 7, SL_TY = 8, SL_TX = 32, SL_RY = SL_TY + SL_W - 1, SL_RX = SL_TX + SL_W - 1;
constexpr int SL_TZ3 = 4;                       // z tile of the 3-D forms (forward: window corners, backward: voxels)
constexpr int SL_PLANE = SL_RY * SL_RX;

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

template <int WZ, int TZ>
__global__ __launch_bounds__(256) void sl_forward_kernel(SlFwd p) {
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
    local += S;
    if (p.q) {
      const double inv = 1.0 / (B1 * B2);       // 1/B1 = B2 inv, 1/B2 = B1 inv
      const double Q = -2.0 * cn * S * (B1 * inv);
      const double R = 2.0 * cn * A1 * inv;
      const long o = item * M + ((long)cz * OH + cy) * OW + cx;
      p.q[o] = Q;
      p.r[o] = R;
      if (p.pa) p.pa[o] = 2.0 * uy * A2 * inv - 2.0 * ux * S * (B2 * inv) - ux * Q - uy * R;
      if (p.pb) p.pb[o] = 2.0 * ux * A2 * inv - 2.0 * uy * S * (B2 * inv) - uy * Q - ux * R;
    }
    __builtin_amdgcn_sched_barrier(0);          // one window's divisions at a time
  }
  local = block_tree_sum<256>(local, red);      // block sum in a fixed order
  if (tid == 0) p.partials[item * p.tiles + blockIdx.x] = local;
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

template <int WZ, int TZ>
__global__ __launch_bounds__(256) void sl_backward_kernel(SlBwd p) {
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
  const double up = (double)p.upstream[(item / p.channels) * p.up_stride] * p.scale;
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

// The ONE place the tiling of both launches is decided.  Status as the entry points return it.
static int sl_geometry(const char* who, const int32_t* dhw, int32_t items, SlGeom* g) {
  MPGAN_CHECK_ARG(dhw != nullptr, "%s: null dhw", who);
  MPGAN_CHECK_ARG(items >= 1 && items <= 65535, "%s: %d items outside [1, 65535]", who, items);
  MPGAN_CHECK_ARG(dhw[0] >= 1 && dhw[1] >= SL_W && dhw[2] >= SL_W, "%s: extents (%d, %d, %d) below the 7-wide window",
                  who, dhw[0], dhw[1], dhw[2]);
  MPGAN_UNSUPPORTED(dhw[0] > 1 && dhw[0] < SL_W, "%s: depth %d is neither a slice (1) nor >= 7", who, dhw[0]);
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
  MPGAN_CHECK_ARG(g->fwd_tiles < (1L << 31) && g->bwd_tiles < (1L << 31), "%s: too many tiles", who);
  return MPGAN_OK;
}

static int sl_maps(int grad_mask) { return grad_mask == 0 ? 0 : (grad_mask == 3 ? 4 : 3); }

}  // namespace mpgan

using namespace mpgan;

extern "C" int64_t mpgan_ssim_loss_workspace(const int32_t* dhw, int32_t items, int32_t grad_mask,
                                             int64_t* coef_bytes) {
  SlGeom g;
  if (grad_mask < 0 || grad_mask > 3 || sl_geometry("ssim_loss_workspace", dhw, items, &g) != MPGAN_OK) return -1;
  if (coef_bytes) *coef_bytes = (int64_t)sl_maps(grad_mask) * items * g.M * (int64_t)sizeof(double);
  return ((int64_t)items * g.fwd_tiles + items) * (int64_t)sizeof(double);
}

extern "C" int mpgan_ssim_loss_forward(const float* a, const float* b, const int32_t* dhw, int32_t items,
                                       int32_t channels, double lo, double hi, int32_t grad_mask, void* workspace,
                                       int64_t workspace_bytes, void* coef, int64_t coef_bytes, int32_t reduction,
                                       float* loss, void* stream) {
  MPGAN_CHECK_ARG(a && b && workspace && loss, "ssim_loss_forward: null pointer");
  SlGeom g;
  if (int rc = sl_geometry("ssim_loss_forward", dhw, items, &g)) return rc;
  MPGAN_CHECK_ARG(channels >= 1 && items % channels == 0, "ssim_loss_forward: %d items are no multiple of %d channels",
                  items, channels);
  MPGAN_CHECK_ARG(hi - lo > 0.0 && (hi - lo) - (hi - lo) == 0.0, "ssim_loss_forward: value range needs finite hi > lo");
  MPGAN_CHECK_ARG(grad_mask >= 0 && grad_mask <= 3, "ssim_loss_forward: grad_mask %d outside [0, 3]", grad_mask);
  MPGAN_CHECK_ARG(reduction >= 0 && reduction <= 2, "ssim_loss_forward: unknown reduction %d", reduction);
  int64_t need_coef = 0;
  const int64_t need_ws = mpgan_ssim_loss_workspace(dhw, items, grad_mask, &need_coef);
  MPGAN_CHECK_ARG(workspace_bytes >= need_ws, "ssim_loss_forward: workspace too small");
  MPGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "ssim_loss_forward: workspace must be 8-byte aligned");
  MPGAN_CHECK_ARG(grad_mask == 0 || (coef && coef_bytes >= need_coef), "ssim_loss_forward: coef missing or too small");
  MPGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(coef) & 7) == 0, "ssim_loss_forward: coef must be 8-byte aligned");
  const double L = hi - lo;
  SlFwd p;
  p.a = a; p.b = b; p.D = g.D; p.H = g.H; p.W = g.W;
  p.tiles_x = g.fwd_tx; p.tiles_y = g.fwd_ty; p.tiles = g.fwd_tiles;
  p.lo = lo; p.c1 = (0.01 * L) * (0.01 * L); p.c2 = (0.03 * L) * (0.03 * L);
  p.partials = static_cast<double*>(workspace);
  double* ssim_item = p.partials + (long)items * g.fwd_tiles;
  double* maps = static_cast<double*>(coef);
  const long per_map = (long)items * g.M;
  p.q = grad_mask ? maps : nullptr;
  p.r = grad_mask ? maps + per_map : nullptr;
  p.pa = (grad_mask & 1) ? maps + 2 * per_map : nullptr;
  p.pb = (grad_mask & 2) ? maps + (grad_mask == 3 ? 3 : 2) * per_map : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)g.fwd_tiles, (unsigned)items);
  if (g.vol) {
    const size_t smem = 2ul * (SL_TZ3 + SL_W - 1) * SL_PLANE * sizeof(float);
    hipLaunchKernelGGL((sl_forward_kernel<SL_W, SL_TZ3>), grid, dim3(256), smem, st, p);
  } else {
    const size_t smem = 2ul * SL_PLANE * sizeof(float);
    hipLaunchKernelGGL((sl_forward_kernel<1, 1>), grid, dim3(256), smem, st, p);
  }
  // ssim_item = (sum of the item's tile partials) / M; loss = 1 - ssim over the items
  launch_loss_tail(p.partials, g.fwd_tiles, 1.0 / (double)g.M, ssim_item, items, channels, reduction, true, loss, st);
  return check_launch("ssim_loss_forward");
}

extern "C" int mpgan_ssim_loss_backward(const float* a, const float* b, const int32_t* dhw, int32_t items,
                                        int32_t channels, double lo, int32_t grad_mask, const void* coef,
                                        int64_t coef_bytes, const float* upstream, int32_t upstream_stride,
                                        double scale, int32_t wrt, float* grad, void* stream) {
  MPGAN_CHECK_ARG(a && b && coef && upstream && grad, "ssim_loss_backward: null pointer");
  SlGeom g;
  if (int rc = sl_geometry("ssim_loss_backward", dhw, items, &g)) return rc;
  MPGAN_CHECK_ARG(channels >= 1 && items % channels == 0, "ssim_loss_backward: %d items are no multiple of %d channels",
                  items, channels);
  MPGAN_CHECK_ARG(wrt == 0 || wrt == 1, "ssim_loss_backward: wrt %d is neither 0 (a) nor 1 (b)", wrt);
  MPGAN_CHECK_ARG(grad_mask >= 1 && grad_mask <= 3 && ((grad_mask >> wrt) & 1),
                  "ssim_loss_backward: the forward's grad_mask %d holds no maps for wrt %d", grad_mask, wrt);
  MPGAN_CHECK_ARG(upstream_stride == 0 || upstream_stride == 1, "ssim_loss_backward: upstream_stride %d not 0 or 1",
                  upstream_stride);
  MPGAN_CHECK_ARG(lo - lo == 0.0 && scale - scale == 0.0, "ssim_loss_backward: non-finite lo or scale");
  const long per_map = (long)items * g.M;
  MPGAN_CHECK_ARG(coef_bytes >= (int64_t)sl_maps(grad_mask) * per_map * (int64_t)sizeof(double),
                  "ssim_loss_backward: coef too small");
  MPGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(coef) & 7) == 0, "ssim_loss_backward: coef must be 8-byte aligned");
  const double* maps = static_cast<const double*>(coef);
  SlBwd p;
  p.x = wrt == 0 ? a : b;
  p.y = wrt == 0 ? b : a;
  p.D = g.D; p.H = g.H; p.W = g.W; p.OD = g.OD; p.OH = g.OH; p.OW = g.OW;
  p.tiles_x = g.bwd_tx; p.tiles_y = g.bwd_ty;
  p.q = maps;
  p.r = maps + per_map;
  p.p = maps + (wrt == 1 && grad_mask == 3 ? 3 : 2) * per_map;
  const double np = g.vol ? 343.0 : 49.0;
  p.lo = lo; p.scale = scale / (np * (double)g.M);
  p.upstream = upstream; p.up_stride = upstream_stride; p.channels = channels;
  p.grad = grad;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)g.bwd_tiles, (unsigned)items);
  if (g.vol) {
    const size_t smem = (size_t)(SL_TZ3 + SL_W - 1) * SL_PLANE * sizeof(double);
    hipLaunchKernelGGL((sl_backward_kernel<SL_W, SL_TZ3>), grid, dim3(256), smem, st, p);
  } else {
    const size_t smem = (size_t)SL_PLANE * sizeof(double);
    hipLaunchKernelGGL((sl_backward_kernel<1, 1>), grid, dim3(256), smem, st, p);
  }
  return check_launch("ssim_loss_backward");
}
