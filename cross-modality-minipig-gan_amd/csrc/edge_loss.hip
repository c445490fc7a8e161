// Sobel edge loss (include/mpgan_hip.h: "Sobel edge loss" states the operator, the loss and the adjoint of the clamp).
// LDS-tiled stencils, one block of 256 threads per TZ x 8 x 32 tile of one item (TZ = 4; 1 when the image is one plane),
// no atomics, no scatter; every sum has a fixed order:
//
//   el_forward_kernel<.., false>   m(x): stages the tile of x with a halo of 1, the border replicated by clamping the
//                                  source coordinates, and writes the map.
//   el_forward_kernel<.., true>    the loss: stages both images, a thread forms m(a) and m(b) of its (y, x) column and
//                                  adds |m(a) - m(b)| in double; block partial -> workspace slot.  No map is written.
//   launch_loss_tail (loss_ops.hip) an item's partials in slot order + a fixed tree (loss_item_kernel), then the
//                                  reduction over the items (loss_reduce_kernel<false>); reduce.h states the orders.
//   el_backward_kernel             the adjoint as a gather.  Stages x (and, for the loss, the other image) with a halo
//                                  of 2, writes the three coefficients w_q G_k(q) / m(q) of the tile plus a halo of 1
//                                  to LDS -- zero for a q outside the image -- and every voxel of the tile then sums its
//                                  transposed taps.  w_q is the upstream map (magnitude backward) or
//                                  sign(m(x)_q - m(other)_q), formed on the fly (loss backward): nothing but the inputs
//                                  passes from forward to backward.
//
// el_column is the ONE place G and m are computed: the loss, the map and both backward forms see the same bits of m.
// The clamp's adjoint only changes the weight of the centre tap of a border voxel, per axis (see the header); a block
// that touches no face of the image runs the gather with the constant interior weights (a block-uniform branch).
// Rows are staged and stored 16 bytes wide wherever a group of four samples lies inside the row and its address is
// 16-byte aligned, sample by sample otherwise: any W and any 4-byte-aligned pointer work.
// The entry points' items / reduction / wrt / upstream_stride / scale / workspace checks are mpgan_common.h's.
#include "mpgan_common.h"

namespace mpgan {

constexpr int EL_TY = 8, EL_TX = 32;
constexpr int EL_TZ3 = 4;                       // z tile when the image has more than one plane
constexpr int EL_RS = 40;                       // LDS row stride in floats: rows stay 16-byte aligned
constexpr int EL_X0 = 4;                        // a row's index of the tile's first x; the halos sit on either side
constexpr int EL_RED = 512;                     // floats in front of the tiles: double[256] for the block sum

// Stage planes [zlo, zlo + planes) x rows [y0 - HALO, y0 + 8 + HALO) x samples [x0 - HALO, x0 + 32 + HALO) of one
// image into s[planes][8 + 2 HALO][EL_RS], every source coordinate clamped into the image (the replicate border).
template <int HALO>
__device__ __forceinline__ void el_stage(const float* __restrict__ img, int D, int H, int W, int zlo, int planes,
                                         int y0, int x0, float* s) {
  constexpr int RY = EL_TY + 2 * HALO;
  constexpr int PER_ROW = EL_TX / 4 + 2 * HALO; // 8 groups of four + the halo samples
  const int n = planes * RY * PER_ROW;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int j = i % PER_ROW, row = i / PER_ROW;
    const int ry = row % RY, rz = row / RY;
    const int z = min(max(zlo + rz, 0), D - 1), y = min(max(y0 - HALO + ry, 0), H - 1);
    const float* src = img + ((long)z * H + y) * W;
    float* dst = s + (rz * RY + ry) * EL_RS + EL_X0;
    if (j < EL_TX / 4) {
      const int x = x0 + 4 * j;
      float4 v;
      if (x + 4 <= W && (reinterpret_cast<uintptr_t>(src + x) & 15) == 0) {
        v = *reinterpret_cast<const float4*>(src + x);
      } else {
        v.x = src[min(x, W - 1)]; v.y = src[min(x + 1, W - 1)];
        v.z = src[min(x + 2, W - 1)]; v.w = src[min(x + 3, W - 1)];
      }
      *reinterpret_cast<float4*>(dst + 4 * j) = v;
    } else {
      const int h = j - EL_TX / 4;              // 0 .. 2 HALO - 1: the left halo, then the right one
      const int off = h < HALO ? h - HALO : EL_TX + (h - HALO);
      dst[off] = src[min(max(x0 + off, 0), W - 1)];
    }
  }
}

// Store the tile t[NZ][8][32] (LDS) into the image, 16 bytes wide where the address allows.
template <int NZ>
__device__ __forceinline__ void el_store(const float* t, float* __restrict__ img, int D, int H, int W, int z0, int y0,
                                         int x0) {
  for (int i = threadIdx.x; i < NZ * EL_TY * EL_TX / 4; i += 256) {
    const int j = i % (EL_TX / 4), ry = (i / (EL_TX / 4)) % EL_TY, rz = i / (EL_TX / 4 * EL_TY);
    const int z = z0 + rz, y = y0 + ry, x = x0 + 4 * j;
    if (z >= D || y >= H || x >= W) continue;
    float* dst = img + ((long)z * H + y) * W + x;
    const float4 v = *reinterpret_cast<const float4*>(t + 4 * i);
    if (x + 4 <= W && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
      *reinterpret_cast<float4*>(dst) = v;
    } else {
      dst[0] = v.x;
      if (x + 1 < W) dst[1] = v.y;
      if (x + 2 < W) dst[2] = v.z;
      if (x + 3 < W) dst[3] = v.w;
    }
  }
}

// G (order z, y, x) and m of NZ consecutive voxels of one (y, x) column.  c points at the column's sample in the plane
// below the first voxel, rows EL_RS apart, planes ps apart (ps == 0: the image is one plane and every z tap reads
// it).  A plane's three in-plane sums are formed once and serve the three voxels that tap the plane.  The sums are
// doubles -- exact for fp32 samples, so G keeps its relative precision where the image is nearly flat -- rounded to
// fp32 once; contraction is off, so the bits do not depend on the kernel this is inlined into.
template <int NZ>
__device__ __forceinline__ void el_column(const float* c, int ps, float eps, float (&g)[NZ][3], float (&m)[NZ]) {
#pragma clang fp contract(off)
  double ss[NZ + 2], sdx[NZ + 2], sdy[NZ + 2];  // per plane: smooth y smooth x, smooth y diff x, diff y smooth x
#pragma unroll
  for (int k = 0; k < NZ + 2; ++k) {
    const float* r = c + k * ps;
    double s[3], d[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float* q = r + (j - 1) * EL_RS;
      const double lo = (double)q[-1], mid = (double)q[0], hi = (double)q[1];
      s[j] = (lo + hi) + 2.0 * mid;
      d[j] = hi - lo;
    }
    ss[k] = (s[0] + s[2]) + 2.0 * s[1];
    sdx[k] = (d[0] + d[2]) + 2.0 * d[1];
    sdy[k] = s[2] - s[0];
  }
#pragma unroll
  for (int k = 0; k < NZ; ++k) {
    const float gz = (float)((ss[k + 2] - ss[k]) * 0.03125);
    const float gy = (float)(((sdy[k] + sdy[k + 2]) + 2.0 * sdy[k + 1]) * 0.03125);
    const float gx = (float)(((sdx[k] + sdx[k + 2]) + 2.0 * sdx[k + 1]) * 0.03125);
    g[k][0] = gz; g[k][1] = gy; g[k][2] = gx;
    m[k] = sqrtf(((gx * gx + gy * gy) + gz * gz) + eps);
  }
}

struct ElFwd {
  const float* a;
  const float* b;                               // the loss only
  int D, H, W, tiles_x, tiles_y;
  long tiles;                                   // per item
  float eps;
  double* partials;                             // [items][tiles], the loss only
  float* out;                                   // [items][D][H][W], the map only
};

template <int NZ, bool LOSS>
__global__ __launch_bounds__(256) void el_forward_kernel(ElFwd p) {
  constexpr int PZ = NZ == 1 ? 1 : NZ + 2;      // staged planes
  constexpr int PLANE = (EL_TY + 2) * EL_RS;
  extern __shared__ __attribute__((aligned(16))) float el_sm[];   // double red[256] | a[PZ][10][EL_RS] | b likewise
  float* sa = el_sm + EL_RED;
  float* sb = sa + PZ * PLANE;
  const int tid = threadIdx.x;
  const long item = blockIdx.y;
  const long vox = (long)p.D * p.H * p.W;
  const int bx = blockIdx.x % p.tiles_x;
  const int by = (blockIdx.x / p.tiles_x) % p.tiles_y;
  const int bz = blockIdx.x / (p.tiles_x * p.tiles_y);
  const int z0 = bz * NZ, y0 = by * EL_TY, x0 = bx * EL_TX;
  const int zlo = NZ == 1 ? 0 : z0 - 1;
  el_stage<1>(p.a + item * vox, p.D, p.H, p.W, zlo, PZ, y0, x0, sa);
  if (LOSS) el_stage<1>(p.b + item * vox, p.D, p.H, p.W, zlo, PZ, y0, x0, sb);
  __syncthreads();
  const int tx = tid % EL_TX, ty = tid / EL_TX;
  const int ps = NZ == 1 ? 0 : PLANE;
  const int col = (ty + 1) * EL_RS + EL_X0 + tx;
  const bool col_ok = y0 + ty < p.H && x0 + tx < p.W;
  float g[NZ][3], ma[NZ];
  el_column<NZ>(sa + col, ps, p.eps, g, ma);
  if (LOSS) {
    float mb[NZ];
    el_column<NZ>(sb + col, ps, p.eps, g, mb);
    double local = 0.0;
#pragma unroll
    for (int k = 0; k < NZ; ++k)
      if (col_ok && z0 + k < p.D) local += fabs((double)ma[k] - (double)mb[k]);
    local = block_tree_sum<256>(local, reinterpret_cast<double*>(el_sm));   // block sum in a fixed order
    if (tid == 0) p.partials[item * p.tiles + blockIdx.x] = local;
  } else {
    __syncthreads();                            // every column has been read: the tile of a becomes the output tile
#pragma unroll
    for (int k = 0; k < NZ; ++k) sa[(k * EL_TY + ty) * EL_TX + tx] = ma[k];
    __syncthreads();
    el_store<NZ>(sa, p.out + item * vox, p.D, p.H, p.W, z0, y0, x0);
  }
}

struct ElBwd {
  const float* x;                               // the image the gradient is for
  const float* y;                               // the other image (the loss only)
  const float* dy;                              // the upstream map (the magnitude backward only)
  int D, H, W, tiles_x, tiles_y;
  float eps;
  double scale;                                 // the loss: reduction factor / N
  const float* upstream;                        // the loss
  int up_stride, channels;
  float* grad;
};

// One coefficient plane's contribution to a voxel: the in-plane transposed taps of the three maps around o (the
// voxel's own position in plane 0 of map z).  Along an axis the taps of p are q = p - 1, p, p + 1 with weights
// (1, sc, 1) for Sv and (1, dc, -1) for Dv.  pz: map z smoothed in y and x; ps: maps y and x, one differentiated and
// one smoothed in-plane, both to be smoothed along z.
__device__ __forceinline__ void el_plane_taps(const float* o, int map_stride, float scy, float dcy, float scx, float dcx,
                                              float& pz, float& ps) {
  float sz[3], sy[3], dx[3];
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    const float* r = o + (u - 1) * EL_RS;
    sz[u] = (r[-1] + r[1]) + scx * r[0];
    const float* ry = r + map_stride;
    sy[u] = (ry[-1] + ry[1]) + scx * ry[0];
    const float* rx = r + 2 * map_stride;
    dx[u] = (rx[-1] - rx[1]) + dcx * rx[0];
  }
  pz = (sz[0] + sz[2]) + scy * sz[1];
  ps = ((sy[0] - sy[2]) + dcy * sy[1]) + ((dx[0] + dx[2]) + scy * dx[1]);
}

template <int NZ, bool LOSS>
__global__ __launch_bounds__(256) void el_backward_kernel(ElBwd p) {
  constexpr int HZ = NZ == 1 ? 0 : 1;           // coefficient planes beyond the tile on either side
  constexpr int CZ = NZ + 2 * HZ;               // coefficient planes
  constexpr int PZ = NZ == 1 ? 1 : CZ + 2;      // staged planes
  constexpr int PLANE = (EL_TY + 4) * EL_RS;    // staged with a halo of 2
  constexpr int CY = EL_TY + 2, CX = EL_TX + 2; // coefficients: the tile plus a halo of 1; x0 - 1 at row index EL_X0 - 1
  constexpr int CPLANE = CY * EL_RS, CMAP = CZ * CPLANE;
  extern __shared__ __attribute__((aligned(16))) float el_sm[];   // x[PZ][12][EL_RS] | other likewise | coef[3][CZ][10][EL_RS]
  float* sx = el_sm;
  float* sy = sx + PZ * PLANE;
  float* co = sx + (LOSS ? 2 : 1) * PZ * PLANE;
  const int tid = threadIdx.x;
  const long item = blockIdx.y;
  const long vox = (long)p.D * p.H * p.W;
  const int bx = blockIdx.x % p.tiles_x;
  const int by = (blockIdx.x / p.tiles_x) % p.tiles_y;
  const int bz = blockIdx.x / (p.tiles_x * p.tiles_y);
  const int z0 = bz * NZ, y0 = by * EL_TY, x0 = bx * EL_TX;
  const int zlo = NZ == 1 ? 0 : z0 - HZ - 1;
  el_stage<2>(p.x + item * vox, p.D, p.H, p.W, zlo, PZ, y0, x0, sx);
  if (LOSS) el_stage<2>(p.y + item * vox, p.D, p.H, p.W, zlo, PZ, y0, x0, sy);
  __syncthreads();
  const int ps = NZ == 1 ? 0 : PLANE;
  // coefficients of the columns of the tile plus a halo of 1: w_q G_k / m inside the image, 0 outside
  for (int col = tid; col < CY * CX; col += 256) {
    const int cy = col / CX, cx = col % CX;
    const int qy = y0 - 1 + cy, qx = x0 - 1 + cx;
    float* dst = co + cy * EL_RS + (EL_X0 - 1) + cx;
    const bool col_ok = qy >= 0 && qy < p.H && qx >= 0 && qx < p.W;
    if (!col_ok) {
#pragma unroll
      for (int k = 0; k < CZ; ++k) dst[k * CPLANE] = dst[CMAP + k * CPLANE] = dst[2 * CMAP + k * CPLANE] = 0.f;
      continue;
    }
    const int src = (cy + 1) * EL_RS + (EL_X0 - 1) + cx;     // the column in plane zlo, the plane below the first q
    float g[CZ][3], m[CZ], w[CZ];
    el_column<CZ>(sx + src, ps, p.eps, g, m);
    if (LOSS) {
      float go[CZ][3], mo[CZ];
      el_column<CZ>(sy + src, ps, p.eps, go, mo);
#pragma unroll
      for (int k = 0; k < CZ; ++k) w[k] = sgn(m[k] - mo[k]);
    }
#pragma unroll
    for (int k = 0; k < CZ; ++k) {
      const int qz = z0 - HZ + k;
      const bool in = qz >= 0 && qz < p.D;
      float wq = 0.f;
      if (in) wq = LOSS ? w[k] : p.dy[item * vox + ((long)qz * p.H + qy) * p.W + qx];
      const float f = in ? wq / m[k] : 0.f;
      dst[k * CPLANE] = f * g[k][0];
      dst[CMAP + k * CPLANE] = f * g[k][1];
      dst[2 * CMAP + k * CPLANE] = f * g[k][2];
    }
  }
  __syncthreads();
  // the gather: every voxel of the tile sums its transposed taps
  const int tx = tid % EL_TX, ty = tid / EL_TX;
  const int py = y0 + ty, px = x0 + tx;
  const bool border = z0 == 0 || z0 + NZ >= p.D || y0 == 0 || y0 + EL_TY >= p.H || x0 == 0 || x0 + EL_TX >= p.W;
  float scy = 2.f, dcy = 0.f, scx = 2.f, dcx = 0.f, scz[NZ], dcz[NZ];
#pragma unroll
  for (int k = 0; k < NZ; ++k) { scz[k] = 2.f; dcz[k] = 0.f; }
  if (border) {                                 // block-uniform: the folded taps of the clamp change the centre weights
    scy += (float)(py == 0) + (float)(py == p.H - 1); dcy = (float)(py == p.H - 1) - (float)(py == 0);
    scx += (float)(px == 0) + (float)(px == p.W - 1); dcx = (float)(px == p.W - 1) - (float)(px == 0);
#pragma unroll
    for (int k = 0; k < NZ; ++k) {
      const int pz = z0 + k;
      scz[k] += (float)(pz == 0) + (float)(pz == p.D - 1); dcz[k] = (float)(pz == p.D - 1) - (float)(pz == 0);
    }
  }
  float acc[NZ];
#pragma unroll
  for (int k = 0; k < NZ; ++k) acc[k] = 0.f;
  const float* o = co + (ty + 1) * EL_RS + EL_X0 + tx;
#pragma unroll
  for (int j = 0; j < CZ; ++j) {
    float pz, pyx;
    el_plane_taps(o + j * CPLANE, CMAP, scy, dcy, scx, dcx, pz, pyx);
#pragma unroll
    for (int k = 0; k < NZ; ++k) {
      const int u = j - HZ - k;                 // the plane is q_z = p_z + u
      if (u == -1) acc[k] += pz + pyx;
      if (u == 0) acc[k] += dcz[k] * pz + scz[k] * pyx;
      if (u == 1) acc[k] += pyx - pz;
    }
  }
  float f = 0.03125f;
  if (LOSS) f = (float)((double)p.upstream[(item / p.channels) * p.up_stride] * p.scale * 0.03125);
  // the staged x was last read before the barrier above: its space becomes the output tile
#pragma unroll
  for (int k = 0; k < NZ; ++k) sx[(k * EL_TY + ty) * EL_TX + tx] = f * acc[k];
  __syncthreads();
  el_store<NZ>(sx, p.grad + item * vox, p.D, p.H, p.W, z0, y0, x0);
}

struct ElGeom {
  bool vol;                                     // more than one plane: the TZ = 4 forms
  int D, H, W, tiles_x, tiles_y;
  long tiles, vox;
};

// The ONE place the tiling of every launch is decided.  Status as the entry points return it.
static int el_geometry(const char* who, const int32_t* dhw, int32_t items, ElGeom* g) {
  MPGAN_CHECK_ARG(dhw != nullptr, "%s: null dhw", who);
  MPGAN_CHECK_ARG(items >= 1 && items <= 65535, "%s: %d items outside [1, 65535]", who, items);
  MPGAN_CHECK_ARG(dhw[0] >= 1 && dhw[1] >= 1 && dhw[2] >= 1, "%s: empty extents (%d, %d, %d)", who, dhw[0], dhw[1],
                  dhw[2]);
  g->D = dhw[0]; g->H = dhw[1]; g->W = dhw[2];
  g->vol = g->D > 1;
  g->vox = (long)g->D * g->H * g->W;
  const int tz = g->vol ? EL_TZ3 : 1;
  g->tiles_x = (g->W + EL_TX - 1) / EL_TX; g->tiles_y = (g->H + EL_TY - 1) / EL_TY;
  g->tiles = (long)((g->D + tz - 1) / tz) * g->tiles_y * g->tiles_x;
  MPGAN_CHECK_ARG(g->tiles < (1L << 31), "%s: too many tiles", who);
  return MPGAN_OK;
}

static size_t el_fwd_lds(int nz, bool loss) {
  return ((size_t)EL_RED + (size_t)(loss ? 2 : 1) * (nz == 1 ? 1 : nz + 2) * (EL_TY + 2) * EL_RS) * sizeof(float);
}

static size_t el_bwd_lds(int nz, bool loss) {
  const size_t cz = nz == 1 ? 1 : nz + 2, pz = nz == 1 ? 1 : nz + 4;
  return ((size_t)(loss ? 2 : 1) * pz * (EL_TY + 4) * EL_RS + 3 * cz * (EL_TY + 2) * EL_RS) * sizeof(float);
}

}  // namespace mpgan

using namespace mpgan;

extern "C" int mpgan_sobel_magnitude_forward(const float* x, const int32_t* dhw, int32_t items, double eps, float* out,
                                             void* stream) {
  MPGAN_CHECK_ARG(x && out, "sobel_magnitude_forward: null pointer");
  ElGeom g;
  if (int rc = el_geometry("sobel_magnitude_forward", dhw, items, &g)) return rc;
  MPGAN_CHECK_ARG((float)eps > 0.f && is_finite(eps), "sobel_magnitude_forward: eps must be positive and finite");
  ElFwd p;
  p.a = x; p.b = nullptr; p.D = g.D; p.H = g.H; p.W = g.W;
  p.tiles_x = g.tiles_x; p.tiles_y = g.tiles_y; p.tiles = g.tiles;
  p.eps = (float)eps; p.partials = nullptr; p.out = out;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)g.tiles, (unsigned)items);
  if (g.vol) {
    hipLaunchKernelGGL((el_forward_kernel<EL_TZ3, false>), grid, dim3(256), el_fwd_lds(EL_TZ3, false), st, p);
  } else {
    hipLaunchKernelGGL((el_forward_kernel<1, false>), grid, dim3(256), el_fwd_lds(1, false), st, p);
  }
  return check_launch("sobel_magnitude_forward");
}

extern "C" int mpgan_sobel_magnitude_backward(const float* x, const int32_t* dhw, int32_t items, double eps,
                                              const float* dy, float* dx, void* stream) {
  MPGAN_CHECK_ARG(x && dy && dx, "sobel_magnitude_backward: null pointer");
  ElGeom g;
  if (int rc = el_geometry("sobel_magnitude_backward", dhw, items, &g)) return rc;
  MPGAN_CHECK_ARG((float)eps > 0.f && is_finite(eps), "sobel_magnitude_backward: eps must be positive and finite");
  ElBwd p;
  p.x = x; p.y = nullptr; p.dy = dy; p.D = g.D; p.H = g.H; p.W = g.W;
  p.tiles_x = g.tiles_x; p.tiles_y = g.tiles_y;
  p.eps = (float)eps; p.scale = 1.0; p.upstream = nullptr; p.up_stride = 0; p.channels = 1;
  p.grad = dx;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)g.tiles, (unsigned)items);
  if (g.vol) {
    hipLaunchKernelGGL((el_backward_kernel<EL_TZ3, false>), grid, dim3(256), el_bwd_lds(EL_TZ3, false), st, p);
  } else {
    hipLaunchKernelGGL((el_backward_kernel<1, false>), grid, dim3(256), el_bwd_lds(1, false), st, p);
  }
  return check_launch("sobel_magnitude_backward");
}

extern "C" int64_t mpgan_edge_loss_workspace(const int32_t* dhw, int32_t items) {
  ElGeom g;
  if (el_geometry("edge_loss_workspace", dhw, items, &g) != MPGAN_OK) return -1;
  return ((int64_t)items * g.tiles + items) * (int64_t)sizeof(double);
}

extern "C" int mpgan_edge_loss_forward(const float* a, const float* b, const int32_t* dhw, int32_t items,
                                       int32_t channels, double eps, void* workspace, int64_t workspace_bytes,
                                       int32_t reduction, float* loss, void* stream) {
  MPGAN_CHECK_ARG(a && b && loss, "edge_loss_forward: null pointer");
  ElGeom g;
  if (int rc = el_geometry("edge_loss_forward", dhw, items, &g)) return rc;
  if (int rc = check_items("edge_loss_forward", items, channels)) return rc;
  MPGAN_CHECK_ARG((float)eps > 0.f && is_finite(eps), "edge_loss_forward: eps must be positive and finite");
  if (int rc = check_reduction("edge_loss_forward", reduction)) return rc;
  if (int rc = check_workspace("edge_loss_forward", workspace, workspace_bytes, mpgan_edge_loss_workspace(dhw, items)))
    return rc;
  ElFwd p;
  p.a = a; p.b = b; p.D = g.D; p.H = g.H; p.W = g.W;
  p.tiles_x = g.tiles_x; p.tiles_y = g.tiles_y; p.tiles = g.tiles;
  p.eps = (float)eps; p.partials = static_cast<double*>(workspace); p.out = nullptr;
  double* loss_item = p.partials + (long)items * g.tiles;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)g.tiles, (unsigned)items);
  if (g.vol) {
    hipLaunchKernelGGL((el_forward_kernel<EL_TZ3, true>), grid, dim3(256), el_fwd_lds(EL_TZ3, true), st, p);
  } else {
    hipLaunchKernelGGL((el_forward_kernel<1, true>), grid, dim3(256), el_fwd_lds(1, true), st, p);
  }
  // loss_item = (sum of the item's tile partials) / N; loss = loss_item over the items
  launch_loss_tail(p.partials, g.tiles, 1.0 / (double)g.vox, loss_item, items, channels, reduction, false, loss, st);
  return check_launch("edge_loss_forward");
}

extern "C" int mpgan_edge_loss_backward(const float* a, const float* b, const int32_t* dhw, int32_t items,
                                        int32_t channels, double eps, const float* upstream, int32_t upstream_stride,
                                        double scale, int32_t wrt, float* grad, void* stream) {
  MPGAN_CHECK_ARG(a && b && upstream && grad, "edge_loss_backward: null pointer");
  ElGeom g;
  if (int rc = el_geometry("edge_loss_backward", dhw, items, &g)) return rc;
  if (int rc = check_items("edge_loss_backward", items, channels)) return rc;
  MPGAN_CHECK_ARG((float)eps > 0.f && is_finite(eps), "edge_loss_backward: eps must be positive and finite");
  if (int rc = check_wrt("edge_loss_backward", wrt)) return rc;
  if (int rc = check_upstream_stride("edge_loss_backward", upstream_stride)) return rc;
  if (int rc = check_scale("edge_loss_backward", scale)) return rc;
  ElBwd p;
  p.x = wrt == 0 ? a : b;                       // -sign(m(a) - m(b)) = sign(m(b) - m(a)): one form for both
  p.y = wrt == 0 ? b : a;
  p.dy = nullptr; p.D = g.D; p.H = g.H; p.W = g.W;
  p.tiles_x = g.tiles_x; p.tiles_y = g.tiles_y;
  p.eps = (float)eps; p.scale = scale / (double)g.vox;
  p.upstream = upstream; p.up_stride = upstream_stride; p.channels = channels;
  p.grad = grad;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)g.tiles, (unsigned)items);
  if (g.vol) {
    hipLaunchKernelGGL((el_backward_kernel<EL_TZ3, true>), grid, dim3(256), el_bwd_lds(EL_TZ3, true), st, p);
  } else {
    hipLaunchKernelGGL((el_backward_kernel<1, true>), grid, dim3(256), el_bwd_lds(1, true), st, p);
  }
  return check_launch("edge_loss_backward");
}
