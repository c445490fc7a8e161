// The HBM-bound passes of the bf16 storage mode: norm + LeakyReLU apply, the BatchNorm + LeakyReLU backward (with and
// without the perceptual taps of a peer pass), the perceptual tap L1.  z is stored bf16, vectors and sums are fp32; thread =
// 8 channels of one pixel.  Row vectors and the backward formula: norm_rows.h, shared with norm_ops.hip and the epilogues.
#include "mpgan_common.h"
#include "norm_rows.h"
#include <type_traits>

namespace mpgan {

// a = LeakyReLU(z*scale + shift): the layer's activation, materialised once (thread = 8 channels of one pixel)
template <typename TO>
__global__ __launch_bounds__(256) void norm_act_bf16_kernel(const __bf16* __restrict__ z, int ldz,
                                                            const float* __restrict__ scale,
                                                            const float* __restrict__ shift, float slope, long rows,
                                                            int C, TO* __restrict__ out, int ldo) {
  const int CG = C / 8;
  const long total = rows * CG;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long row = i / CG;
    const int c = (int)(i - row * CG) * 8;
    float v[8], sc[8], sh[8];
    ld8(z + row * ldz + c, v);
    ld8(scale + c, sc);
    ld8(shift + c, sh);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float y = v[e] * sc[e] + sh[e];
      v[e] = y < 0.f ? y * slope : y;
    }
    st8(out + row * ldo + c, v);
  }
}

// BatchNorm + LeakyReLU backward on bf16 z:  gy = g*act'(y);  partial rows [chunks*n][3][C] of
// (sum gy, sum gy*zhat, 0) in the layout mpgan_norm_bwd_finalize consumes; apply: dz = scale*(gy - c1 - zhat*c2).
// block = R rows x C/8 column groups; chunk = blockIdx.x of gridDim.x over the rows.
// PEER: with the perceptual taps of a peer pass (variant B): the formula of norm_rows.h on the stored bf16 z of both
// passes, with y = z*scale + shift and a = LeakyReLU_slope(y) in fp32 on each side.  Same grid, rows and partial layout;
// the instantiations without a peer take an empty descriptor and load and compute nothing for it.
struct PeerBf16 {
  const __bf16* z;     // the peer pass's stored raw conv output, [rows][ld]
  int ld;
  const float* scale;  // its norm scale / shift
  const float* shift;
  const float* coef;   // device float[3]: (cz, cy, ca)
};
struct NoPeerBf16 {};
template <bool PEER>
using peer_bf16_t = std::conditional_t<PEER, PeerBf16, NoPeerBf16>;

template <typename TG, bool PEER>
__global__ __launch_bounds__(256) void norm_bwd_reduce_bf16_kernel(const TG* __restrict__ g, int ldg,
                                                                   const __bf16* __restrict__ z, int ldz,
                                                                   const float* __restrict__ scale,
                                                                   const float* __restrict__ shift,
                                                                   const float* __restrict__ mean,
                                                                   const float* __restrict__ invstd,
                                                                   peer_bf16_t<PEER> pr, float slope, long rows, int C,
                                                                   float* __restrict__ partials) {
  extern __shared__ float red[];   // [R][2][C]
  const int CG = C / 8, R = 256 / CG;
  const int q = threadIdx.x % CG, r = threadIdx.x / CG, c = q * 8;
  const long per = (rows + gridDim.x - 1) / gridDim.x;
  const long beg = (long)blockIdx.x * per, end = beg + per < rows ? beg + per : rows;
  float a0[8], a1[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) a0[e] = a1[e] = 0.f;
  if (r < R) {
    float sc[8], sh[8], mu[8], is[8], psc[8], psh[8], cy, ca;
    ld8(scale + c, sc); ld8(shift + c, sh); ld8(mean + c, mu); ld8(invstd + c, is);
    if constexpr (PEER) {
      ld8(pr.scale + c, psc); ld8(pr.shift + c, psh);
      cy = pr.coef[1], ca = pr.coef[2];
    }
    for (long row = beg + r; row < end; row += R) {
      float zv[8], gv[8], zp[8];
      ld8(z + row * ldz + c, zv);
      ld8(g + row * ldg + c, gv);
      if constexpr (PEER) ld8(pr.z + row * pr.ld + c, zp);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float y = zv[e] * sc[e] + sh[e];
        float gy;
        if constexpr (PEER) gy = norm_bwd_gy_peer(gv[e], y, zp[e] * psc[e] + psh[e], true, slope, cy, ca);
        else gy = norm_bwd_gy(gv[e], y, true, slope);
        a0[e] += gy;
        a1[e] = fmaf(gy, (zv[e] - mu[e]) * is[e], a1[e]);
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      red[(r * 2 + 0) * C + c + e] = a0[e];
      red[(r * 2 + 1) * C + c + e] = a1[e];
    }
  }
  __syncthreads();
  float* out = partials + (long)blockIdx.x * 3 * C;
  for (int i = threadIdx.x; i < 3 * C; i += 256) {
    float s = 0.f;
    if (i < 2 * C)
      for (int rr = 0; rr < R; ++rr) s += red[rr * 2 * C + i];
    out[i] = s;
  }
}

// dz (bf16) = scale*(gy - c1 - zhat*c2); optionally per-block column sums of the ROUNDED dz (the conv's bias
// gradient: dbias = colsum(dy)) as partial rows [gridDim.x][C].
template <typename TG, bool PEER>
__global__ __launch_bounds__(256) void norm_bwd_apply_bf16_kernel(const TG* __restrict__ g, int ldg,
                                                                  const __bf16* __restrict__ z, int ldz,
                                                                  const float* __restrict__ scale,
                                                                  const float* __restrict__ shift,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd,
                                                                  const float* __restrict__ c1,
                                                                  const float* __restrict__ c2, peer_bf16_t<PEER> pr,
                                                                  float slope, long rows, int C,
                                                                  __bf16* __restrict__ dz, int lddz,
                                                                  float* __restrict__ bias_partials) {
  extern __shared__ float red[];   // [R][C]
  const int CG = C / 8, R = 256 / CG;
  const int q = threadIdx.x % CG, r = threadIdx.x / CG, c = q * 8;
  float bs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bs[e] = 0.f;
  if (r < R) {
    float sc[8], sh[8], mu[8], is[8], k1[8], k2[8], psc[8], psh[8], cz, cy, ca;
    ld8(scale + c, sc); ld8(shift + c, sh); ld8(mean + c, mu); ld8(invstd + c, is); ld8(c1 + c, k1); ld8(c2 + c, k2);
    if constexpr (PEER) {
      ld8(pr.scale + c, psc); ld8(pr.shift + c, psh);
      cz = pr.coef[0], cy = pr.coef[1], ca = pr.coef[2];
    }
    for (long row = (long)blockIdx.x * R + r; row < rows; row += (long)gridDim.x * R) {
      float zv[8], gv[8], zp[8], o[8];
      ld8(z + row * ldz + c, zv);
      ld8(g + row * ldg + c, gv);
      if constexpr (PEER) ld8(pr.z + row * pr.ld + c, zp);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float y = zv[e] * sc[e] + sh[e];
        const float zh = (zv[e] - mu[e]) * is[e];
        if constexpr (PEER) {
          const float gy = norm_bwd_gy_peer(gv[e], y, zp[e] * psc[e] + psh[e], true, slope, cy, ca);
          o[e] = norm_bwd_dz(sc[e], gy, zh, k1[e], k2[e]) + norm_bwd_dz_peer(cz, zv[e], zp[e]);
        } else {
          o[e] = norm_bwd_dz(sc[e], norm_bwd_gy(gv[e], y, true, slope), zh, k1[e], k2[e]);
        }
        bs[e] += (float)(__bf16)o[e];
      }
      st8(dz + row * lddz + c, o);
    }
  }
  if (bias_partials) {
    if (r < R) {
#pragma unroll
      for (int e = 0; e < 8; ++e) red[r * C + c + e] = bs[e];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += 256) {
      float s = 0.f;
      for (int rr = 0; rr < R; ++rr) s += red[rr * C + i];
      bias_partials[(long)blockIdx.x * C + i] = s;
    }
  }
}

// Perceptual-loss value of one layer of two passes in bf16 storage (variant B): block partials [gridDim.x][3] of
// sum |z_a - z_b|, |y_a - y_b|, |a_a - a_b|, with z the STORED bf16 raw conv outputs, y = z*scale + shift (fp32) and
// a = LeakyReLU_slope(y).  Thread = 8 channels of one row (16-byte loads); fp32 sums in a fixed grid-stride order, then
// block_sum4 (reduce.h): no atomics, the result is reproducible.
__global__ __launch_bounds__(256) void tap_l1_bf16_kernel(const __bf16* __restrict__ za, int lda,
                                                          const float* __restrict__ sca, const float* __restrict__ sha,
                                                          const __bf16* __restrict__ zb, int ldb,
                                                          const float* __restrict__ scb, const float* __restrict__ shb,
                                                          float slope, long rows, int C, float* __restrict__ partials) {
  __shared__ float red[3][4];
  const int CG = C / 8;
  const long total = rows * CG;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long row = i / CG;
    const int c = (int)(i - row * CG) * 8;
    float va[8], vb[8], ka[8], ha[8], kb[8], hb[8];
    ld8(za + row * lda + c, va);
    ld8(zb + row * ldb + c, vb);
    ld8(sca + c, ka); ld8(sha + c, ha); ld8(scb + c, kb); ld8(shb + c, hb);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float ya = va[e] * ka[e] + ha[e], yb = vb[e] * kb[e] + hb[e];
      const float aa = ya < 0.f ? ya * slope : ya, ab = yb < 0.f ? yb * slope : yb;
      s0 += fabsf(va[e] - vb[e]);
      s1 += fabsf(ya - yb);
      s2 += fabsf(aa - ab);
    }
  }
  s0 = block_sum4(s0, red[0]); s1 = block_sum4(s1, red[1]); s2 = block_sum4(s2, red[2]);
  if (threadIdx.x == 0) {
    partials[blockIdx.x * 3 + 0] = s0; partials[blockIdx.x * 3 + 1] = s1; partials[blockIdx.x * 3 + 2] = s2;
  }
}

// out3[q] = (fp64 sum of the block partials in block order) / numel, rounded once to fp32.  (The fp32 path's final,
// norm_ops.hip, multiplies by 1 / numel instead: other bits, so the two stay two kernels.)
__global__ __launch_bounds__(64) void tap_l1_bf16_final_kernel(const float* __restrict__ partials, int nblocks,
                                                               double numel, float* __restrict__ out3) {
  const int q = threadIdx.x;
  if (q >= 3) return;
  double s = 0.0;
  for (int b = 0; b < nblocks; ++b) s += (double)partials[b * 3 + q];
  out3[q] = (float)(s / numel);
}

static inline int hb_ew_blocks(long total) {
  long b = (total + 255) / 256;
  if (b > 8192) b = 8192;
  return (int)(b < 1 ? 1 : b);
}

}  // namespace mpgan

using namespace mpgan;

extern "C" int mpgan_norm_act_bf16(const void* z, int32_t ldz, const float* scale, const float* shift, float slope,
                                   int64_t rows, int32_t c, void* out, int32_t ldo, int32_t out_f32, void* stream) {
  MPGAN_CHECK_ARG(z && scale && shift && out && rows > 0 && c > 0 && ldz >= c && ldo >= c, "norm_act_bf16: bad argument");
  MPGAN_UNSUPPORTED(c % 8 || ldz % 8 || ldo % 8 || any_misaligned16({z, out}),
                    "norm_act_bf16: channels / pitches %% 8, 16-byte aligned tensors");
  const int blocks = hb_ew_blocks(rows * (c / 8));
  if (out_f32)
    hipLaunchKernelGGL(norm_act_bf16_kernel<float>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const __bf16*>(z), ldz, scale, shift, slope, (long)rows, c, static_cast<float*>(out), ldo);
  else
    hipLaunchKernelGGL(norm_act_bf16_kernel<__bf16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const __bf16*>(z), ldz, scale, shift, slope, (long)rows, c, static_cast<__bf16*>(out), ldo);
  return check_launch("norm_act_bf16");
}

extern "C" int32_t mpgan_norm_bwd_rows_bf16(int64_t rows, int32_t c) {
  if (c <= 0 || c % 8 || c / 8 > 256) return -1;
  const int R = 256 / (c / 8);
  long b = (rows + (long)R * 32 - 1) / ((long)R * 32);     // >= 32 rows per thread row
  if (b > 2048) b = 2048;
  return (int32_t)(b < 1 ? 1 : b);
}

// The argument rules of the four norm-backward entries: `tensors` is what the kernels touch with 16-byte accesses (all
// required and aligned), `pitches` the row pitches (>= C, % 8).  An entry checks its plainly stored partial rows itself.
static int check_norm_bwd_bf16(const char* what, std::initializer_list<const void*> tensors,
                               std::initializer_list<int32_t> pitches, int64_t rows, int32_t c) {
  bool ok = rows > 0;
  for (const void* p : tensors) ok = ok && p != nullptr;
  for (int32_t ld : pitches) ok = ok && ld >= c;
  MPGAN_CHECK_ARG(ok, "%s: bad argument", what);
  bool pitch8 = true;
  for (int32_t ld : pitches) pitch8 = pitch8 && ld % 8 == 0;
  MPGAN_UNSUPPORTED(mpgan_norm_bwd_rows_bf16(rows, c) < 0 || !pitch8 || any_misaligned16(tensors),
                    "%s: C %% 8, C <= 2048, pitches %% 8, 16-byte aligned tensors", what);
  return MPGAN_OK;
}

// The four entries' launches: grid = mpgan_norm_bwd_rows_bf16's rows; g dtype and peer descriptor pick the instantiation.
template <bool PEER>
static int launch_norm_bwd_reduce_bf16(const char* what, const void* g, int32_t g_f32, int32_t ldg, const void* z,
                                       int32_t ldz, const float* scale, const float* shift, const float* mean,
                                       const float* invstd, float slope, int64_t rows, int32_t c, float* partials,
                                       peer_bf16_t<PEER> pr, void* stream) {
  const int nb = mpgan_norm_bwd_rows_bf16(rows, c);
  const int R = 256 / (c / 8);
  const size_t smem = (size_t)R * 2 * c * sizeof(float);
  if (g_f32)
    hipLaunchKernelGGL((norm_bwd_reduce_bf16_kernel<float, PEER>), dim3(nb), dim3(256), smem, (hipStream_t)stream,
                       static_cast<const float*>(g), ldg, static_cast<const __bf16*>(z), ldz, scale, shift, mean, invstd,
                       pr, slope, (long)rows, c, partials);
  else
    hipLaunchKernelGGL((norm_bwd_reduce_bf16_kernel<__bf16, PEER>), dim3(nb), dim3(256), smem, (hipStream_t)stream,
                       static_cast<const __bf16*>(g), ldg, static_cast<const __bf16*>(z), ldz, scale, shift, mean,
                       invstd, pr, slope, (long)rows, c, partials);
  return check_launch(what);
}

template <bool PEER>
static int launch_norm_bwd_apply_bf16(const char* what, const void* g, int32_t g_f32, int32_t ldg, const void* z,
                                      int32_t ldz, const float* scale, const float* shift, const float* mean,
                                      const float* invstd, const float* c1, const float* c2, float slope, int64_t rows,
                                      int32_t c, void* dz, int32_t lddz, float* bias_partials, peer_bf16_t<PEER> pr,
                                      void* stream) {
  const int nb = mpgan_norm_bwd_rows_bf16(rows, c);
  const int R = 256 / (c / 8);
  const size_t smem = bias_partials ? (size_t)R * c * sizeof(float) : 0;
  if (g_f32)
    hipLaunchKernelGGL((norm_bwd_apply_bf16_kernel<float, PEER>), dim3(nb), dim3(256), smem, (hipStream_t)stream,
                       static_cast<const float*>(g), ldg, static_cast<const __bf16*>(z), ldz, scale, shift, mean, invstd,
                       c1, c2, pr, slope, (long)rows, c, static_cast<__bf16*>(dz), lddz, bias_partials);
  else
    hipLaunchKernelGGL((norm_bwd_apply_bf16_kernel<__bf16, PEER>), dim3(nb), dim3(256), smem, (hipStream_t)stream,
                       static_cast<const __bf16*>(g), ldg, static_cast<const __bf16*>(z), ldz, scale, shift, mean,
                       invstd, c1, c2, pr, slope, (long)rows, c, static_cast<__bf16*>(dz), lddz, bias_partials);
  return check_launch(what);
}

extern "C" int mpgan_norm_bwd_reduce_bf16(const void* g, int32_t g_f32, int32_t ldg, const void* z, int32_t ldz,
                                          const float* scale, const float* shift, const float* mean,
                                          const float* invstd, float slope, int64_t rows, int32_t c, float* partials,
                                          void* stream) {
  MPGAN_CHECK_ARG(partials, "norm_bwd_reduce_bf16: bad argument");
  int rc = check_norm_bwd_bf16("norm_bwd_reduce_bf16", {g, z, scale, shift, mean, invstd}, {ldg, ldz}, rows, c);
  if (rc) return rc;
  return launch_norm_bwd_reduce_bf16<false>("norm_bwd_reduce_bf16", g, g_f32, ldg, z, ldz, scale, shift, mean, invstd,
                                            slope, rows, c, partials, NoPeerBf16{}, stream);
}

extern "C" int mpgan_norm_bwd_apply_bf16(const void* g, int32_t g_f32, int32_t ldg, const void* z, int32_t ldz,
                                         const float* scale, const float* shift, const float* mean, const float* invstd,
                                         const float* c1, const float* c2, float slope, int64_t rows, int32_t c, void* dz,
                                         int32_t lddz, float* bias_partials, void* stream) {
  int rc = check_norm_bwd_bf16("norm_bwd_apply_bf16", {g, z, dz, scale, shift, mean, invstd, c1, c2}, {ldg, ldz, lddz},
                               rows, c);
  if (rc) return rc;
  return launch_norm_bwd_apply_bf16<false>("norm_bwd_apply_bf16", g, g_f32, ldg, z, ldz, scale, shift, mean, invstd, c1,
                                           c2, slope, rows, c, dz, lddz, bias_partials, NoPeerBf16{}, stream);
}

static int peer_bf16_of(const mpgan_peer_taps_bf16* t, int32_t c, PeerBf16& pr, const char* what) {
  MPGAN_CHECK_ARG(t && t->z_peer && t->scale_peer && t->shift_peer && t->coef && t->ld_peer >= c,
                  "%s: bad peer descriptor", what);
  MPGAN_UNSUPPORTED(t->ld_peer % 8 || any_misaligned16({t->z_peer, t->scale_peer, t->shift_peer}),
                    "%s: peer pitch %% 8, 16-byte aligned peer tensors", what);
  pr.z = static_cast<const __bf16*>(t->z_peer);
  pr.ld = t->ld_peer;
  pr.scale = t->scale_peer;
  pr.shift = t->shift_peer;
  pr.coef = t->coef;
  return MPGAN_OK;
}

extern "C" int mpgan_norm_bwd_reduce_bf16_peer(const void* g, int32_t g_f32, int32_t ldg, const void* z, int32_t ldz,
                                               const float* scale, const float* shift, const float* mean,
                                               const float* invstd, const mpgan_peer_taps_bf16* peer, float slope,
                                               int64_t rows, int32_t c, float* partials, void* stream) {
  MPGAN_CHECK_ARG(partials, "norm_bwd_reduce_bf16_peer: bad argument");
  int rc = check_norm_bwd_bf16("norm_bwd_reduce_bf16_peer", {g, z, scale, shift, mean, invstd}, {ldg, ldz}, rows, c);
  if (rc) return rc;
  PeerBf16 pr;
  rc = peer_bf16_of(peer, c, pr, "norm_bwd_reduce_bf16_peer");
  if (rc) return rc;
  return launch_norm_bwd_reduce_bf16<true>("norm_bwd_reduce_bf16_peer", g, g_f32, ldg, z, ldz, scale, shift, mean, invstd,
                                           slope, rows, c, partials, pr, stream);
}

extern "C" int mpgan_norm_bwd_apply_bf16_peer(const void* g, int32_t g_f32, int32_t ldg, const void* z, int32_t ldz,
                                              const float* scale, const float* shift, const float* mean,
                                              const float* invstd, const float* c1, const float* c2,
                                              const mpgan_peer_taps_bf16* peer, float slope, int64_t rows, int32_t c,
                                              void* dz, int32_t lddz, float* bias_partials, void* stream) {
  int rc = check_norm_bwd_bf16("norm_bwd_apply_bf16_peer", {g, z, dz, scale, shift, mean, invstd, c1, c2},
                               {ldg, ldz, lddz}, rows, c);
  if (rc) return rc;
  PeerBf16 pr;
  rc = peer_bf16_of(peer, c, pr, "norm_bwd_apply_bf16_peer");
  if (rc) return rc;
  return launch_norm_bwd_apply_bf16<true>("norm_bwd_apply_bf16_peer", g, g_f32, ldg, z, ldz, scale, shift, mean, invstd, c1,
                                          c2, slope, rows, c, dz, lddz, bias_partials, pr, stream);
}

extern "C" int mpgan_tap_l1_bf16(const void* za, int32_t lda, const float* scale_a, const float* shift_a, const void* zb,
                                 int32_t ldb, const float* scale_b, const float* shift_b, float slope, int64_t rows,
                                 int32_t c, float* partials, float* out3, void* stream) {
  MPGAN_CHECK_ARG(za && zb && scale_a && shift_a && scale_b && shift_b && partials && out3 && rows > 0 && c > 0 &&
                      lda >= c && ldb >= c,
                  "tap_l1_bf16: bad argument");
  MPGAN_UNSUPPORTED(c % 8 || lda % 8 || ldb % 8 || any_misaligned16({za, zb, scale_a, shift_a, scale_b, shift_b}),
                    "tap_l1_bf16: channels / pitches %% 8, 16-byte aligned tensors");
  long blocks = (rows * (c / 8) + 255) / 256;
  const long cap = mpgan_tap_l1_partials() / 3;          // the partials size query of mpgan_tap_l1
  if (blocks > cap) blocks = cap;
  hipLaunchKernelGGL(tap_l1_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     static_cast<const __bf16*>(za), lda, scale_a, shift_a, static_cast<const __bf16*>(zb), ldb, scale_b,
                     shift_b, slope, (long)rows, c, partials);
  hipLaunchKernelGGL(tap_l1_bf16_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partials, (int)blocks,
                     (double)rows * c, out3);
  return check_launch("tap_l1_bf16");
}
