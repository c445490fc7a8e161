// What the norm passes of both storage types (norm_ops.hip, norm_bf16.hip) and the conv epilogues that leave norm-backward
// sums (conv_pipe.h, conv_bf16.hip) share: row vectors, the backward formula, the element-wise grid, the vector predicate.
#pragma once
#include <initializer_list>
#include "mpgan_common.h"

namespace mpgan {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// Row vectors: V fp32 channels of one pixel (16-byte accesses for V = 4).
template <int V>
struct Vec;
template <>
struct Vec<4> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[4]) {
    float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  static __device__ __forceinline__ void store(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};
template <>
struct Vec<1> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[1]) { v[0] = *p; }
  static __device__ __forceinline__ void store(float* p, const float (&v)[1]) { *p = v[0]; }
};

// 8 channels of one pixel as fp32 values, from / to bf16 (one 16-byte access) or fp32 (two).
__device__ __forceinline__ void ld8(const __bf16* p, float (&v)[8]) {
  const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
}
__device__ __forceinline__ void ld8(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void st8(__bf16* p, const float (&v)[8]) {
  bf16x8 t;
#pragma unroll
  for (int e = 0; e < 8; ++e) t[e] = (__bf16)v[e];
  *reinterpret_cast<bf16x8*>(p) = t;
}
__device__ __forceinline__ void st8(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// The norm-backward formula of one element.  With y = z*scale + shift, zhat = (z - mean)*invstd, a = act(y) as (leaky, slope):
//   gy = g*act'(y),  dz = scale*(gy - c1 - zhat*c2);  the sums are (sum gy, sum gy*zhat, sum over y < 0 of g*y)
// and with the perceptual taps of a peer pass (L1 between the two passes' z, y and a; coefficients cz, cy, ca):
//   g_a = g - ca*sign(a_peer - a),  gy = g_a*act'(y) - cy*sign(y_peer - y),  dz += -cz*sign(z_peer - z).
// Callers form y and zhat and keep their own accumulation statements (the order of the additions and the second sum's
// fused multiply-add are theirs); norm_bwd_gy holds nothing that `fp contract(off)` in a caller would change.
__device__ __forceinline__ float norm_bwd_gy(float g, float y, bool leaky, float slope) {
  return (leaky && y < 0.f) ? g * slope : g;
}

// gy with a peer; its two terms apart for the fp32 passes, whose slope-gradient sum needs g_a itself.
__device__ __forceinline__ float norm_bwd_ga_peer(float y, float yp, bool leaky, float slope, float ca) {
  const float ap = (leaky && yp < 0.f) ? yp * slope : yp;
  const float a = (leaky && y < 0.f) ? y * slope : y;
  return -ca * sgn(ap - a);
}
__device__ __forceinline__ float norm_bwd_gy_tap(float y, float yp, float cy) { return -cy * sgn(yp - y); }

__device__ __forceinline__ float norm_bwd_gy_peer(float g, float y, float yp, bool leaky, float slope, float cy,
                                                  float ca) {
  return norm_bwd_gy(g + norm_bwd_ga_peer(y, yp, leaky, slope, ca), y, leaky, slope) + norm_bwd_gy_tap(y, yp, cy);
}

__device__ __forceinline__ float norm_bwd_dz(float scale, float gy, float zhat, float c1, float c2) {
  return scale * (gy - c1 - zhat * c2);
}

// The peer's z tap, which bypasses the norm: added to norm_bwd_dz's value.
__device__ __forceinline__ float norm_bwd_dz_peer(float cz, float z, float zp) { return -cz * sgn(zp - z); }

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static inline bool any_misaligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (!aligned16(p)) return true;
  return false;
}

// Vec<4> serves channel counts and pitches % 4 == 0 on 16-byte aligned tensors (null: absent), Vec<1> everything else.
static inline bool vec4_rows(int c, std::initializer_list<int> pitches, std::initializer_list<const void*> ptrs) {
  if (c % 4) return false;
  for (int ld : pitches)
    if (ld % 4) return false;
  return !any_misaligned16(ptrs);
}

// Element-wise grid: blocks of R rows, four rows per thread and trip; x over a sample's P pixels (<= 4096 / n), y = n.
static inline dim3 ew_rows_grid(long P, int n, int R) {
  long gx = (P + 4L * R - 1) / (4L * R);
  const long cap = 4096 / n > 1 ? 4096 / n : 1;
  if (gx > cap) gx = cap;
  return dim3((unsigned)gx, (unsigned)n);
}

}  // namespace mpgan
