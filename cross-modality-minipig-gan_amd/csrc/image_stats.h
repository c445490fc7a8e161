// What the streaming image statistics share (metric_ops.hip: the joint histogram; foreground.hip: Otsu's histogram and
// every chunked stream; mi_loss.hip: the value-range rules): the ONE fp32 bin rule, the ONE wave peel of the LDS
// counters, the ONE chunk planner and the ONE set of value-range refusals.
#pragma once
#include "mpgan_common.h"

namespace mpgan {

// idx = min((int)floorf((v - lo) * s), bins - 1) with s = (float)bins / (hi - lo) formed on the host: explicit
// round-to-nearest operations, so no contraction can change a bin.  For lo <= v <= hi.
__device__ __forceinline__ int hist_bin(float v, float lo, float s, int bins) {
  const int i = (int)floorf(__fmul_rn(__fsub_rn(v, lo), s));
  return i < bins - 1 ? i : bins - 1;
}

// One value per lane, called by every lane of the wave (pend = this lane has a counter to bump).  A wave whose lanes
// crowd one counter (the background bin of an MRI pair, a constant image) would serialise on an LDS atomic: up to
// ROUNDS times, the leading pending lane adds the number of lanes that share its counter in ONE atomic and all of them
// retire; lanes still pending after that issue their own.
template <int ROUNDS>
__device__ __forceinline__ void hist_submit(unsigned* lh, bool pend, unsigned key) {
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const unsigned long long act = __ballot(pend);
    if (act == 0ull) return;
    const int leader = __ffsll((long long)act) - 1;
    const unsigned lk = (unsigned)__shfl((int)key, leader, 64);
    const bool same = pend && key == lk;
    const unsigned long long m = __ballot(same);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&lh[lk], (unsigned)__popcll(m));
    pend = pend && !same;
  }
  if (pend) atomicAdd(&lh[key], 1u);
}

// How `groups` independent streams of n values each are cut into blocks' chunks: at least chunk_min values per chunk,
// about target_blocks blocks in all, at most 2^30 values per chunk (a block's uint32 counters cannot overflow).
struct StreamChunks {
  long chunks, per_chunk;                       // per stream; per_chunk is a multiple of 4: every chunk starts float4-aligned
};

inline StreamChunks stream_chunks(long n, long groups, long chunk_min, long target_blocks) {
  constexpr long CHUNK_MAX = 1L << 30;
  long cap = target_blocks / groups;
  if (cap < 1) cap = 1;
  long chunks = (n + chunk_min - 1) / chunk_min;
  if (chunks > cap) chunks = cap;
  const long floor_chunks = (n + CHUNK_MAX - 1) / CHUNK_MAX;
  if (chunks < floor_chunks) chunks = floor_chunks;
  if (chunks < 1) chunks = 1;
  StreamChunks c;
  c.chunks = chunks;
  c.per_chunk = (((n + chunks - 1) / chunks) + 3) & ~3L;
  return c;
}

// The refusals of a value range [lo, hi]; with s, also *s = (float)bins / (hi - lo) of hist_bin and the refusal of a
// range too narrow for it (Parzen windows do no fp32 binning and pass null).
inline int check_bin_range(const char* fn, float lo, float hi, int bins, float* s) {
  const float span = hi - lo;
  MPGAN_CHECK_ARG(is_finite(lo) && is_finite(hi) && is_finite(span), "%s: non-finite value range", fn);
  MPGAN_CHECK_ARG(hi > lo, "%s: value range needs hi > lo", fn);
  if (s) {
    *s = (float)bins / span;
    MPGAN_CHECK_ARG(is_finite(*s), "%s: value range too narrow for fp32 binning", fn);
  }
  return MPGAN_OK;
}

}  // namespace mpgan
