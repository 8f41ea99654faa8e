// The 64-bit orderable keys of the top-k selections and the sorted-across-the-lanes insertion, shared by tg_topk.hip
// (tg_topk_rows: selection over a score matrix) and tg_knn.hip (tg_knn_rows: selection on MFMA accumulators).
//   key = (order-preserving bits of the float32 score, -0.0 folded onto +0.0) << 32 | ~column
// A larger key is a better column - higher score first, equal scores by ascending column - and no two columns of a row
// share a key.  Key 0 is "nothing": a finite score's ordered bits are never 0.
#pragma once
#include "tg_common.h"

namespace tg {

__host__ __device__ __forceinline__ bool topk_finite(uint32_t u) { return (u & 0x7f800000u) != 0x7f800000u; }
__host__ __device__ __forceinline__ uint64_t topk_key(uint32_t u, uint32_t col) {
  if ((u << 1) == 0) u = 0;  // -0.0 ties +0.0
  const uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)o << 32) | (uint64_t)(uint32_t)~col;
}

__device__ __forceinline__ uint64_t lane_bcast(uint64_t v, int src) {
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, src), hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}

// best: lane p holds the p-th largest key met so far (0: none).  Inserts the lanes' keys that beat the one at lane kth.
__device__ __forceinline__ void topk_insert(uint64_t& best, uint64_t key, int kth, int lane) {
  uint64_t thr = lane_bcast(best, kth);
  unsigned long long todo = __ballot(key > thr);
  while (todo) {  // wave-uniform
    const int src = __builtin_amdgcn_readfirstlane(__ffsll(todo) - 1);
    todo &= todo - 1;
    const uint64_t x = lane_bcast(key, src);
    if (x > thr) {  // the threshold has risen since the ballot
      const uint64_t up = __shfl_up(best, 1);
      if (best < x) best = (lane == 0 || up > x) ? x : up;
      thr = lane_bcast(best, kth);
    }
  }
}

}  // namespace tg
