// Upper-bound searches over ascending row bounds: the owner of an entry of the T-CSR is an upper bound in indptr
// (tg_trim.hip: k_trim_apply, tg_erase.hip: k_erase_flags) - in global memory, or in a window staged in LDS.
#pragma once
#include "tg_common.h"

namespace tg {

// first index i in [lo, hi) with a[i] > x, else hi; a ascending
__device__ __forceinline__ int64_t upper_bound_i64(const int64_t* __restrict__ a, int64_t lo, int64_t hi, int64_t x) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ uint32_t upper_bound_lds(const uint32_t* a, uint32_t n, uint32_t x) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

}  // namespace tg
