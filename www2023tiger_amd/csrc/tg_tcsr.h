// What the T-CSR maintenance kernels share (tg_append.hip, tg_trim.hip, tg_erase.hip; the host checks also serve
// tg_edge_rows.hip and tg_trend.hip).  The algorithms stay in their own files.
#pragma once
#include "tg_common.h"

namespace tg {

// first index i in [lo, hi) with a[i] > x (upper) / a[i] >= x (lower), else hi; a ascending
__device__ __forceinline__ int64_t upper_bound_i64(const int64_t* __restrict__ a, int64_t lo, int64_t hi, int64_t x) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ uint32_t upper_bound_u32(const uint32_t* a, uint32_t lo, uint32_t hi, uint32_t x) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t* a, uint32_t lo, uint32_t hi, uint32_t x) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// The rows a tile of entries [p0, p_last] spans.  owner(p) = (first v in [1, N) with indptr[v] > p, else N) - 1: a row of
// the graph whatever indptr holds.  The workgroup searches once for the owners lo, hi of its first and last entry (hi is
// galloped for from lo) and, if they are at most `cap` rows apart, stages indptr[lo + 1 .. hi] in the caller's LDS array
// `win` [cap]; a tile that spans more (thousands of empty rows) searches global memory.  All but owner() is block-uniform.
// The caller synchronises before the first owner() if `staged`: it may stage per-row values of its own beside the window.
struct RowWindow {
  const int64_t* indptr;
  const uint32_t* win;
  int64_t lo, hi;
  uint32_t nwin;  // min(hi - lo, cap + 1): the staged row bounds (a caller may stage nwin + 1 per-row values beside them)
  bool staged;
  // the owner of p: row lo + slot(p) of a staged window, searched(p) in global memory otherwise
  __device__ __forceinline__ uint32_t slot(int64_t p) const { return upper_bound_u32(win, 0u, nwin, (uint32_t)p); }
  __device__ __forceinline__ int64_t searched(int64_t p) const { return upper_bound_i64(indptr, lo + 1, hi + 1, p) - 1; }
  __device__ __forceinline__ int64_t owner(int64_t p) const { return staged ? lo + (int64_t)slot(p) : searched(p); }
};
template <int THREADS>
__device__ __forceinline__ RowWindow row_window(const int64_t* __restrict__ indptr, int64_t N, int64_t p0, int64_t p_last,
                                                uint32_t* win, int64_t cap) {
  RowWindow w{indptr, win};
  w.lo = upper_bound_i64(indptr, 1, N, p0) - 1;
  int64_t reach = 1;
  while (w.lo + reach < N && indptr[w.lo + reach] <= p_last) reach <<= 1;
  w.hi = upper_bound_i64(indptr, w.lo + 1, min(w.lo + reach + 1, N), p_last) - 1;
  w.nwin = (uint32_t)min(w.hi - w.lo, cap + 1);
  w.staged = w.hi - w.lo <= cap;
  if (w.staged)
    for (uint32_t i = threadIdx.x; i < w.nwin; i += THREADS) win[i] = (uint32_t)indptr[w.lo + 1 + i];
  return w;
}

// entry p of g becomes entry q of the output arrays
__device__ __forceinline__ void move_entry(const tg_tcsr& g, int64_t p, double* ts_out, int32_t* nbr_out, int32_t* eid_out,
                                           int64_t q) {
  ts_out[q] = g.ts[p];
  nbr_out[q] = g.nbr[p];
  eid_out[q] = g.eid[p];
}

// ---- host side, before the first launch: a graph with ids within 31 bits, fewer than 2^32 entries and no array missing
static inline int tcsr_args(const tg_tcsr* g) {
  if (!g || g->num_node <= 0 || g->num_node > 0x7fffffffLL || g->num_entry < 0 || g->num_entry > 0xffffffffLL || !g->indptr)
    return TG_EINVAL;
  if (g->num_entry > 0 && (!g->ts || !g->nbr || !g->eid)) return TG_EINVAL;
  return TG_OK;
}
// a workspace of at least `need` bytes (TG_EWORKSPACE), 16-byte aligned (TG_EINVAL)
static inline int ws_check(const void* ws, size_t ws_bytes, size_t need) {
  if (!ws || ws_bytes < need) return TG_EWORKSPACE;
  if (reinterpret_cast<uintptr_t>(ws) & 15) return TG_EINVAL;
  return TG_OK;
}

}  // namespace tg
