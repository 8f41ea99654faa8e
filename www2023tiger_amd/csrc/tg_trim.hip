// Sliding-window expiry of the T-CSR (online serving; reference tiger/data/graph.py:11-42: the reference builds its adjacency
// lists once over the whole stream and never drops an entry - it has no counterpart of this).
//
// Every row of the T-CSR is ascending in time, so both forms of expiry keep a SUFFIX of every row.  Per node v with old row
// [b, e):  s = max(b, first p in [b, e) with ts[p] >= t_cut, e - keep_last);  kept row = [s, e).  The cut is
// prefix_end_group (tg_sample.h) - the float64 '<' of the samplers, so trimming and sampling agree on every boundary.
//   plan A (k_trim_plan_rows, one workgroup per 256 nodes): s and the kept length per node (with a horizon: 16 lanes per
//           node search the cut together, sixteen nodes per round; with a cap alone: one thread per node, no search), an
//           exclusive scan of the lengths inside the workgroup, one total per workgroup.
//   plan B (k_trim_plan_ptr, the same grid): workgroup b sums the b totals in front of it (block_sum_front: no third
//           scan launch), writes indptr_out (indptr_out[num_node] = kept entries) and turns the row starts into
//           shift[v] = s_v - indptr_out[v] >= 0, non-decreasing in v.
//   apply  (k_trim_apply, one workgroup per 2048 KEPT entries): lane l takes kept entry q = base + l, its owner is an
//           upper bound in indptr_out, its old position q + shift[owner].  The workgroup searches once for the owners of
//           its first and last entry and stages that window of indptr_out (row_window, tg_tcsr.h) and shift in LDS (up to
//           TR_WIN rows; a tile that spans more - tens of thousands of empty rows - searches global memory).  Loads and
//           stores coalesce whatever was dropped, and a hub row is spread over as many workgroups as it has tiles.
// No atomics (the result does not depend on the launch geometry), no grid is capped (every workgroup owns one chunk / tile),
// integer work and one float64 comparison: device, host twin and numpy agree bit for bit.
#include <algorithm>
#include <cmath>

#include "tg_sample.h"
#include "tg_tcsr.h"
#include "tg_step.h"

namespace tg {

constexpr int TR_THREADS = TG_SCAN_BLOCK;       // nodes per workgroup of the plan (block_excl_scan: 256)
constexpr int TR_ITEMS = 8;
constexpr int TR_TILE = TR_THREADS * TR_ITEMS;  // kept entries per copy workgroup
constexpr int TR_WIN = 2048;                    // rows of one copy tile staged in LDS (more: searched in global memory)

template <bool HORIZON>
__global__ void __launch_bounds__(TR_THREADS) k_trim_plan_rows(tg_tcsr g, double t_cut, int64_t keep,
                                                               uint32_t* __restrict__ start, uint32_t* __restrict__ rank,
                                                               uint32_t* __restrict__ blk) {
  __shared__ uint32_t s_w[TR_THREADS / TG_WAVE];
  __shared__ uint32_t s_cut[TR_THREADS];
  const int t = threadIdx.x;
  const int64_t v0 = (int64_t)blockIdx.x * TR_THREADS;
  if (HORIZON) {
    const int sub = t % 16, grp = t / 16;
#pragma unroll 1
    for (int it = 0; it < TR_THREADS / 16; ++it) {  // block-uniform trip count: the ballots see whole wavefronts
      const int slot = it * 16 + grp;
      const int64_t v = v0 + slot;
      int64_t b;
      const int64_t cut = prefix_end_group<16>(g, v < g.num_node ? v : (int64_t)-1, t_cut, &b, sub);
      if (sub == 0) s_cut[slot] = (uint32_t)cut;
    }
    __syncthreads();
  }
  const int64_t v = v0 + t;
  uint32_t len = 0;
  if (v < g.num_node) {
    const int64_t b = g.indptr[v], e = g.indptr[v + 1];
    int64_t s = b;
    if (HORIZON) s = max(s, (int64_t)s_cut[t]);
    if (e - b > keep) s = max(s, e - keep);
    len = (uint32_t)(e - s);
    start[v] = (uint32_t)s;
  }
  uint32_t total;
  const uint32_t r = block_excl_scan(len, s_w, &total);
  if (v < g.num_node) rank[v] = r;
  if (t == 0) blk[blockIdx.x] = total;
}

// workgroup b: the chunk of workgroup b of k_trim_plan_rows.  `shift` holds the row starts on entry.
__global__ void __launch_bounds__(TR_THREADS) k_trim_plan_ptr(int64_t num_node, uint32_t* __restrict__ shift,
                                                              const uint32_t* __restrict__ rank,
                                                              const uint32_t* __restrict__ blk,
                                                              int64_t* __restrict__ indptr_out) {
  __shared__ uint32_t s_w[TR_THREADS / TG_WAVE];
  const uint32_t base = block_sum_front(blk, blockIdx.x, s_w);  // kept entries in front of this chunk
  const int64_t v = (int64_t)blockIdx.x * TR_THREADS + threadIdx.x;
  if (v < num_node) {
    const uint32_t o = base + rank[v];
    indptr_out[v] = (int64_t)o;
    shift[v] -= o;
  }
  if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1) indptr_out[num_node] = (int64_t)base + (int64_t)blk[blockIdx.x];
}

struct TrimApplyArgs {
  tg_tcsr g;
  const int64_t* indptr_out;
  const uint32_t* shift;
  int64_t P;  // kept entries
  double* ts_out;
  int32_t *nbr_out, *eid_out;
};
__global__ void __launch_bounds__(TR_THREADS) k_trim_apply(TrimApplyArgs a) {
  __shared__ uint32_t win[TR_WIN];     // indptr_out[lo + 1 .. hi]: where the rows after the first one begin
  __shared__ uint32_t sh[TR_WIN + 1];  // shift[lo .. hi]
  const uint32_t t = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * TR_TILE, q1 = min(q0 + TR_TILE, a.P);
  const RowWindow w = row_window<TR_THREADS>(a.indptr_out, a.g.num_node, q0, q1 - 1, win, TR_WIN);
  if (w.staged) {
    for (uint32_t i = t; i <= w.nwin; i += TR_THREADS) sh[i] = a.shift[w.lo + i];
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < TR_ITEMS; ++i) {
    const int64_t q = q0 + (int64_t)i * TR_THREADS + t;  // lane l takes entry base + l: loads and stores coalesce
    if (q >= q1) break;
    uint32_t s;
    if (w.staged) s = sh[w.slot(q)];
    else s = a.shift[w.searched(q)];
    const int64_t p = q + (int64_t)s;
    if (p >= a.g.num_entry) continue;  // (an indptr_out that is no plan of this graph: nothing is read out of bounds)
    move_entry(a.g, p, a.ts_out, a.nbr_out, a.eid_out, q);
  }
}

struct TrimLayout {
  size_t shift, rank, blk, total;
};
static TrimLayout trim_layout(int64_t num_node) {
  TrimLayout l{};
  l.shift = 0;
  l.rank = l.shift + align16((size_t)num_node * sizeof(uint32_t));
  l.blk = l.rank + align16((size_t)num_node * sizeof(uint32_t));
  l.total = l.blk + align16((size_t)cdiv(num_node, TR_THREADS) * sizeof(uint32_t));
  return l;
}

}  // namespace tg

using namespace tg;

extern "C" size_t tg_tcsr_trim_workspace_bytes(int64_t num_node) {
  if (num_node <= 0 || num_node > 0x7fffffffLL) return 0;
  return trim_layout(num_node).total;
}

extern "C" int tg_tcsr_trim_plan(const tg_tcsr* g, double t_cut, int64_t keep_last, int64_t* indptr_out, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (int rc = tcsr_args(g)) return rc;
  if (!indptr_out || std::isnan(t_cut)) return TG_EINVAL;
  const TrimLayout l = trim_layout(g->num_node);
  if (int rc = ws_check(ws, ws_bytes, l.total)) return rc;  // before the first launch
  hipStream_t st = as_stream(stream);
  char* base = static_cast<char*>(ws);
  uint32_t* shift = reinterpret_cast<uint32_t*>(base + l.shift);
  uint32_t* rank = reinterpret_cast<uint32_t*>(base + l.rank);
  uint32_t* blk = reinterpret_cast<uint32_t*>(base + l.blk);
  const int64_t keep = keep_last < 0 || keep_last > g->num_entry ? g->num_entry : keep_last;  // (off: no row is longer)
  const dim3 grid((unsigned)cdiv(g->num_node, TR_THREADS));
  if (t_cut > -INFINITY)
    hipLaunchKernelGGL(k_trim_plan_rows<true>, grid, dim3(TR_THREADS), 0, st, *g, t_cut, keep, shift, rank, blk);
  else
    hipLaunchKernelGGL(k_trim_plan_rows<false>, grid, dim3(TR_THREADS), 0, st, *g, t_cut, keep, shift, rank, blk);
  hipLaunchKernelGGL(k_trim_plan_ptr, grid, dim3(TR_THREADS), 0, st, g->num_node, shift, rank, blk, indptr_out);
  return check_launch("tg_tcsr_trim_plan");
}

extern "C" int tg_tcsr_trim_apply(const tg_tcsr* g, const int64_t* indptr_out, int64_t num_entry_out, double* ts_out,
                                  int32_t* nbr_out, int32_t* eid_out, const void* ws, size_t ws_bytes, void* stream) {
  if (int rc = tcsr_args(g)) return rc;
  if (!indptr_out || num_entry_out < 0 || num_entry_out > g->num_entry) return TG_EINVAL;
  if (num_entry_out > 0 && (!ts_out || !nbr_out || !eid_out)) return TG_EINVAL;
  const TrimLayout l = trim_layout(g->num_node);
  if (int rc = ws_check(ws, ws_bytes, l.total)) return rc;
  if (num_entry_out == 0) return TG_OK;
  TrimApplyArgs a{*g, indptr_out, reinterpret_cast<const uint32_t*>(static_cast<const char*>(ws) + l.shift), num_entry_out,
                  ts_out, nbr_out, eid_out};
  hipLaunchKernelGGL(k_trim_apply, dim3((unsigned)cdiv(num_entry_out, TR_TILE)), dim3(TR_THREADS), 0, as_stream(stream), a);
  return check_launch("tg_tcsr_trim_apply");
}

// The host twin: plain C++ over host pointers.
extern "C" int tg_tcsr_trim_host(const tg_tcsr* g, double t_cut, int64_t keep_last, int64_t* indptr_out, double* ts_out,
                                 int32_t* nbr_out, int32_t* eid_out, int64_t* num_entry_out) {
  if (int rc = tcsr_args(g)) return rc;
  if (!indptr_out || !num_entry_out || std::isnan(t_cut)) return TG_EINVAL;
  if (g->num_entry > 0 && (!ts_out || !nbr_out || !eid_out)) return TG_EINVAL;
  int64_t q = 0;
  for (int64_t v = 0; v < g->num_node; ++v) {
    const int64_t b = g->indptr[v], e = g->indptr[v + 1];
    int64_t s = std::lower_bound(g->ts + b, g->ts + e, t_cut) - g->ts;  // first entry with ts >= t_cut (ts < t_cut: dropped)
    if (keep_last >= 0 && e - b > keep_last) s = std::max(s, e - keep_last);
    indptr_out[v] = q;
    std::copy(g->ts + s, g->ts + e, ts_out + q);
    std::copy(g->nbr + s, g->nbr + e, nbr_out + q);
    std::copy(g->eid + s, g->eid + e, eid_out + q);
    q += e - s;
  }
  indptr_out[g->num_node] = q;
  *num_entry_out = q;
  return TG_OK;
}
