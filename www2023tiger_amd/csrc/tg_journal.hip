// Incremental online state files (TIGE.journal / apply_online_delta; DESIGN 7.23.  The reference - tiger.py, memory.py,
// graph.py:11-42 - rebuilds graph, mailbox and tables from the data set and never saves a served model: it has no
// counterpart of anything here).
//
// pack    The listed rows of a T-CSR, one after the other.  rows [D] int32, ascending and distinct.
//   plan  (k_jp_len, one workgroup per tile of 2048 listed rows): a thread takes 8 consecutive rows, their lengths are
//          scanned inside the workgroup; off[j] = entries of the tile in front of row j, one total per tile.  A single
//          tile is final at once; otherwise k_jp_off (the same grid) adds the totals of the tiles in front
//          (block_sum_front: no third scan launch).  off[D] = the packed length: the ONE read-back.
//   apply (k_jp_apply, one workgroup per 2048 PACKED entries): lane l takes packed entry q = base + l; its owner is an
//          upper bound in off, staged through row_window (tg_tcsr.h) beside shift[j] = indptr[rows[j]] - off[j]; its
//          source is q + shift.  A hub row is spread over as many workgroups as it has tiles.
// splice  A new T-CSR over N_new >= num_node ids: row rows[j] is pack row j, every other row the old one (empty for ids
//          at and beyond the old num_node).
//   plan  k_js_check (one thread per listed row: rows strictly ascending inside [0, N_new); off[0] == 0, non-decreasing,
//          off[D] == the packed length), k_js_len (one workgroup per 256 NEW ids: the id is looked for in `rows` by a
//          binary search, its length and source start follow; a scan inside the workgroup), k_js_ptr (the same grid:
//          indptr_out and, per id, enc = 2 (source start - indptr_out[v]) | from-pack), k_js_result (one thread):
//          out3 = {num_entry_new, error class, smallest offender} - the one read-back.
//   apply (k_js_apply, one workgroup per 2048 NEW entries): the owner through row_window over indptr_out, enc staged
//          beside it; the entry is read from the old arrays or from the pack.  Rows are distinct: every new entry has one
//          writer.
// A loaded row id, offset or row bound is range-checked before it is used as an index; an error is folded with a 64-bit
// atomicMin per class (only offenders issue one), so the smallest offender is named whatever the launch geometry.  The
// copies use no atomics.  Entries move as 8- and 4-byte elements, consecutive lanes on consecutive entries (as tg_trim.hip,
// tg_erase.hip): source and destination of a row differ in alignment row by row.
// scatter (k_jr_scatter, ONE launch for up to 8 tables): dst[ids[j]] = src[j], the inverse of k_nc_rows
//          (tg_node_compact.hip).  Rows of a multiple of 16 bytes: a tile of whole INPUT rows, about 4096 16-byte pieces,
//          their ids staged in LDS, contiguous 16-byte loads, four in flight per lane, 16-byte stores.  Rows of 8, 4 or 1
//          bytes: 2048 rows per tile.  Every id is checked against the destination's rows before the store.
// bits    (k_jr_bits): bit ids[j] = (bytes[j] != 0).  Neighbouring ids share a word: one 64-bit atomicOr / atomicAnd per
//          id (as tg_bitmap_mark); ids are distinct, so the result does not depend on the order.
// Integer work and bit copies only: device, host twin and numpy agree bit for bit.
#include <algorithm>
#include <cstring>

#include "tg_step.h"
#include "tg_tcsr.h"

namespace tg {

constexpr int JR_THREADS = TG_SCAN_BLOCK;  // block_excl_scan: 256
constexpr int JR_ITEMS = 8;
constexpr int JR_TILE = JR_THREADS * JR_ITEMS;  // listed rows per plan tile, entries per copy tile
constexpr int JR_WIN = 2048;                    // rows of one copy tile staged in LDS (more: searched in global memory)
constexpr int JR_TILE_F4 = 4096;                // 16-byte pieces per wide scatter tile
constexpr int JR_TILE_ROWS = 2048;              // most rows of one scatter tile (their ids: 8 KiB of LDS)
constexpr int JR_BATCH = 4;                     // independent 16-byte loads in flight per lane
constexpr unsigned long long JR_NONE = ~0ull;   // an error word nobody lowered
constexpr int64_t JR_NOWHERE = -(1ll << 62);    // a shift that lands outside every array

__device__ __forceinline__ int64_t clamp_i64(int64_t x, int64_t lo, int64_t hi) { return min(max(x, lo), hi); }

// first index j in [0, n) with a[j] >= x, else n; a ascending
__device__ __forceinline__ int64_t lower_bound_i32(const int32_t* __restrict__ a, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if ((int64_t)a[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- pack ----------------------------------------------------------------------------------------------------------------
// the length of listed row j (0 for a row id that is no node); *start = where it begins in g
__device__ __forceinline__ uint32_t jp_row(const tg_tcsr& g, const int32_t* __restrict__ rows, int64_t j, int64_t* start) {
  const int64_t v = (int64_t)rows[j];
  *start = 0;
  if (v < 0 || v >= g.num_node) return 0u;
  const int64_t b = clamp_i64(g.indptr[v], 0, g.num_entry), e = clamp_i64(g.indptr[v + 1], 0, g.num_entry);
  *start = b;
  return e > b ? (uint32_t)(e - b) : 0u;
}

__global__ void __launch_bounds__(JR_THREADS) k_jp_len(tg_tcsr g, const int32_t* __restrict__ rows, int64_t D,
                                                       int64_t* __restrict__ off, uint32_t* __restrict__ blk) {
  __shared__ uint32_t s_w[JR_THREADS / TG_WAVE];
  const int64_t j0 = (int64_t)blockIdx.x * JR_TILE + (int64_t)threadIdx.x * JR_ITEMS;  // thread order is row order
  uint32_t len[JR_ITEMS];
  uint32_t mine = 0;
#pragma unroll
  for (int i = 0; i < JR_ITEMS; ++i) {
    int64_t b;
    len[i] = j0 + i < D ? jp_row(g, rows, j0 + i, &b) : 0u;
    mine += len[i];
  }
  uint32_t total;
  uint32_t r = block_excl_scan(mine, s_w, &total);
#pragma unroll
  for (int i = 0; i < JR_ITEMS; ++i) {
    if (j0 + i < D) off[j0 + i] = (int64_t)r;
    r += len[i];
  }
  if (threadIdx.x == 0) {
    blk[blockIdx.x] = total;
    if (gridDim.x == 1) off[D] = (int64_t)total;  // a single tile: final
  }
}

__global__ void __launch_bounds__(JR_THREADS) k_jp_off(int64_t D, int64_t* __restrict__ off, const uint32_t* __restrict__ blk) {
  __shared__ uint32_t s_w[JR_THREADS / TG_WAVE];
  const uint32_t front = block_sum_front(blk, blockIdx.x, s_w);  // packed entries in front of this tile (< 2^32)
  const int64_t j0 = (int64_t)blockIdx.x * JR_TILE + (int64_t)threadIdx.x * JR_ITEMS;
#pragma unroll
  for (int i = 0; i < JR_ITEMS; ++i)
    if (j0 + i < D) off[j0 + i] += (int64_t)front;
  if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1) off[D] = (int64_t)front + (int64_t)blk[blockIdx.x];
}

struct JpApplyArgs {
  tg_tcsr g;
  const int32_t* rows;
  int64_t D;
  const int64_t* off;
  int64_t P;  // packed entries
  double* ts_out;
  int32_t *nbr_out, *eid_out;
};
// where packed row j begins in g, minus off[j]
__device__ __forceinline__ int64_t jp_shift(const JpApplyArgs& a, int64_t j) {
  const int64_t v = (int64_t)a.rows[j];
  if (v < 0 || v >= a.g.num_node) return JR_NOWHERE;
  return a.g.indptr[v] - a.off[j];
}
__global__ void __launch_bounds__(JR_THREADS) k_jp_apply(JpApplyArgs a) {
  __shared__ uint32_t win[JR_WIN];     // off[lo + 1 .. hi]: where the packed rows after the first one begin
  __shared__ int64_t sh[JR_WIN + 1];   // shift[lo .. hi]
  const uint32_t t = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * JR_TILE, q1 = min(q0 + JR_TILE, a.P);
  const RowWindow w = row_window<JR_THREADS>(a.off, a.D, q0, q1 - 1, win, JR_WIN);
  if (w.staged) {
    for (uint32_t i = t; i <= w.nwin; i += JR_THREADS) sh[i] = jp_shift(a, w.lo + i);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < JR_ITEMS; ++i) {
    const int64_t q = q0 + (int64_t)i * JR_THREADS + t;  // lane l takes entry base + l: loads and stores coalesce
    if (q >= q1) break;
    const int64_t p = q + (w.staged ? sh[w.slot(q)] : jp_shift(a, w.searched(q)));
    if (p < 0 || p >= a.g.num_entry) continue;  // (an off that is no plan of these rows: nothing is read out of bounds)
    move_entry(a.g, p, a.ts_out, a.nbr_out, a.eid_out, q);
  }
}

static int jp_args(const tg_tcsr* g, const int32_t* rows, int64_t D, const int64_t* off) {
  if (int rc = tcsr_args(g)) return rc;
  if (D < 0 || D > g->num_node || !off || (D > 0 && !rows)) return TG_EINVAL;
  return TG_OK;
}
static size_t jp_ws_bytes(int64_t D) { return align16((size_t)std::max<int64_t>(cdiv(D, JR_TILE), 1) * sizeof(uint32_t)); }

// ---- splice --------------------------------------------------------------------------------------------------------------
struct JsArgs {
  tg_tcsr g;
  int64_t N_new;
  const int32_t* rows;
  int64_t D;
  const int64_t* off;
  int64_t n_pack;
  int64_t* indptr_out;
  int64_t* enc;              // [N_new] 2 (source start - indptr_out[v]) | from-pack; the source start itself after k_js_len
  uint32_t* rank;            // [N_new]
  uint32_t* blk;             // [ceil(N_new / 256)]
  unsigned long long* errs;  // [3] the smallest offender per class, JR_NONE without one
  int64_t* total;            // [1]
  int64_t* out3;
};

__global__ void __launch_bounds__(JR_THREADS) k_js_check(JsArgs a) {
  const int64_t j = (int64_t)blockIdx.x * JR_THREADS + threadIdx.x;
  if (j > a.D) return;
  if (j < a.D) {
    const int64_t r = (int64_t)a.rows[j];
    if (r < 0 || r >= a.N_new || (j > 0 && (int64_t)a.rows[j - 1] >= r)) atomicMin(a.errs + 0, (unsigned long long)j);
    if (a.off[j + 1] < a.off[j]) atomicMin(a.errs + 1, (unsigned long long)(j + 1));
  }
  if (j == 0 && a.off[0] != 0) atomicMin(a.errs + 1, 0ull);
  if (j == a.D && a.off[a.D] != a.n_pack) atomicMin(a.errs + 1, (unsigned long long)a.D);
}

__global__ void __launch_bounds__(JR_THREADS) k_js_len(JsArgs a) {
  __shared__ uint32_t s_w[JR_THREADS / TG_WAVE];
  const int64_t v = (int64_t)blockIdx.x * JR_THREADS + threadIdx.x;
  uint32_t len = 0;
  if (v < a.N_new) {
    int64_t start = 0, pack = 0;
    if (v < a.g.num_node) {
      const int64_t b = a.g.indptr[v], e = a.g.indptr[v + 1];
      if (b < 0 || e < b || e > a.g.num_entry) atomicMin(a.errs + 2, (unsigned long long)v);
      else {
        len = (uint32_t)(e - b);
        start = b;
      }
    }
    const int64_t j = lower_bound_i32(a.rows, a.D, v);
    if (j < a.D && (int64_t)a.rows[j] == v) {
      const int64_t o0 = a.off[j], o1 = a.off[j + 1];
      const bool ok = o0 >= 0 && o1 >= o0 && o1 <= a.n_pack;  // (else k_js_check has reported it)
      len = ok ? (uint32_t)(o1 - o0) : 0u;
      start = ok ? o0 : 0;
      pack = 1;
    }
    a.enc[v] = start * 2 + pack;
  }
  uint32_t total;
  const uint32_t r = block_excl_scan(len, s_w, &total);
  if (v < a.N_new) a.rank[v] = r;
  if (threadIdx.x == 0) a.blk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(JR_THREADS) k_js_ptr(JsArgs a) {
  __shared__ uint32_t s_w[JR_THREADS / TG_WAVE];
  const uint32_t base = block_sum_front(a.blk, blockIdx.x, s_w);  // new entries in front of this chunk
  const int64_t v = (int64_t)blockIdx.x * JR_THREADS + threadIdx.x;
  if (v < a.N_new) {
    const int64_t o = (int64_t)(base + a.rank[v]);
    a.indptr_out[v] = o;
    const int64_t e = a.enc[v];
    a.enc[v] = ((e >> 1) - o) * 2 + (e & 1);
  }
  if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1) {
    const int64_t total = (int64_t)base + (int64_t)a.blk[blockIdx.x];
    a.indptr_out[a.N_new] = total;
    a.total[0] = total;
  }
}

__global__ void k_js_result(JsArgs a) {
  if (threadIdx.x || blockIdx.x) return;
  int64_t cls = 0, first = -1;
  for (int c = 2; c >= 0; --c)
    if (a.errs[c] != JR_NONE) {
      cls = c + 1;
      first = (int64_t)a.errs[c];
    }
  a.out3[0] = a.total[0];
  a.out3[1] = cls;
  a.out3[2] = first;
}

struct JsApplyArgs {
  tg_tcsr g;
  int64_t N_new;
  const int64_t* indptr_out;
  const int64_t* enc;
  int64_t P;  // new entries
  int64_t n_pack;
  const double* ts_pack;
  const int32_t *nbr_pack, *eid_pack;
  double* ts_out;
  int32_t *nbr_out, *eid_out;
};
__global__ void __launch_bounds__(JR_THREADS) k_js_apply(JsApplyArgs a) {
  __shared__ uint32_t win[JR_WIN];    // indptr_out[lo + 1 .. hi]
  __shared__ int64_t sh[JR_WIN + 1];  // enc[lo .. hi]
  const uint32_t t = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * JR_TILE, q1 = min(q0 + JR_TILE, a.P);
  const RowWindow w = row_window<JR_THREADS>(a.indptr_out, a.N_new, q0, q1 - 1, win, JR_WIN);
  if (w.staged) {
    for (uint32_t i = t; i <= w.nwin; i += JR_THREADS) sh[i] = a.enc[w.lo + i];
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < JR_ITEMS; ++i) {
    const int64_t q = q0 + (int64_t)i * JR_THREADS + t;
    if (q >= q1) break;
    const int64_t e = w.staged ? sh[w.slot(q)] : a.enc[w.searched(q)];
    const int64_t p = q + (e >> 1);
    if (e & 1) {  // (a workspace that is no plan of these arrays: nothing is read out of bounds)
      if (p < 0 || p >= a.n_pack) continue;
      a.ts_out[q] = a.ts_pack[p];
      a.nbr_out[q] = a.nbr_pack[p];
      a.eid_out[q] = a.eid_pack[p];
    } else {
      if (p < 0 || p >= a.g.num_entry) continue;
      move_entry(a.g, p, a.ts_out, a.nbr_out, a.eid_out, q);
    }
  }
}

struct JsLayout {
  size_t enc, rank, blk, errs, total_word, total;
};
static JsLayout js_layout(int64_t N_new) {
  JsLayout l{};
  l.enc = 0;
  l.rank = l.enc + align16((size_t)N_new * sizeof(int64_t));
  l.blk = l.rank + align16((size_t)N_new * sizeof(uint32_t));
  l.errs = l.blk + align16((size_t)cdiv(N_new, JR_THREADS) * sizeof(uint32_t));
  l.total_word = l.errs + 4 * sizeof(uint64_t);
  l.total = l.total_word + 16;
  return l;
}
static int js_args(const tg_tcsr* g, int64_t N_new, const int32_t* rows, int64_t D, const int64_t* off, int64_t n_pack) {
  if (int rc = tcsr_args(g)) return rc;
  if (N_new < g->num_node || N_new > 0x7fffffffLL || D < 0 || D > N_new || !off || (D > 0 && !rows)) return TG_EINVAL;
  if (n_pack < 0 || g->num_entry + n_pack > 0xffffffffLL) return TG_EINVAL;  // (no partial sum of the scan wraps)
  return TG_OK;
}

// ---- scatter -------------------------------------------------------------------------------------------------------------
struct JrScatArgs {
  tg_node_rows tab[TG_NODE_ROWS_MAX];
  uint32_t tile0[TG_NODE_ROWS_MAX + 1];  // the first workgroup of every table; [n_tab] = the grid
  uint32_t tile_rows[TG_NODE_ROWS_MAX];
  const int32_t* ids;
  int32_t n_tab;
};

template <typename T>
__device__ __forceinline__ void jr_scatter_narrow(const tg_node_rows& d, const int32_t* __restrict__ ids, int64_t row0) {
  const T* __restrict__ src = static_cast<const T*>(d.src);
  T* __restrict__ dst = static_cast<T*>(d.dst);
  const int64_t end = min(row0 + JR_TILE, d.n_rows_src);
#pragma unroll
  for (int i = 0; i < JR_ITEMS; ++i) {
    const int64_t j = row0 + (int64_t)i * JR_THREADS + threadIdx.x;
    if (j >= end) continue;
    const int32_t o = ids[j];
    if ((uint32_t)o < (uint64_t)d.n_rows_out) dst[o] = src[j];  // (an id that is no row of this table stores nothing)
  }
}

__global__ void __launch_bounds__(JR_THREADS) k_jr_scatter(JrScatArgs a) {
  __shared__ int32_t s_id[JR_TILE_ROWS];
  int tb = 0;  // (block-uniform) the table of this workgroup
#pragma unroll
  for (int i = 1; i < TG_NODE_ROWS_MAX; ++i)
    if (i < a.n_tab && blockIdx.x >= a.tile0[i]) tb = i;
  const tg_node_rows d = a.tab[tb];
  const int64_t row0 = (int64_t)(blockIdx.x - a.tile0[tb]) * a.tile_rows[tb];
  if (d.row_bytes == 8) return jr_scatter_narrow<uint64_t>(d, a.ids, row0);
  if (d.row_bytes == 4) return jr_scatter_narrow<uint32_t>(d, a.ids, row0);
  if (d.row_bytes == 1) return jr_scatter_narrow<uint8_t>(d, a.ids, row0);
  const uint32_t t = threadIdx.x;
  const uint32_t d4 = (uint32_t)(d.row_bytes / 16);
  const uint32_t rows = (uint32_t)min((int64_t)a.tile_rows[tb], d.n_rows_src - row0);
  for (uint32_t i = t; i < rows; i += JR_THREADS) {
    const int32_t o = a.ids[row0 + i];
    s_id[i] = (uint32_t)o < (uint64_t)d.n_rows_out ? o : -1;
  }
  __syncthreads();
  const uint64_t nf = (uint64_t)rows * d4;  // 16-byte pieces of the tile, swept in input order
  const float4* __restrict__ src = static_cast<const float4*>(d.src) + row0 * (int64_t)d4;
  float4* __restrict__ dst = static_cast<float4*>(d.dst);
  const uint32_t q_step = JR_THREADS / d4, r_step = JR_THREADS % d4;
  uint32_t row = t / d4, col = t % d4;  // of piece f = t; both advance by the step of JR_THREADS
  for (uint64_t f = t; f < nf; f += (uint64_t)JR_BATCH * JR_THREADS) {
    // (the loads stay unconditional: a piece past the tile's end reads piece 0 of the tile and is not stored)
    int64_t where[JR_BATCH];
    float4 v[JR_BATCH];
#pragma unroll
    for (int i = 0; i < JR_BATCH; ++i) {
      const uint64_t fi = f + (uint64_t)i * JR_THREADS;
      const int32_t o = s_id[min(row, rows - 1u)];
      where[i] = fi < nf && o >= 0 ? (int64_t)o * d4 + col : (int64_t)-1;
      v[i] = src[fi < nf ? fi : 0];
      row += q_step;
      col += r_step;
      if (col >= d4) {
        col -= d4;
        ++row;
      }
    }
#pragma unroll
    for (int i = 0; i < JR_BATCH; ++i)
      if (where[i] >= 0) dst[where[i]] = v[i];
  }
}

// everything the device entry and the host twin refuse; wide rows also want 16-byte aligned tables when `aligned`
static int jr_scatter_args(const tg_node_rows* tabs, int32_t n_tab, const int32_t* ids, int64_t n_ids, bool aligned) {
  if (n_tab < 0 || n_tab > TG_NODE_ROWS_MAX || (n_tab > 0 && !tabs) || n_ids < 0 || n_ids > 0x7fffffffLL) return TG_EINVAL;
  for (int i = 0; i < n_tab; ++i) {
    const tg_node_rows& d = tabs[i];
    const bool wide = d.row_bytes >= 16 && d.row_bytes % 16 == 0;
    if (!wide && d.row_bytes != 8 && d.row_bytes != 4 && d.row_bytes != 1) return TG_EINVAL;
    if (d.row_bytes > (1 << 20) || d.n_rows_src < 0 || d.n_rows_src > n_ids || d.n_rows_out < 1 || d.n_rows_out > 0x7fffffffLL)
      return TG_EINVAL;
    if (d.n_rows_src == 0) continue;
    if (!d.src || !d.dst || !ids) return TG_EINVAL;
    const uintptr_t s = reinterpret_cast<uintptr_t>(d.src), o = reinterpret_cast<uintptr_t>(d.dst);
    if (aligned && wide && ((s | o) & 15)) return TG_EINVAL;
    if (s < o + (uintptr_t)(d.n_rows_out * d.row_bytes) && o < s + (uintptr_t)(d.n_rows_src * d.row_bytes)) return TG_EINVAL;
  }
  return TG_OK;
}

// ---- bits ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(JR_THREADS) k_jr_bits(const uint8_t* __restrict__ bytes, const int32_t* __restrict__ ids,
                                                        int64_t n, uint64_t* __restrict__ bits, int64_t n_ids) {
  for (int64_t j = (int64_t)blockIdx.x * JR_THREADS + threadIdx.x; j < n; j += (int64_t)gridDim.x * JR_THREADS) {
    const int64_t id = (int64_t)ids[j];
    if (id < 0 || id >= n_ids) continue;  // (an id that is no bit of this bitmap stores nothing)
    const unsigned long long bit = 1ull << (id & 63);
    unsigned long long* w = reinterpret_cast<unsigned long long*>(bits + (id >> 6));
    if (bytes[j]) atomicOr(w, bit);
    else atomicAnd(w, ~bit);
  }
}

static int jr_bits_args(const uint8_t* bytes, const int32_t* ids, int64_t n, const uint64_t* bits, int64_t n_ids) {
  if (n < 0 || n > 0x7fffffffLL || n_ids < 1 || n_ids > 0x7fffffffLL || !bits) return TG_EINVAL;
  if (n > 0 && (!bytes || !ids)) return TG_EINVAL;
  return TG_OK;
}

}  // namespace tg

using namespace tg;

extern "C" size_t tg_tcsr_rows_pack_workspace_bytes(int64_t D) {
  if (D < 0 || D > 0x7fffffffLL) return 0;
  return jp_ws_bytes(D);
}

extern "C" int tg_tcsr_rows_pack_plan(const tg_tcsr* g, const int32_t* rows, int64_t D, int64_t* off, void* ws, size_t ws_bytes,
                                      void* stream) {
  if (int rc = jp_args(g, rows, D, off)) return rc;
  if (int rc = ws_check(ws, ws_bytes, jp_ws_bytes(D))) return rc;  // before the first launch
  hipStream_t st = as_stream(stream);
  if (D == 0) {
    if (hipError_t e = hipMemsetAsync(off, 0, sizeof(int64_t), st)) {
      set_hip_error(e, "tg_tcsr_rows_pack_plan");
      return TG_EHIP;
    }
    return TG_OK;
  }
  uint32_t* blk = static_cast<uint32_t*>(ws);
  const dim3 grid((unsigned)cdiv(D, JR_TILE));
  hipLaunchKernelGGL(k_jp_len, grid, dim3(JR_THREADS), 0, st, *g, rows, D, off, blk);
  if (grid.x > 1) hipLaunchKernelGGL(k_jp_off, grid, dim3(JR_THREADS), 0, st, D, off, (const uint32_t*)blk);
  return check_launch("tg_tcsr_rows_pack_plan");
}

extern "C" int tg_tcsr_rows_pack_apply(const tg_tcsr* g, const int32_t* rows, int64_t D, const int64_t* off, int64_t n_pack,
                                       double* ts_out, int32_t* nbr_out, int32_t* eid_out, void* stream) {
  if (int rc = jp_args(g, rows, D, off)) return rc;
  if (n_pack < 0 || n_pack > g->num_entry) return TG_EINVAL;
  if (n_pack == 0) return TG_OK;
  if (D == 0 || !ts_out || !nbr_out || !eid_out) return TG_EINVAL;
  JpApplyArgs a{*g, rows, D, off, n_pack, ts_out, nbr_out, eid_out};
  hipLaunchKernelGGL(k_jp_apply, dim3((unsigned)cdiv(n_pack, JR_TILE)), dim3(JR_THREADS), 0, as_stream(stream), a);
  return check_launch("tg_tcsr_rows_pack_apply");
}

extern "C" size_t tg_tcsr_rows_splice_workspace_bytes(int64_t N_new) {
  if (N_new < 1 || N_new > 0x7fffffffLL) return 0;
  return js_layout(N_new).total;
}

extern "C" int tg_tcsr_rows_splice_plan(const tg_tcsr* g, int64_t N_new, const int32_t* rows, int64_t D, const int64_t* off,
                                        int64_t n_pack, int64_t* indptr_out, int64_t* out3, void* ws, size_t ws_bytes,
                                        void* stream) {
  if (int rc = js_args(g, N_new, rows, D, off, n_pack)) return rc;
  if (!indptr_out || !out3) return TG_EINVAL;
  const JsLayout l = js_layout(N_new);
  if (int rc = ws_check(ws, ws_bytes, l.total)) return rc;  // before the first launch
  char* b = static_cast<char*>(ws);
  JsArgs a{*g, N_new, rows, D, off, n_pack, indptr_out, reinterpret_cast<int64_t*>(b + l.enc),
           reinterpret_cast<uint32_t*>(b + l.rank), reinterpret_cast<uint32_t*>(b + l.blk),
           reinterpret_cast<unsigned long long*>(b + l.errs), reinterpret_cast<int64_t*>(b + l.total_word), out3};
  hipStream_t st = as_stream(stream);
  if (hipError_t e = hipMemsetAsync(a.errs, 0xff, 4 * sizeof(uint64_t), st)) {
    set_hip_error(e, "tg_tcsr_rows_splice_plan");
    return TG_EHIP;
  }
  const dim3 grid((unsigned)cdiv(N_new, JR_THREADS));
  hipLaunchKernelGGL(k_js_check, dim3((unsigned)cdiv(D + 1, JR_THREADS)), dim3(JR_THREADS), 0, st, a);
  hipLaunchKernelGGL(k_js_len, grid, dim3(JR_THREADS), 0, st, a);
  hipLaunchKernelGGL(k_js_ptr, grid, dim3(JR_THREADS), 0, st, a);
  hipLaunchKernelGGL(k_js_result, dim3(1), dim3(TG_WAVE), 0, st, a);
  return check_launch("tg_tcsr_rows_splice_plan");
}

extern "C" int tg_tcsr_rows_splice_apply(const tg_tcsr* g, int64_t N_new, const int64_t* indptr_out, int64_t num_entry_out,
                                         int64_t n_pack, const double* ts_pack, const int32_t* nbr_pack, const int32_t* eid_pack,
                                         double* ts_out, int32_t* nbr_out, int32_t* eid_out, const void* ws, size_t ws_bytes,
                                         void* stream) {
  if (int rc = tcsr_args(g)) return rc;
  if (N_new < g->num_node || N_new > 0x7fffffffLL || !indptr_out || n_pack < 0 || g->num_entry + n_pack > 0xffffffffLL)
    return TG_EINVAL;
  if (num_entry_out < 0 || num_entry_out > g->num_entry + n_pack) return TG_EINVAL;
  if (n_pack > 0 && (!ts_pack || !nbr_pack || !eid_pack)) return TG_EINVAL;
  if (num_entry_out > 0 && (!ts_out || !nbr_out || !eid_out)) return TG_EINVAL;
  const JsLayout l = js_layout(N_new);
  if (int rc = ws_check(ws, ws_bytes, l.total)) return rc;
  if (num_entry_out == 0) return TG_OK;
  JsApplyArgs a{*g, N_new, indptr_out, reinterpret_cast<const int64_t*>(static_cast<const char*>(ws) + l.enc), num_entry_out,
                n_pack, ts_pack, nbr_pack, eid_pack, ts_out, nbr_out, eid_out};
  hipLaunchKernelGGL(k_js_apply, dim3((unsigned)cdiv(num_entry_out, JR_TILE)), dim3(JR_THREADS), 0, as_stream(stream), a);
  return check_launch("tg_tcsr_rows_splice_apply");
}

extern "C" int tg_node_rows_scatter(const tg_node_rows* tabs, int32_t n_tab, const int32_t* ids, int64_t n_ids, void* stream) {
  if (int rc = jr_scatter_args(tabs, n_tab, ids, n_ids, true)) return rc;
  JrScatArgs a{};
  a.ids = ids;
  int64_t tiles = 0;
  for (int i = 0; i < n_tab; ++i) {
    if (tabs[i].n_rows_src == 0) continue;  // (a table without input rows takes no workgroup)
    const int k = a.n_tab++;
    a.tab[k] = tabs[i];
    const int64_t d4 = tabs[i].row_bytes / 16;
    a.tile_rows[k] = d4 ? (uint32_t)std::min<int64_t>(JR_TILE_ROWS, std::max<int64_t>(1, JR_TILE_F4 / d4)) : (uint32_t)JR_TILE;
    a.tile0[k] = (uint32_t)tiles;
    tiles += cdiv(tabs[i].n_rows_src, a.tile_rows[k]);
    if (tiles > 0x7fffffffLL) return TG_EINVAL;
  }
  a.tile0[a.n_tab] = (uint32_t)tiles;
  if (tiles == 0) return TG_OK;
  hipLaunchKernelGGL(k_jr_scatter, dim3((unsigned)tiles), dim3(JR_THREADS), 0, as_stream(stream), a);
  return check_launch("tg_node_rows_scatter");
}

extern "C" int tg_bitmap_scatter(const uint8_t* bytes, const int32_t* ids, int64_t n, uint64_t* bits, int64_t n_ids,
                                 void* stream) {
  if (int rc = jr_bits_args(bytes, ids, n, bits, n_ids)) return rc;
  if (n == 0) return TG_OK;
  hipLaunchKernelGGL(k_jr_bits, dim3(flat_grid(n, JR_THREADS)), dim3(JR_THREADS), 0, as_stream(stream), bytes, ids, n, bits,
                     n_ids);
  return check_launch("tg_bitmap_scatter");
}

// The host twins: plain C++ over host pointers (those of `g` and the descriptors included), one row after the other.
extern "C" int tg_tcsr_rows_pack_host(const tg_tcsr* g, const int32_t* rows, int64_t D, int64_t* off, double* ts_out,
                                      int32_t* nbr_out, int32_t* eid_out) {
  if (int rc = jp_args(g, rows, D, off)) return rc;
  int64_t q = 0;
  for (int64_t j = 0; j < D; ++j) {
    off[j] = q;
    const int64_t v = rows[j];
    if (v < 0 || v >= g->num_node) continue;
    const int64_t b = std::min(std::max(g->indptr[v], (int64_t)0), g->num_entry);
    const int64_t e = std::min(std::max(g->indptr[v + 1], (int64_t)0), g->num_entry);
    if (e <= b) continue;
    if (!ts_out || !nbr_out || !eid_out) return TG_EINVAL;
    std::copy(g->ts + b, g->ts + e, ts_out + q);
    std::copy(g->nbr + b, g->nbr + e, nbr_out + q);
    std::copy(g->eid + b, g->eid + e, eid_out + q);
    q += e - b;
  }
  off[D] = q;
  return TG_OK;
}

extern "C" int tg_tcsr_rows_splice_host(const tg_tcsr* g, int64_t N_new, const int32_t* rows, int64_t D, const int64_t* off,
                                        int64_t n_pack, const double* ts_pack, const int32_t* nbr_pack, const int32_t* eid_pack,
                                        int64_t* indptr_out, double* ts_out, int32_t* nbr_out, int32_t* eid_out, int64_t* out3) {
  if (int rc = js_args(g, N_new, rows, D, off, n_pack)) return rc;
  if (!indptr_out || !out3) return TG_EINVAL;
  if (n_pack > 0 && (!ts_pack || !nbr_pack || !eid_pack)) return TG_EINVAL;
  int64_t first[3] = {-1, -1, -1};
  for (int64_t j = D - 1; j >= 0; --j) {
    const int64_t r = rows[j];
    if (r < 0 || r >= N_new || (j > 0 && (int64_t)rows[j - 1] >= r)) first[0] = j;
  }
  if (off[D] != n_pack) first[1] = D;
  for (int64_t j = D - 1; j >= 0; --j)
    if (off[j + 1] < off[j]) first[1] = j + 1;
  if (off[0] != 0) first[1] = 0;
  for (int64_t v = g->num_node - 1; v >= 0; --v)
    if (g->indptr[v] < 0 || g->indptr[v + 1] < g->indptr[v] || g->indptr[v + 1] > g->num_entry) first[2] = v;
  out3[0] = 0;
  out3[1] = 0;
  out3[2] = -1;
  for (int c = 2; c >= 0; --c)
    if (first[c] >= 0) {
      out3[1] = c + 1;
      out3[2] = first[c];
    }
  if (out3[1]) {  // (the device's other outputs are not to be used either)
    for (int64_t v = 0; v <= N_new; ++v) indptr_out[v] = 0;
    return TG_OK;
  }
  int64_t q = 0, j = 0;
  for (int64_t v = 0; v < N_new; ++v) {
    indptr_out[v] = q;
    const bool hit = j < D && rows[j] == v;
    const int64_t b = hit ? off[j] : (v < g->num_node ? g->indptr[v] : 0);
    const int64_t e = hit ? off[j + 1] : (v < g->num_node ? g->indptr[v + 1] : 0);
    if (e > b) {
      if (!ts_out || !nbr_out || !eid_out) return TG_EINVAL;
      std::copy((hit ? ts_pack : g->ts) + b, (hit ? ts_pack : g->ts) + e, ts_out + q);
      std::copy((hit ? nbr_pack : g->nbr) + b, (hit ? nbr_pack : g->nbr) + e, nbr_out + q);
      std::copy((hit ? eid_pack : g->eid) + b, (hit ? eid_pack : g->eid) + e, eid_out + q);
      q += e - b;
    }
    j += hit;
  }
  indptr_out[N_new] = q;
  out3[0] = q;
  return TG_OK;
}

extern "C" int tg_node_rows_scatter_host(const tg_node_rows* tabs, int32_t n_tab, const int32_t* ids, int64_t n_ids) {
  if (int rc = jr_scatter_args(tabs, n_tab, ids, n_ids, false)) return rc;
  for (int i = 0; i < n_tab; ++i) {
    const tg_node_rows& d = tabs[i];
    for (int64_t j = 0; j < d.n_rows_src; ++j) {
      const int32_t o = ids[j];
      if ((uint32_t)o < (uint64_t)d.n_rows_out)
        std::memcpy(static_cast<char*>(d.dst) + (int64_t)o * d.row_bytes, static_cast<const char*>(d.src) + j * d.row_bytes,
                    (size_t)d.row_bytes);
    }
  }
  return TG_OK;
}

extern "C" int tg_bitmap_scatter_host(const uint8_t* bytes, const int32_t* ids, int64_t n, uint64_t* bits, int64_t n_ids) {
  if (int rc = jr_bits_args(bytes, ids, n, bits, n_ids)) return rc;
  for (int64_t j = 0; j < n; ++j) {
    const int64_t id = ids[j];
    if (id < 0 || id >= n_ids) continue;
    const uint64_t bit = 1ull << (id & 63);
    if (bytes[j]) bits[id >> 6] |= bit;
    else bits[id >> 6] &= ~bit;
  }
  return TG_OK;
}
