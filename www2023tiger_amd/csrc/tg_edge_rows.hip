// Releasing edge-feature rows of forgotten events (online serving; reference tiger/data/graph.py:11-42 and
// tiger/model/feature_getter.py: the reference builds graph and tables once over the whole stream and never drops a row -
// it has no counterpart of this).
//
// The T-CSR names edge-table rows (eid & 0x7FFFFFFF).  After a trim most rows are named by no entry any more.  A row r of
// the table T [n_rows, d_e] is LIVE iff r == 0 (the padding row), some entry names it, r >= keep_from (rows of events the
// caller has not observed yet) or r is pinned.  remap[r] = number of live rows below r (-1: dead) is monotone, so the
// packed table keeps the order of the rows and [keep_from, n_rows) moves as one block.
//   mark  (k_er_mark, one workgroup per 2048 entries / pins): one BYTE per row, plain stores of the value 1 - whichever
//          lane wins, the byte is 1 (as k_involved_mark does; packed bits would need atomics).  An id >= n_rows stores 1
//          into a flag word instead.  Marks and flag are zeroed by a memset node in front.
//   scan A (k_er_scan_rows, one workgroup per 2048 rows): a thread loads its 8 marks as one 8-byte word, adds row 0 and
//          the tail, counts; exclusive scan inside the workgroup, one total per workgroup.
//   scan B (k_er_scan_emit, the same grid): workgroup b sums the b totals in front of it (block_sum_front: no third
//          scan launch) and writes remap, the inverse list old_of[new] and n_live (-1 if the flag is set; then
//          remap is not written at all).
//   apply  (k_er_copy_rows, one workgroup per tile of whole OUTPUT rows, about 4096 float4): the tile's old_of values
//          are staged once in LDS; the lanes then sweep the tile's float4s in output order - stores are contiguous over
//          T_out, loads are contiguous inside every source row (and across rows wherever neighbours survived) - four
//          independent 16-byte loads in flight per lane before the first store.  Row / column of a float4 advance
//          incrementally (d_e / 4 is a runtime value, 43 at d_e = 172: one division per thread, none in the loop).
//          (k_er_remap_eids, one workgroup per 2048 entries): eid_out[p] = remap[eid & 0x7FFFFFFF] | (eid & 0x80000000).
// No atomics, no capped grid, integer work and bit copies: device, host twin and numpy agree bit for bit whatever the
// launch geometry.
#include <algorithm>
#include <cstring>
#include <vector>

#include "tg_step.h"
#include "tg_tcsr.h"

namespace tg {

constexpr int ER_THREADS = TG_SCAN_BLOCK;       // block_excl_scan: 256
constexpr int ER_MARKS = 8;                     // marks per thread of the scan: one 8-byte load
constexpr int ER_CHUNK = ER_THREADS * ER_MARKS;  // rows per scan workgroup
constexpr int ER_ITEMS = 8;
constexpr int ER_ENTRIES = ER_THREADS * ER_ITEMS;  // entries per workgroup of mark / eid remap
constexpr int ER_TILE_F4 = 4096;                // float4s per copy tile (64 KiB read, 64 KiB written)
constexpr int ER_TILE_ROWS = 2048;              // most rows of one copy tile (their old_of values: 8 KiB of LDS)
constexpr int ER_BATCH = 4;                     // independent 16-byte loads in flight per lane

__global__ void __launch_bounds__(ER_THREADS) k_er_mark(const int32_t* __restrict__ eid, int64_t num_entry,
                                                        const int64_t* __restrict__ pin, int64_t n_pin, int64_t n_rows,
                                                        uint8_t* __restrict__ marks, uint32_t* __restrict__ flag) {
  const int64_t p0 = (int64_t)blockIdx.x * ER_ENTRIES + threadIdx.x;
#pragma unroll
  for (int i = 0; i < ER_ITEMS; ++i) {
    const int64_t p = p0 + (int64_t)i * ER_THREADS;
    if (p < num_entry) {
      const int64_t r = (int64_t)((uint32_t)eid[p] & 0x7fffffffu);
      if (r < n_rows) marks[r] = 1;
      else *flag = 1u;
    }
    if (p < n_pin) {
      const int64_t r = pin[p];
      if (r >= 0 && r < n_rows) marks[r] = 1;
      else *flag = 1u;
    }
  }
}

// live rows among [r0, r0 + 8) as 8 bits; r0 is a multiple of 8 and the marks are padded with zeros to a multiple of 16
__device__ __forceinline__ uint32_t live_bits(const uint8_t* __restrict__ marks, int64_t r0, int64_t n_rows, int64_t keep_from) {
  if (r0 >= n_rows) return 0u;
  uint32_t bits = (uint32_t)pack8(*reinterpret_cast<const uint64_t*>(marks + r0));
  const int lo = (int)min(max(keep_from - r0, (int64_t)0), (int64_t)8);  // rows [r0 + lo, r0 + 8) belong to the tail
  bits |= 0xffu & ~((1u << lo) - 1u);
  if (r0 == 0) bits |= 1u;  // the padding row
  const int nv = (int)min(n_rows - r0, (int64_t)8);
  return bits & ((1u << nv) - 1u);
}

__global__ void __launch_bounds__(ER_THREADS) k_er_scan_rows(const uint8_t* __restrict__ marks, int64_t n_rows,
                                                             int64_t keep_from, uint32_t* __restrict__ rank,
                                                             uint32_t* __restrict__ blk) {
  __shared__ uint32_t s_w[ER_THREADS / TG_WAVE];
  const int64_t slot = (int64_t)blockIdx.x * ER_THREADS + threadIdx.x;
  const int64_t r0 = slot * ER_MARKS;
  const uint32_t n = (uint32_t)__popc(live_bits(marks, r0, n_rows, keep_from));
  uint32_t total;
  const uint32_t r = block_excl_scan(n, s_w, &total);
  if (r0 < n_rows) rank[slot] = r;
  if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(ER_THREADS) k_er_scan_emit(const uint8_t* __restrict__ marks, int64_t n_rows,
                                                             int64_t keep_from, const uint32_t* __restrict__ rank,
                                                             const uint32_t* __restrict__ blk,
                                                             const uint32_t* __restrict__ flag, int32_t* __restrict__ remap,
                                                             int32_t* __restrict__ old_of, int64_t* __restrict__ n_live) {
  __shared__ uint32_t s_w[ER_THREADS / TG_WAVE];
  if (*flag) {  // (uniform over the grid) an id that is no row: nothing but the error is written
    if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1) *n_live = -1;
    return;
  }
  const uint32_t base = block_sum_front(blk, blockIdx.x, s_w);  // live rows in front of this chunk
  const int64_t slot = (int64_t)blockIdx.x * ER_THREADS + threadIdx.x;
  const int64_t r0 = slot * ER_MARKS;
  if (r0 < n_rows) {
    const uint32_t bits = live_bits(marks, r0, n_rows, keep_from);
    uint32_t o = base + rank[slot];
    int32_t out[ER_MARKS];
#pragma unroll
    for (int j = 0; j < ER_MARKS; ++j) {
      const bool live = (bits >> j) & 1u;
      out[j] = live ? (int32_t)o : -1;
      if (live) old_of[o++] = (int32_t)(r0 + j);
    }
    if (r0 + ER_MARKS <= n_rows) {  // remap is 16-byte aligned and r0 a multiple of 8
      int4* dst = reinterpret_cast<int4*>(remap + r0);
      dst[0] = make_int4(out[0], out[1], out[2], out[3]);
      dst[1] = make_int4(out[4], out[5], out[6], out[7]);
    } else {
#pragma unroll
      for (int j = 0; j < ER_MARKS; ++j)
        if (r0 + j < n_rows) remap[r0 + j] = out[j];
    }
  }
  if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1) *n_live = (int64_t)base + (int64_t)blk[blockIdx.x];
}

struct ErCopyArgs {
  const float4* src;
  float4* dst;
  const int32_t* old_of;
  int64_t n_rows, n_live;
  uint32_t d4, tile_rows;
  uint32_t q_step, r_step;  // ER_THREADS / d4, ER_THREADS % d4
};
__global__ void __launch_bounds__(ER_THREADS) k_er_copy_rows(ErCopyArgs a) {
  __shared__ int32_t s_old[ER_TILE_ROWS];
  const uint32_t t = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * a.tile_rows;
  const uint32_t rows = (uint32_t)min((int64_t)a.tile_rows, a.n_live - row0);
  for (uint32_t i = t; i < rows; i += ER_THREADS) {
    const int32_t o = a.old_of[row0 + i];
    s_old[i] = (uint32_t)o < (uint64_t)a.n_rows ? o : -1;  // (a workspace that is no plan of this table: nothing is read out of bounds)
  }
  __syncthreads();
  const uint64_t nf = (uint64_t)rows * a.d4;  // float4s of the tile, swept in output order
  float4* __restrict__ dst = a.dst + row0 * (int64_t)a.d4;
  uint32_t row = t / a.d4, col = t % a.d4;  // of float4 f = t; both advance by the step of ER_THREADS
  for (uint64_t f = t; f < nf; f += (uint64_t)ER_BATCH * ER_THREADS) {
    // (the loads stay unconditional: a float4 past the tile's end reads row 0, which every table has, and is not stored)
    auto load = [&](int i, bool& ok) {
      const int32_t o = s_old[min(row, rows - 1u)];
      ok = f + (uint64_t)i * ER_THREADS < nf && o >= 0;
      const float4 v = a.src[(int64_t)(ok ? o : 0) * a.d4 + col];
      row += a.q_step;
      col += a.r_step;
      if (col >= a.d4) {
        col -= a.d4;
        ++row;
      }
      return v;
    };
    static_assert(ER_BATCH == 4, "four named registers below");
    bool k0, k1, k2, k3;
    const float4 v0 = load(0, k0), v1 = load(1, k1), v2 = load(2, k2), v3 = load(3, k3);
    if (k0) dst[f] = v0;
    if (k1) dst[f + ER_THREADS] = v1;
    if (k2) dst[f + 2 * ER_THREADS] = v2;
    if (k3) dst[f + 3 * ER_THREADS] = v3;
  }
}

__global__ void __launch_bounds__(ER_THREADS) k_er_remap_eids(const int32_t* __restrict__ eid, int64_t num_entry,
                                                              const int32_t* __restrict__ remap, int64_t n_rows,
                                                              int32_t* __restrict__ eid_out) {
  const int64_t p0 = (int64_t)blockIdx.x * ER_ENTRIES + threadIdx.x;
  uint32_t e[ER_ITEMS];
#pragma unroll
  for (int i = 0; i < ER_ITEMS; ++i) {
    const int64_t p = p0 + (int64_t)i * ER_THREADS;
    e[i] = p < num_entry ? (uint32_t)eid[p] : 0xffffffffu;
  }
#pragma unroll
  for (int i = 0; i < ER_ITEMS; ++i) {
    const int64_t p = p0 + (int64_t)i * ER_THREADS;
    const int64_t r = (int64_t)(e[i] & 0x7fffffffu);
    if (p < num_entry && r < n_rows) eid_out[p] = (int32_t)((uint32_t)remap[r] | (e[i] & 0x80000000u));
  }
}

struct ErLayout {
  size_t marks, flag, rank, blk, old_of, total;
};
static ErLayout er_layout(int64_t n_rows) {
  ErLayout l{};
  l.marks = 0;
  l.flag = l.marks + align16((size_t)n_rows);  // (right behind the marks: one memset zeroes both)
  l.rank = l.flag + 16;
  l.blk = l.rank + align16((size_t)cdiv(n_rows, ER_MARKS) * sizeof(uint32_t));
  l.old_of = l.blk + align16((size_t)cdiv(n_rows, ER_CHUNK) * sizeof(uint32_t));
  l.total = l.old_of + align16((size_t)n_rows * sizeof(int32_t));
  return l;
}

static int er_args(const tg_tcsr* g, int64_t n_rows) {
  if (!g || g->num_entry < 0 || g->num_entry > 0xffffffffLL || n_rows < 1 || n_rows > 0x7fffffffLL) return TG_EINVAL;
  if (g->num_entry > 0 && !g->eid) return TG_EINVAL;
  return TG_OK;
}

}  // namespace tg

using namespace tg;

extern "C" size_t tg_edge_rows_workspace_bytes(int64_t n_rows, int64_t num_entry) {
  if (n_rows < 1 || n_rows > 0x7fffffffLL || num_entry < 0 || num_entry > 0xffffffffLL) return 0;
  return er_layout(n_rows).total;
}

extern "C" int tg_edge_rows_plan(const tg_tcsr* g, int64_t n_rows, int64_t keep_from, const int64_t* pin, int64_t n_pin,
                                 int32_t* remap, int64_t* n_live_dev, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = er_args(g, n_rows)) return rc;
  if (keep_from < 0 || keep_from > n_rows || n_pin < 0 || n_pin > 0xffffffffLL || (n_pin > 0 && !pin)) return TG_EINVAL;
  if (!remap || !n_live_dev || (reinterpret_cast<uintptr_t>(remap) & 15)) return TG_EINVAL;
  const ErLayout l = er_layout(n_rows);
  if (int rc = ws_check(ws, ws_bytes, l.total)) return rc;  // before the first launch
  hipStream_t st = as_stream(stream);
  char* base = static_cast<char*>(ws);
  uint8_t* marks = reinterpret_cast<uint8_t*>(base + l.marks);
  uint32_t* flag = reinterpret_cast<uint32_t*>(base + l.flag);
  uint32_t* rank = reinterpret_cast<uint32_t*>(base + l.rank);
  uint32_t* blk = reinterpret_cast<uint32_t*>(base + l.blk);
  int32_t* old_of = reinterpret_cast<int32_t*>(base + l.old_of);
  const hipError_t e = hipMemsetAsync(marks, 0, l.rank - l.marks, st);  // marks (with their padding) and the flag
  if (e != hipSuccess) {
    set_hip_error(e, "tg_edge_rows_plan");
    return TG_EHIP;
  }
  const int64_t work = std::max(g->num_entry, n_pin);
  if (work > 0)
    hipLaunchKernelGGL(k_er_mark, dim3((unsigned)cdiv(work, ER_ENTRIES)), dim3(ER_THREADS), 0, st, g->eid, g->num_entry, pin,
                       n_pin, n_rows, marks, flag);
  const dim3 grid((unsigned)cdiv(n_rows, ER_CHUNK));
  hipLaunchKernelGGL(k_er_scan_rows, grid, dim3(ER_THREADS), 0, st, marks, n_rows, keep_from, rank, blk);
  hipLaunchKernelGGL(k_er_scan_emit, grid, dim3(ER_THREADS), 0, st, marks, n_rows, keep_from, rank, blk, flag, remap, old_of,
                     n_live_dev);
  return check_launch("tg_edge_rows_plan");
}

extern "C" int tg_edge_rows_apply(const tg_tcsr* g, const float* table, int64_t n_rows, int32_t d_e, const int32_t* remap,
                                  int64_t n_live, float* table_out, int32_t* eid_out, const void* ws, size_t ws_bytes,
                                  void* stream) {
  if (int rc = er_args(g, n_rows)) return rc;
  if (!remap || n_live < 1 || n_live > n_rows) return TG_EINVAL;
  if (g->num_entry > 0 && !eid_out) return TG_EINVAL;
  if (table && (d_e < 4 || d_e % 4 != 0 || !table_out)) return TG_EINVAL;
  if (table && ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(table_out)) & 15)) return TG_EINVAL;
  const ErLayout l = er_layout(n_rows);
  if (int rc = ws_check(ws, ws_bytes, l.total)) return rc;
  hipStream_t st = as_stream(stream);
  if (table) {
    ErCopyArgs a{};
    a.src = reinterpret_cast<const float4*>(table);
    a.dst = reinterpret_cast<float4*>(table_out);
    a.old_of = reinterpret_cast<const int32_t*>(static_cast<const char*>(ws) + l.old_of);
    a.n_rows = n_rows;
    a.n_live = n_live;
    a.d4 = (uint32_t)(d_e / 4);
    a.tile_rows = std::min<uint32_t>(ER_TILE_ROWS, std::max<uint32_t>(1u, ER_TILE_F4 / a.d4));
    a.q_step = ER_THREADS / a.d4;
    a.r_step = ER_THREADS % a.d4;
    hipLaunchKernelGGL(k_er_copy_rows, dim3((unsigned)cdiv(n_live, a.tile_rows)), dim3(ER_THREADS), 0, st, a);
  }
  if (g->num_entry > 0)
    hipLaunchKernelGGL(k_er_remap_eids, dim3((unsigned)cdiv(g->num_entry, ER_ENTRIES)), dim3(ER_THREADS), 0, st, g->eid,
                       g->num_entry, remap, n_rows, eid_out);
  return check_launch("tg_edge_rows_apply");
}

// The host twin: plain C++ over host pointers.  Everything is checked before anything is written.
extern "C" int tg_edge_rows_host(const tg_tcsr* g, const float* table, int64_t n_rows, int32_t d_e, int64_t keep_from,
                                 const int64_t* pin, int64_t n_pin, int32_t* remap, float* table_out, int32_t* eid_out,
                                 int64_t* n_live_out) {
  if (int rc = er_args(g, n_rows)) return rc;
  if (keep_from < 0 || keep_from > n_rows || n_pin < 0 || (n_pin > 0 && !pin) || !remap || !n_live_out) return TG_EINVAL;
  if (g->num_entry > 0 && !eid_out) return TG_EINVAL;
  if (table && (d_e < 4 || d_e % 4 != 0 || !table_out)) return TG_EINVAL;
  std::vector<uint8_t> live((size_t)n_rows, 0);
  live[0] = 1;
  for (int64_t p = 0; p < g->num_entry; ++p) {
    const int64_t r = (int64_t)((uint32_t)g->eid[p] & 0x7fffffffu);
    if (r >= n_rows) return TG_EINVAL;
    live[(size_t)r] = 1;
  }
  for (int64_t i = 0; i < n_pin; ++i) {
    if (pin[i] < 0 || pin[i] >= n_rows) return TG_EINVAL;
    live[(size_t)pin[i]] = 1;
  }
  int64_t n = 0;
  for (int64_t r = 0; r < n_rows; ++r) {
    if (live[(size_t)r] || r >= keep_from) {
      if (table) std::memcpy(table_out + n * d_e, table + r * d_e, (size_t)d_e * sizeof(float));
      remap[r] = (int32_t)n++;
    } else {
      remap[r] = -1;
    }
  }
  for (int64_t p = 0; p < g->num_entry; ++p) {
    const uint32_t e = (uint32_t)g->eid[p];
    eid_out[p] = (int32_t)((uint32_t)remap[e & 0x7fffffffu] | (e & 0x80000000u));
  }
  *n_live_out = n;
  return TG_OK;
}
