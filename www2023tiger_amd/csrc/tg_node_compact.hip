// Compacting the node id space (online serving after erasures; DESIGN 7.20.  The reference numbers its nodes offline and
// never releases an id - it has no counterpart of this).
//
// drop_bits: 64-bit words over the ids [0, N), a set bit = the id leaves (the layout of the id map's free_bits).  The remap
// is MONOTONE: remap[i] = the number of kept ids below i (-1: dropped), old_of its inverse list, ascending.  A dropped id
// must own no entry and be nobody's neighbour, so no T-CSR entry moves: ts / eid stay the parent's arrays, indptr_out is a
// gather of the kept rows' bounds and nbr_out an element-wise remap.
//   count  (k_nc_count, one workgroup per tile of 2048 words = 131 072 ids): a thread loads its 8 consecutive words (bits at
//           or beyond N masked off), counts the KEPT ids; one total per tile.  The workgroup that holds word 0 reports ID0,
//           the one that holds the last word SPARE.
//   emit   (k_nc_emit, the same grid): the tile sums the totals in front of it (block_sum_front: no third scan launch),
//           scans its threads' counts, then every wavefront writes together: the eight words of one lane are broadcast and
//           lane l handles bit l of each - remap, old_of and indptr_out leave as runs of consecutive ids.  A dropped id
//           below g->num_node with a non-empty row reports ROW.  The lanes that own ids num_node - 1 and N - 1 write the
//           two counts.
//   nbr    (k_nc_nbr, one workgroup per 2048 entries): nbr_out[p] = remap[nbr[p]]; a value outside [0, num_node) or with
//           remap -1 reports NBR and indexes nothing.
//   result (k_nc_result, one thread): {n_new, n_new_graph, error class, smallest offender} - the one read-back.
// An error is folded with a 64-bit atomicMin per class over the offending index (only offenders issue one), so the
// smallest offender is named whatever the launch geometry; the classes are reported in the order ID0, SPARE, ROW, NBR.
// No kernel waits for another workgroup: every value another workgroup writes is read by a LATER launch.
//
// rows   (k_nc_rows, ONE launch for up to 8 tables): dst[j] = src[old_of[j]].  A workgroup belongs to one table (the tile
//           starts of the tables are kernel arguments).  Rows of a multiple of 16 bytes: a tile of whole OUTPUT rows, about
//           4096 16-byte pieces; the tile's old_of values are staged in LDS and the lanes sweep the pieces in output order,
//           four independent 16-byte loads in flight per lane, contiguous stores (as k_er_copy_rows of tg_edge_rows.hip).
//           Rows of 8, 4 or 1 bytes: 2048 rows per tile, one element per lane and step.
// bitmap (k_nc_bitmap): one lane per output bit, the wavefront's ballot is the output word.
// Integer work and bit copies only: device, host twin and numpy agree bit for bit.
#include <algorithm>
#include <cstring>
#include <vector>

#include "tg_step.h"
#include "tg_tcsr.h"

namespace tg {

constexpr int NC_THREADS = TG_SCAN_BLOCK;  // block_excl_scan: 256
constexpr int NC_WAVES = NC_THREADS / TG_WAVE;
constexpr int NC_ITEMS = 8;
constexpr int NC_TILE = NC_THREADS * NC_ITEMS;  // bitmap words per workgroup: 131 072 ids; entries per workgroup of the nbr pass
constexpr int NC_TILE_F4 = 4096;                // 16-byte pieces per wide copy tile (64 KiB read, 64 KiB written)
constexpr int NC_TILE_ROWS = 2048;              // most rows of one copy tile (their old_of values: 8 KiB of LDS)
constexpr int NC_BATCH = 4;                     // independent 16-byte loads in flight per lane
constexpr unsigned long long NC_NONE = ~0ull;   // an error word nobody lowered

struct NcPlanArgs {
  const uint64_t* bits;
  int64_t N, words;  // words = ceil(N / 64)
  int64_t num_node, num_entry;
  const int64_t* indptr;
  const int32_t* nbr;
  int32_t *remap, *old_of, *nbr_out;
  int64_t* indptr_out;
  int64_t* out4;
  uint32_t* tcnt;             // [n_tile] kept ids per tile
  unsigned long long* errs;   // [4] the smallest offender per class, NC_NONE without one
  int64_t* counts;            // [2] {n_new, n_new_graph}
};

// the word `w` of the bitmap with the bits at or beyond N cleared; 0 for a word past the end
__device__ __forceinline__ uint64_t nc_word(const NcPlanArgs& a, int64_t w) {
  if (w >= a.words) return 0ull;
  const uint64_t v = a.bits[w];
  const int64_t left = a.N - w * 64;
  return left >= 64 ? v : v & ((1ull << left) - 1ull);
}
// ids of word `w` that exist: 64, fewer in the last word, 0 past the end
__device__ __forceinline__ int nc_valid(const NcPlanArgs& a, int64_t w) {
  return (int)min(max(a.N - w * 64, (int64_t)0), (int64_t)64);
}
// thread t of tile `tile` owns the 8 consecutive words from tile * 2048 + 8 t: thread order is id order
__device__ __forceinline__ uint32_t nc_load(const NcPlanArgs& a, int64_t tile, uint64_t (&w)[NC_ITEMS]) {
  const int64_t w0 = tile * NC_TILE + (int64_t)threadIdx.x * NC_ITEMS;
  uint32_t kept = 0;
#pragma unroll
  for (int j = 0; j < NC_ITEMS; ++j) {
    w[j] = nc_word(a, w0 + j);
    kept += (uint32_t)(nc_valid(a, w0 + j) - __popcll(w[j]));
  }
  return kept;
}

__global__ void __launch_bounds__(NC_THREADS) k_nc_count(NcPlanArgs a) {
  __shared__ uint32_t s_w[NC_WAVES];
  const int64_t tile = (int64_t)blockIdx.x;
  uint64_t w[NC_ITEMS];
  uint32_t total;
  block_excl_scan(nc_load(a, tile, w), s_w, &total);
  if (threadIdx.x == 0) {
    a.tcnt[tile] = total;
    if (tile == 0 && (w[0] & 1ull)) atomicMin(a.errs + 0, 0ull);  // ID0
  }
  const int64_t last = a.words - 1;  // SPARE: set bits at or beyond N in the last word
  if (tile == last / NC_TILE && threadIdx.x == (uint32_t)((last % NC_TILE) / NC_ITEMS)) {
    const uint64_t spare = a.bits[last] & ~nc_word(a, last);
    if (spare) atomicMin(a.errs + 1, (unsigned long long)(last * 64 + (__ffsll((unsigned long long)spare) - 1)));
  }
}

__global__ void __launch_bounds__(NC_THREADS) k_nc_emit(NcPlanArgs a) {
  __shared__ uint32_t s_w[NC_WAVES];
  const int64_t tile = (int64_t)blockIdx.x;
  const uint32_t front = block_sum_front(a.tcnt, (uint32_t)tile, s_w);  // (tile < 2^14)
  uint64_t w[NC_ITEMS];
  uint32_t total;
  const uint32_t mine = nc_load(a, tile, w);
  const uint32_t r = front + block_excl_scan(mine, s_w, &total);  // kept ids in front of this thread's first id (< 2^31)
  // The wavefront writes together: the eight words of lane `src` are broadcast and lane l handles bit l of each, 64
  // consecutive ids per store instruction.  (The loop bounds are wave-uniform.)
  const int lane = lane_id();
  const uint64_t below = (1ull << lane) - 1ull;
  const int64_t w_wave = tile * NC_TILE + (int64_t)(threadIdx.x - lane) * NC_ITEMS;  // the first word of lane 0
  const int n_src = (int)min((max(a.words - w_wave, (int64_t)0) + NC_ITEMS - 1) / NC_ITEMS, (int64_t)TG_WAVE);
  unsigned long long bad_row = NC_NONE;
  for (int src = 0; src < n_src; ++src) {
    int64_t rr = (int64_t)(uint32_t)__shfl((int)r, src);
    const int64_t ws = w_wave + (int64_t)src * NC_ITEMS;
#pragma unroll
    for (int j = 0; j < NC_ITEMS; ++j) {
      const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)w[j], src), hi = (uint32_t)__shfl((int)(uint32_t)(w[j] >> 32), src);
      const uint64_t word = ((uint64_t)hi << 32) | lo;
      const int valid = nc_valid(a, ws + j);
      const uint64_t keep = ~word & (valid >= 64 ? ~0ull : (1ull << valid) - 1ull);
      const int64_t id = (ws + j) * 64 + lane;
      if (lane < valid) {
        const bool kept = (keep >> lane) & 1ull;
        const int64_t rank = rr + __popcll(keep & below);
        a.remap[id] = kept ? (int32_t)rank : -1;
        if (kept) a.old_of[rank] = (int32_t)id;
        if (id < a.num_node) {
          const int64_t p = a.indptr[id];
          if (kept) a.indptr_out[rank] = p;
          else if (a.indptr[id + 1] != p) bad_row = min(bad_row, (unsigned long long)id);
          if (id == a.num_node - 1) {
            a.counts[1] = rank + kept;
            a.indptr_out[rank + kept] = a.indptr[a.num_node];
          }
        }
        if (id == a.N - 1) a.counts[0] = rank + kept;
      }
      rr += __popcll(keep);
    }
  }
  if (bad_row != NC_NONE) atomicMin(a.errs + 2, bad_row);
}

__global__ void __launch_bounds__(NC_THREADS) k_nc_nbr(NcPlanArgs a) {
  const int64_t p0 = (int64_t)blockIdx.x * NC_TILE + threadIdx.x;
  int32_t v[NC_ITEMS];
#pragma unroll
  for (int i = 0; i < NC_ITEMS; ++i) {
    const int64_t p = p0 + (int64_t)i * NC_THREADS;
    v[i] = p < a.num_entry ? a.nbr[p] : 0;
  }
  unsigned long long bad = NC_NONE;
#pragma unroll
  for (int i = 0; i < NC_ITEMS; ++i) {
    const int64_t p = p0 + (int64_t)i * NC_THREADS;
    if (p >= a.num_entry) continue;
    const int32_t r = (uint32_t)v[i] < (uint64_t)a.num_node ? a.remap[v[i]] : -1;  // (range-checked before it indexes)
    a.nbr_out[p] = r;
    if (r < 0) bad = min(bad, (unsigned long long)p);
  }
  if (bad != NC_NONE) atomicMin(a.errs + 3, bad);
}

__global__ void k_nc_result(NcPlanArgs a) {
  if (threadIdx.x || blockIdx.x) return;
  int64_t cls = 0, first = -1;
  for (int c = 3; c >= 0; --c)
    if (a.errs[c] != NC_NONE) {
      cls = c + 1;
      first = (int64_t)a.errs[c];
    }
  a.out4[0] = a.counts[0];
  a.out4[1] = a.counts[1];
  a.out4[2] = cls;
  a.out4[3] = first;
}

struct NcLayout {
  int64_t n_tile;
  size_t tcnt, errs, counts, total;
};
static NcLayout nc_layout(int64_t N) {
  NcLayout l{};
  l.n_tile = cdiv(cdiv(N, 64), NC_TILE);
  l.tcnt = 0;
  l.errs = l.tcnt + align16((size_t)l.n_tile * sizeof(uint32_t));
  l.counts = l.errs + 4 * sizeof(uint64_t);
  l.total = l.counts + 2 * sizeof(int64_t);
  return l;
}

static int nc_plan_args(const tg_tcsr* g, const uint64_t* drop_bits, int64_t bit_words, int64_t N, const int32_t* remap,
                        const int32_t* old_of, const int64_t* indptr_out, const int32_t* nbr_out, const int64_t* out4) {
  if (int rc = tcsr_args(g)) return rc;
  if (N < g->num_node || N > 0x7fffffffLL || !drop_bits || bit_words < cdiv(N, 64)) return TG_EINVAL;
  if (!remap || !old_of || !indptr_out || !out4 || (g->num_entry > 0 && !nbr_out)) return TG_EINVAL;
  return TG_OK;
}

// ---- rows ---------------------------------------------------------------------------------------------------------------
struct NcRowsArgs {
  tg_node_rows tab[TG_NODE_ROWS_MAX];
  uint32_t tile0[TG_NODE_ROWS_MAX + 1];  // the first workgroup of every table; [n_tab] = the grid
  uint32_t tile_rows[TG_NODE_ROWS_MAX];
  const int32_t* old_of;
  int32_t n_tab;
};

template <typename T>
__device__ __forceinline__ void nc_rows_narrow(const tg_node_rows& d, const int32_t* __restrict__ old_of, int64_t row0) {
  const T* __restrict__ src = static_cast<const T*>(d.src);
  T* __restrict__ dst = static_cast<T*>(d.dst);
  const int64_t end = min(row0 + NC_TILE, d.n_rows_out);
  int32_t o[NC_ITEMS];
#pragma unroll
  for (int i = 0; i < NC_ITEMS; ++i) {
    const int64_t j = row0 + (int64_t)i * NC_THREADS + threadIdx.x;
    o[i] = j < end ? old_of[j] : -1;
  }
#pragma unroll
  for (int i = 0; i < NC_ITEMS; ++i) {
    const int64_t j = row0 + (int64_t)i * NC_THREADS + threadIdx.x;
    if (j < end && (uint32_t)o[i] < (uint64_t)d.n_rows_src) dst[j] = src[o[i]];  // (an old_of that is no plan of this table reads nothing)
  }
}

__global__ void __launch_bounds__(NC_THREADS) k_nc_rows(NcRowsArgs a) {
  __shared__ int32_t s_old[NC_TILE_ROWS];
  int tb = 0;  // (block-uniform) the table of this workgroup
#pragma unroll
  for (int i = 1; i < TG_NODE_ROWS_MAX; ++i)
    if (i < a.n_tab && blockIdx.x >= a.tile0[i]) tb = i;
  const tg_node_rows d = a.tab[tb];
  const int64_t row0 = (int64_t)(blockIdx.x - a.tile0[tb]) * a.tile_rows[tb];
  if (d.row_bytes == 8) return nc_rows_narrow<uint64_t>(d, a.old_of, row0);
  if (d.row_bytes == 4) return nc_rows_narrow<uint32_t>(d, a.old_of, row0);
  if (d.row_bytes == 1) return nc_rows_narrow<uint8_t>(d, a.old_of, row0);
  const uint32_t t = threadIdx.x;
  const uint32_t d4 = (uint32_t)(d.row_bytes / 16);
  const uint32_t rows = (uint32_t)min((int64_t)a.tile_rows[tb], d.n_rows_out - row0);
  for (uint32_t i = t; i < rows; i += NC_THREADS) {
    const int32_t o = a.old_of[row0 + i];
    s_old[i] = (uint32_t)o < (uint64_t)d.n_rows_src ? o : -1;
  }
  __syncthreads();
  const uint64_t nf = (uint64_t)rows * d4;  // 16-byte pieces of the tile, swept in output order
  const float4* __restrict__ src = static_cast<const float4*>(d.src);
  float4* __restrict__ dst = static_cast<float4*>(d.dst) + row0 * (int64_t)d4;
  const uint32_t q_step = NC_THREADS / d4, r_step = NC_THREADS % d4;
  uint32_t row = t / d4, col = t % d4;  // of piece f = t; both advance by the step of NC_THREADS
  for (uint64_t f = t; f < nf; f += (uint64_t)NC_BATCH * NC_THREADS) {
    // (the loads stay unconditional: a piece past the tile's end reads row 0 of the source and is not stored)
    auto load = [&](int i, bool& ok) {
      const int32_t o = s_old[min(row, rows - 1u)];
      ok = f + (uint64_t)i * NC_THREADS < nf && o >= 0;
      const float4 v = src[(int64_t)(ok ? o : 0) * d4 + col];
      row += q_step;
      col += r_step;
      if (col >= d4) {
        col -= d4;
        ++row;
      }
      return v;
    };
    static_assert(NC_BATCH == 4, "four named registers below");
    bool k0, k1, k2, k3;
    const float4 v0 = load(0, k0), v1 = load(1, k1), v2 = load(2, k2), v3 = load(3, k3);
    if (k0) dst[f] = v0;
    if (k1) dst[f + NC_THREADS] = v1;
    if (k2) dst[f + 2 * NC_THREADS] = v2;
    if (k3) dst[f + 3 * NC_THREADS] = v3;
  }
}

// everything the device entry and the host twin refuse; wide rows also want 16-byte aligned tables when `aligned`
static int nc_rows_args(const tg_node_rows* tabs, int32_t n_tab, const int32_t* old_of, int64_t n_new, bool aligned) {
  if (n_tab < 0 || n_tab > TG_NODE_ROWS_MAX || (n_tab > 0 && !tabs) || n_new < 0 || n_new > 0x7fffffffLL) return TG_EINVAL;
  for (int i = 0; i < n_tab; ++i) {
    const tg_node_rows& d = tabs[i];
    const bool wide = d.row_bytes >= 16 && d.row_bytes % 16 == 0;
    if (!wide && d.row_bytes != 8 && d.row_bytes != 4 && d.row_bytes != 1) return TG_EINVAL;
    if (d.row_bytes > (1 << 20) || d.n_rows_out < 0 || d.n_rows_out > n_new || d.n_rows_src < 1 || d.n_rows_src > 0x7fffffffLL)
      return TG_EINVAL;
    if (d.n_rows_out == 0) continue;
    if (!d.src || !d.dst || !old_of) return TG_EINVAL;
    const uintptr_t s = reinterpret_cast<uintptr_t>(d.src), o = reinterpret_cast<uintptr_t>(d.dst);
    if (aligned && wide && ((s | o) & 15)) return TG_EINVAL;
    if (s < o + (uintptr_t)(d.n_rows_out * d.row_bytes) && o < s + (uintptr_t)(d.n_rows_src * d.row_bytes)) return TG_EINVAL;
  }
  return TG_OK;
}

// ---- bitmap -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NC_THREADS) k_nc_bitmap(const uint64_t* __restrict__ in, int64_t n_in,
                                                          const int32_t* __restrict__ old_of, int64_t n_out,
                                                          uint64_t* __restrict__ out, int64_t out_words) {
  const int lane = lane_id();
  const int64_t nwave = (int64_t)gridDim.x * NC_WAVES;
  for (int64_t w = (int64_t)blockIdx.x * NC_WAVES + threadIdx.x / TG_WAVE; w < out_words; w += nwave) {  // (wave-uniform)
    const int64_t j = w * 64 + lane;
    bool bit = false;
    if (j < n_out) {
      const int32_t o = old_of[j];
      if ((uint32_t)o < (uint64_t)n_in) bit = (in[o >> 6] >> (o & 63)) & 1ull;
    }
    const uint64_t word = __ballot(bit);
    if (lane == 0) out[w] = word;
  }
}

}  // namespace tg

using namespace tg;

extern "C" size_t tg_node_compact_workspace_bytes(int64_t N) {
  if (N < 1 || N > 0x7fffffffLL) return 0;
  return nc_layout(N).total;
}

extern "C" int tg_node_compact_plan(const tg_tcsr* g, const uint64_t* drop_bits, int64_t bit_words, int64_t N, int32_t* remap,
                                    int32_t* old_of, int64_t* indptr_out, int32_t* nbr_out, int64_t* out4, void* ws,
                                    size_t ws_bytes, void* stream) {
  if (int rc = nc_plan_args(g, drop_bits, bit_words, N, remap, old_of, indptr_out, nbr_out, out4)) return rc;
  const NcLayout l = nc_layout(N);
  if (int rc = ws_check(ws, ws_bytes, l.total)) return rc;  // before the first launch
  char* b = static_cast<char*>(ws);
  NcPlanArgs a{drop_bits, N, cdiv(N, 64), g->num_node, g->num_entry, g->indptr, g->nbr, remap, old_of, nbr_out, indptr_out, out4,
               reinterpret_cast<uint32_t*>(b + l.tcnt), reinterpret_cast<unsigned long long*>(b + l.errs),
               reinterpret_cast<int64_t*>(b + l.counts)};
  hipStream_t st = as_stream(stream);
  if (hipError_t e = hipMemsetAsync(a.errs, 0xff, 4 * sizeof(uint64_t), st)) {
    set_hip_error(e, "tg_node_compact_plan");
    return TG_EHIP;
  }
  hipLaunchKernelGGL(k_nc_count, dim3((unsigned)l.n_tile), dim3(NC_THREADS), 0, st, a);
  hipLaunchKernelGGL(k_nc_emit, dim3((unsigned)l.n_tile), dim3(NC_THREADS), 0, st, a);
  if (g->num_entry > 0)
    hipLaunchKernelGGL(k_nc_nbr, dim3((unsigned)cdiv(g->num_entry, NC_TILE)), dim3(NC_THREADS), 0, st, a);
  hipLaunchKernelGGL(k_nc_result, dim3(1), dim3(TG_WAVE), 0, st, a);
  return check_launch("tg_node_compact_plan");
}

extern "C" int tg_node_rows_compact(const tg_node_rows* tabs, int32_t n_tab, const int32_t* old_of, int64_t n_new, void* stream) {
  if (int rc = nc_rows_args(tabs, n_tab, old_of, n_new, true)) return rc;
  NcRowsArgs a{};
  a.old_of = old_of;
  int64_t tiles = 0;
  for (int i = 0; i < n_tab; ++i) {
    if (tabs[i].n_rows_out == 0) continue;  // (a table without output rows takes no workgroup)
    const int k = a.n_tab++;
    a.tab[k] = tabs[i];
    const int64_t d4 = tabs[i].row_bytes / 16;
    a.tile_rows[k] = d4 ? (uint32_t)std::min<int64_t>(NC_TILE_ROWS, std::max<int64_t>(1, NC_TILE_F4 / d4)) : (uint32_t)NC_TILE;
    a.tile0[k] = (uint32_t)tiles;
    tiles += cdiv(tabs[i].n_rows_out, a.tile_rows[k]);
    if (tiles > 0x7fffffffLL) return TG_EINVAL;
  }
  a.tile0[a.n_tab] = (uint32_t)tiles;
  if (tiles == 0) return TG_OK;
  hipLaunchKernelGGL(k_nc_rows, dim3((unsigned)tiles), dim3(NC_THREADS), 0, as_stream(stream), a);
  return check_launch("tg_node_rows_compact");
}

extern "C" int tg_bitmap_compact(const uint64_t* in, int64_t n_in, const int32_t* old_of, int64_t n_out, uint64_t* out,
                                 void* stream) {
  if (n_in < 0 || n_in > 0x7fffffffLL || n_out < 0 || n_out > 0x7fffffffLL || (n_in > 0 && !in)) return TG_EINVAL;
  if (n_out == 0) return TG_OK;
  if (!old_of || !out) return TG_EINVAL;
  const int64_t words = cdiv(n_out, 64);
  hipLaunchKernelGGL(k_nc_bitmap, dim3(flat_grid(words, NC_WAVES)), dim3(NC_THREADS), 0, as_stream(stream), in, n_in, old_of,
                     n_out, out, words);
  return check_launch("tg_bitmap_compact");
}

// The host twins: plain C++ over host pointers (those of `g` included), one id after the other.
extern "C" int tg_node_compact_plan_host(const tg_tcsr* g, const uint64_t* drop_bits, int64_t bit_words, int64_t N,
                                         int32_t* remap, int32_t* old_of, int64_t* indptr_out, int32_t* nbr_out, int64_t* out4) {
  if (int rc = nc_plan_args(g, drop_bits, bit_words, N, remap, old_of, indptr_out, nbr_out, out4)) return rc;
  int64_t first[4] = {-1, -1, -1, -1};
  if (drop_bits[0] & 1ull) first[0] = 0;
  const int64_t last = cdiv(N, 64) - 1;
  if (N % 64) {
    const uint64_t spare = drop_bits[last] & ~((1ull << (N % 64)) - 1ull);
    if (spare) first[1] = last * 64 + __builtin_ctzll(spare);
  }
  int64_t n = 0, n_graph = 0;
  for (int64_t i = 0; i < N; ++i) {
    const bool kept = !((drop_bits[i >> 6] >> (i & 63)) & 1ull);
    remap[i] = kept ? (int32_t)n : -1;
    if (i < g->num_node) {
      if (kept) indptr_out[n] = g->indptr[i];
      else if (g->indptr[i + 1] != g->indptr[i] && first[2] < 0) first[2] = i;
    }
    if (kept) old_of[n++] = (int32_t)i;
    if (i == g->num_node - 1) n_graph = n;
  }
  indptr_out[n_graph] = g->indptr[g->num_node];
  for (int64_t p = 0; p < g->num_entry; ++p) {
    const int32_t v = g->nbr[p];
    const int32_t r = (uint32_t)v < (uint64_t)g->num_node ? remap[v] : -1;
    nbr_out[p] = r;
    if (r < 0 && first[3] < 0) first[3] = p;
  }
  out4[0] = n;
  out4[1] = n_graph;
  out4[2] = 0;
  out4[3] = -1;
  for (int c = 3; c >= 0; --c)
    if (first[c] >= 0) {
      out4[2] = c + 1;
      out4[3] = first[c];
    }
  return TG_OK;
}

extern "C" int tg_node_rows_compact_host(const tg_node_rows* tabs, int32_t n_tab, const int32_t* old_of, int64_t n_new) {
  if (int rc = nc_rows_args(tabs, n_tab, old_of, n_new, false)) return rc;
  for (int i = 0; i < n_tab; ++i) {
    const tg_node_rows& d = tabs[i];
    for (int64_t j = 0; j < d.n_rows_out; ++j) {
      const int32_t o = old_of[j];
      if ((uint32_t)o < (uint64_t)d.n_rows_src)
        std::memcpy(static_cast<char*>(d.dst) + j * d.row_bytes, static_cast<const char*>(d.src) + (int64_t)o * d.row_bytes,
                    (size_t)d.row_bytes);
    }
  }
  return TG_OK;
}

extern "C" int tg_bitmap_compact_host(const uint64_t* in, int64_t n_in, const int32_t* old_of, int64_t n_out, uint64_t* out) {
  if (n_in < 0 || n_in > 0x7fffffffLL || n_out < 0 || n_out > 0x7fffffffLL || (n_in > 0 && !in)) return TG_EINVAL;
  if (n_out == 0) return TG_OK;
  if (!old_of || !out) return TG_EINVAL;
  const int64_t words = cdiv(n_out, 64);
  for (int64_t w = 0; w < words; ++w) out[w] = 0;
  for (int64_t j = 0; j < n_out; ++j) {
    const int32_t o = old_of[j];
    if ((uint32_t)o < (uint64_t)n_in && ((in[o >> 6] >> (o & 63)) & 1ull)) out[j >> 6] |= 1ull << (j & 63);
  }
  return TG_OK;
}
