// Erasing nodes and retracting events from the T-CSR (online serving; reference tiger/data/graph.py:11-42: the reference
// builds its adjacency lists once over the whole stream and never takes a node or an event out - it has no counterpart
// of this).
//
// An entry p of row v is DROPPED iff node_bits has bit v (the owner is erased), node_bits has bit nbr[p] (the partner is
// erased) or eid_bits has bit eid[p] & 0x7FFFFFFF (the event is retracted; an eid >= n_rows is never matched).  Every other
// entry is kept with its time, neighbour, eid (bit 31 included) and order.  Unlike a trim (tg_trim.hip: every row keeps a
// suffix; what the two share is in tg_tcsr.h) an arbitrary subset of every row goes, so this is a stable stream compaction over the ENTRIES; the rows follow
// from where their first old entry lands.  All passes are entry-parallel over tiles of ES_TILE = 2048 OLD entries: a hub
// row is spread over as many workgroups as it has tiles.
//   flags  (k_erase_flags, one workgroup per tile): lane l takes entries base + l + 256 i: loads coalesce.  The owner of
//           an entry is an upper bound in indptr; the workgroup searches once for the owners of its first and last entry
//           and stages that window of indptr in LDS (row_window, tg_tcsr.h: up to ES_WIN rows; a tile that spans more -
//           thousands of empty rows - searches global memory).  No owner is looked for without node_bits.  The keep flags leave as ballot words,
//           1 bit per entry in entry order (32 words of 64 bits per tile, bits past num_entry are 0), and one kept-count
//           per tile.
//   bases  (k_erase_bases, one workgroup per 256 tiles): workgroup b sums the counts of the tiles in front of its chunk
//           (block_sum_front: no third scan launch) and scans its own: base[s] = kept entries in front of tile s,
//           s in [0, n_tile]; base[n_tile] is the total.
//   ptr    (k_erase_ptr, one workgroup per 256 of the num_node + 1 row bounds): indptr_out[v] = base of indptr[v]'s
//           tile + the popcount of the keep bits in front of indptr[v] inside that tile (at most 31 words and a part).
//   apply  (k_erase_apply, one workgroup per tile): the tile's 32 keep words and their exclusive popcount scan go to LDS;
//           a kept entry lands at base + scan[word] + popcount(bits below its own).  Loads coalesce as in `flags`, the
//           stores of a tile are one contiguous run, ascending with the lane inside every wavefront.
// Workspace: 8 B * 32 * n_tile (the keep words: num_entry / 8 bytes, rounded up to whole tiles) + 4 B * n_tile (counts)
// + 4 B * (n_tile + 1) (bases), each part rounded up to 16 bytes; n_tile = ceil(num_entry / 2048).
// No atomics (the result does not depend on the launch geometry), no grid is capped (every workgroup owns one tile /
// chunk), integer work and bit copies: device, host twin and numpy agree bit for bit.
#include <algorithm>

#include "tg_tcsr.h"
#include "tg_step.h"

namespace tg {

constexpr int ES_THREADS = TG_SCAN_BLOCK;              // block_excl_scan: 256
constexpr int ES_ITEMS = 8;
constexpr int ES_TILE = ES_THREADS * ES_ITEMS;         // old entries per workgroup
constexpr int ES_WORDS = ES_TILE / 64;                 // keep words per tile
constexpr int ES_WAVES = ES_THREADS / TG_WAVE;
constexpr int ES_WIN = 2048;                           // rows of one tile staged in LDS (more: searched in global memory)

struct EraseFlagArgs {
  tg_tcsr g;
  const uint64_t* node_bits;  // over g.num_node ids, or NULL
  const uint64_t* eid_bits;   // over n_rows ids, or NULL
  int64_t n_rows;
  uint64_t* words;            // [n_tile * ES_WORDS]
  uint32_t* cnt;              // [n_tile]
};
__global__ void __launch_bounds__(ES_THREADS) k_erase_flags(EraseFlagArgs a) {
  __shared__ uint32_t win[ES_WIN];  // indptr[lo + 1 .. hi]: where the rows after the tile's first one begin
  __shared__ uint32_t s_cnt[ES_WAVES];
  const uint32_t t = threadIdx.x, lane = t & (TG_WAVE - 1), wv = t / TG_WAVE;
  const int64_t N = a.g.num_node, P = a.g.num_entry;
  const int64_t p0 = (int64_t)blockIdx.x * ES_TILE, p1 = min(p0 + ES_TILE, P);
  RowWindow w{};
  if (a.node_bits) {  // (no owner is looked for without node_bits: no window, no search)
    w = row_window<ES_THREADS>(a.g.indptr, N, p0, p1 - 1, win, ES_WIN);
    if (w.staged) __syncthreads();
  }
  uint32_t kept = 0;  // (the same value on every lane of a wavefront)
#pragma unroll
  for (int i = 0; i < ES_ITEMS; ++i) {
    const int64_t p = p0 + (int64_t)i * ES_THREADS + t;
    bool keep = false;
    if (p < p1) {
      keep = true;
      if (a.node_bits) {
        const int64_t v = w.owner(p);
        const int64_t u = (int64_t)a.g.nbr[p];
        if (bm_test(a.node_bits, v)) keep = false;
        if (u >= 0 && u < N && bm_test(a.node_bits, u)) keep = false;  // (an id that is no node: no bit to read)
      }
      if (a.eid_bits) {
        const int64_t e = (int64_t)((uint32_t)a.g.eid[p] & 0x7fffffffu);
        if (e < a.n_rows && bm_test(a.eid_bits, e)) keep = false;
      }
    }
    const uint64_t word = __ballot(keep);  // bit l: entry p0 + 256 i + 64 wv + l
    if (lane == 0) a.words[(int64_t)blockIdx.x * ES_WORDS + i * ES_WAVES + wv] = word;
    kept += (uint32_t)__popcll(word);
  }
  if (lane == 0) s_cnt[wv] = kept;
  __syncthreads();
  if (t == 0) {
    uint32_t c = 0;
#pragma unroll
    for (int w = 0; w < ES_WAVES; ++w) c += s_cnt[w];
    a.cnt[blockIdx.x] = c;
  }
}

// workgroup b: slots [256 b, 256 b + 256) of base[0 .. n_tile]
__global__ void __launch_bounds__(ES_THREADS) k_erase_bases(int64_t n_tile, const uint32_t* __restrict__ cnt,
                                                            uint32_t* __restrict__ base) {
  __shared__ uint32_t s_w[ES_WAVES];
  const int64_t s0 = (int64_t)blockIdx.x * ES_THREADS;
  const uint32_t front = block_sum_front(cnt, (uint32_t)s0, s_w);  // kept entries in front of this chunk (s0 <= n_tile < 2^22)
  const int64_t s = s0 + threadIdx.x;
  uint32_t total;
  const uint32_t r = block_excl_scan(s < n_tile ? cnt[s] : 0u, s_w, &total);
  if (s <= n_tile) base[s] = front + r;
}

// kept entries in front of old position p (0 <= p <= num_entry)
__device__ __forceinline__ uint32_t es_rank_of(const uint64_t* __restrict__ words, const uint32_t* __restrict__ base,
                                               int64_t p) {
  const int64_t tile = p / ES_TILE;
  const uint32_t off = (uint32_t)(p % ES_TILE);  // (off == 0: no word is read - tile may be n_tile, which has none)
  const uint64_t* __restrict__ w = words + tile * ES_WORDS;
  uint32_t r = base[tile];
  const uint32_t full = off / 64, part = off % 64;
  for (uint32_t j = 0; j < full; ++j) r += (uint32_t)__popcll(w[j]);
  if (part) r += (uint32_t)__popcll(w[full] & ((1ull << part) - 1ull));
  return r;
}

__global__ void __launch_bounds__(ES_THREADS) k_erase_ptr(tg_tcsr g, const uint64_t* __restrict__ words,
                                                          const uint32_t* __restrict__ base,
                                                          int64_t* __restrict__ indptr_out) {
  const int64_t v = (int64_t)blockIdx.x * ES_THREADS + threadIdx.x;
  if (v > g.num_node) return;
  // (an indptr that is no row bound of this graph: nothing is read out of bounds)
  const int64_t p = min(max(g.indptr[v], (int64_t)0), g.num_entry);
  indptr_out[v] = (int64_t)es_rank_of(words, base, p);
}

struct EraseApplyArgs {
  tg_tcsr g;
  const uint64_t* words;
  const uint32_t* base;
  int64_t P_out;  // kept entries
  double* ts_out;
  int32_t *nbr_out, *eid_out;
};
__global__ void __launch_bounds__(ES_THREADS) k_erase_apply(EraseApplyArgs a) {
  __shared__ uint64_t s_word[ES_WORDS];
  __shared__ uint32_t s_pref[ES_WORDS];  // kept entries of the tile in front of word j
  const uint32_t t = threadIdx.x, lane = t & (TG_WAVE - 1), wv = t / TG_WAVE;
  const int64_t p0 = (int64_t)blockIdx.x * ES_TILE;
  if (t < TG_WAVE) {  // the first wavefront: 32 words, a shuffle scan of their popcounts
    const uint64_t w = t < ES_WORDS ? a.words[(int64_t)blockIdx.x * ES_WORDS + t] : 0ull;
    const uint32_t c = (uint32_t)__popcll(w);
    uint32_t inc = c;
#pragma unroll
    for (int o = 1; o < ES_WORDS; o <<= 1) {
      const uint32_t x = __shfl_up(inc, o, TG_WAVE);
      if (lane >= (uint32_t)o) inc += x;
    }
    if (t < ES_WORDS) {
      s_word[t] = w;
      s_pref[t] = inc - c;
    }
  }
  __syncthreads();
  const int64_t q0 = (int64_t)a.base[blockIdx.x];
#pragma unroll
  for (int i = 0; i < ES_ITEMS; ++i) {
    const int j = i * ES_WAVES + (int)wv;
    const uint64_t w = s_word[j];
    if (!((w >> lane) & 1ull)) continue;
    const int64_t p = p0 + (int64_t)i * ES_THREADS + t;
    const int64_t q = q0 + (int64_t)s_pref[j] + (int64_t)__popcll(w & ((1ull << lane) - 1ull));
    if (p >= a.g.num_entry || q >= a.P_out) continue;  // (a workspace that is no plan of this graph: nothing out of bounds)
    move_entry(a.g, p, a.ts_out, a.nbr_out, a.eid_out, q);
  }
}

struct EraseLayout {
  int64_t n_tile;
  size_t words, cnt, base, total;
};
static EraseLayout erase_layout(int64_t num_entry) {
  EraseLayout l{};
  l.n_tile = cdiv(num_entry, ES_TILE);
  l.words = 0;
  l.cnt = l.words + align16((size_t)l.n_tile * ES_WORDS * sizeof(uint64_t));
  l.base = l.cnt + align16((size_t)l.n_tile * sizeof(uint32_t));
  l.total = l.base + align16((size_t)(l.n_tile + 1) * sizeof(uint32_t));
  return l;
}

static inline bool host_bit(const int64_t* bits, int64_t id) { return ((uint64_t)bits[id >> 6] >> (id & 63)) & 1ull; }

}  // namespace tg

using namespace tg;

extern "C" size_t tg_tcsr_erase_workspace_bytes(int64_t num_node, int64_t num_entry) {
  if (num_node <= 0 || num_node > 0x7fffffffLL || num_entry < 0 || num_entry > 0xffffffffLL) return 0;
  return erase_layout(num_entry).total;
}

extern "C" int tg_tcsr_erase_plan(const tg_tcsr* g, const int64_t* node_bits, const int64_t* eid_bits, int64_t n_rows,
                                  int64_t* indptr_out, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = tcsr_args(g)) return rc;
  if (!indptr_out || n_rows < 0) return TG_EINVAL;
  const EraseLayout l = erase_layout(g->num_entry);
  if (int rc = ws_check(ws, ws_bytes, l.total)) return rc;  // before the first launch
  hipStream_t st = as_stream(stream);
  char* base = static_cast<char*>(ws);
  uint64_t* words = reinterpret_cast<uint64_t*>(base + l.words);
  uint32_t* cnt = reinterpret_cast<uint32_t*>(base + l.cnt);
  uint32_t* tb = reinterpret_cast<uint32_t*>(base + l.base);
  if (l.n_tile > 0) {
    EraseFlagArgs a{*g, reinterpret_cast<const uint64_t*>(node_bits), reinterpret_cast<const uint64_t*>(eid_bits), n_rows,
                    words, cnt};
    hipLaunchKernelGGL(k_erase_flags, dim3((unsigned)l.n_tile), dim3(ES_THREADS), 0, st, a);
  }
  hipLaunchKernelGGL(k_erase_bases, dim3((unsigned)cdiv(l.n_tile + 1, ES_THREADS)), dim3(ES_THREADS), 0, st, l.n_tile, cnt, tb);
  hipLaunchKernelGGL(k_erase_ptr, dim3((unsigned)cdiv(g->num_node + 1, ES_THREADS)), dim3(ES_THREADS), 0, st, *g, words, tb,
                     indptr_out);
  return check_launch("tg_tcsr_erase_plan");
}

extern "C" int tg_tcsr_erase_apply(const tg_tcsr* g, const int64_t* indptr_out, int64_t num_entry_out, double* ts_out,
                                   int32_t* nbr_out, int32_t* eid_out, const void* ws, size_t ws_bytes, void* stream) {
  if (int rc = tcsr_args(g)) return rc;
  if (!indptr_out || num_entry_out < 0 || num_entry_out > g->num_entry) return TG_EINVAL;
  if (num_entry_out > 0 && (!ts_out || !nbr_out || !eid_out)) return TG_EINVAL;
  const EraseLayout l = erase_layout(g->num_entry);
  if (int rc = ws_check(ws, ws_bytes, l.total)) return rc;
  if (num_entry_out == 0) return TG_OK;
  const char* base = static_cast<const char*>(ws);
  EraseApplyArgs a{*g, reinterpret_cast<const uint64_t*>(base + l.words), reinterpret_cast<const uint32_t*>(base + l.base),
                   num_entry_out, ts_out, nbr_out, eid_out};
  hipLaunchKernelGGL(k_erase_apply, dim3((unsigned)l.n_tile), dim3(ES_THREADS), 0, as_stream(stream), a);
  return check_launch("tg_tcsr_erase_apply");
}

// The host twin: plain C++ over host pointers.
extern "C" int tg_tcsr_erase_host(const tg_tcsr* g, const int64_t* node_bits, const int64_t* eid_bits, int64_t n_rows,
                                  int64_t* indptr_out, double* ts_out, int32_t* nbr_out, int32_t* eid_out,
                                  int64_t* num_entry_out) {
  if (int rc = tcsr_args(g)) return rc;
  if (!indptr_out || !num_entry_out || n_rows < 0) return TG_EINVAL;
  if (g->num_entry > 0 && (!ts_out || !nbr_out || !eid_out)) return TG_EINVAL;
  int64_t q = 0;
  for (int64_t v = 0; v < g->num_node; ++v) {
    const int64_t b = std::min(std::max(g->indptr[v], (int64_t)0), g->num_entry);
    const int64_t e = std::min(std::max(g->indptr[v + 1], (int64_t)0), g->num_entry);
    indptr_out[v] = q;
    if (node_bits && host_bit(node_bits, v)) continue;  // an erased node owns an empty row
    for (int64_t p = b; p < e; ++p) {
      const int64_t u = (int64_t)g->nbr[p];
      if (node_bits && u >= 0 && u < g->num_node && host_bit(node_bits, u)) continue;
      const int64_t r = (int64_t)((uint32_t)g->eid[p] & 0x7fffffffu);
      if (eid_bits && r < n_rows && host_bit(eid_bits, r)) continue;
      ts_out[q] = g->ts[p];
      nbr_out[q] = g->nbr[p];
      eid_out[q] = g->eid[p];
      ++q;
    }
  }
  indptr_out[g->num_node] = q;
  *num_entry_out = q;
  return TG_OK;
}
