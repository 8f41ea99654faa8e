// Involved list of a flat list of (node, time) queries: which nodes will the embeddings of these queries read, and which
// of them are not up to date yet?  The lazy restart of eval_utils.py:37-42 over the set GraphCollator.collate_memory_nodes
// builds (data_loader.py:105-131) - for queries whose neighbour lists nobody wants yet (ranking candidates, recommendation
// catalogues): the set is marked without writing a single slot array.
//
// involved = {nids[q]}  +  the K sampler slots of every (nids[q], ts[q])  (padding id 0 included, as the sampler marks it)
//            +  (two layers) the K slots of every hop-1 slot at the slot's float32 time (padding slots: node 0 at time 0).
//
// Launch 1 (k_involved_edges / k_involved_nodes), one wavefront per query; the enumeration itself lives in
// tg_involved_visit.h (shared with tg_snapshot_refresh.hip): the cut is prefix_end_group (strict float64),
// lane j holds hop-1 slot j in registers, the wavefront flags its query and its slots (byte flags, plain stores: every
// writer stores the same value) and then walks its own slots and flags their tails.  Nothing is written per slot.  All
// padding slots of a query are the same hop-2 query, searched once.  The batch's earliest time travels as the
// complemented orderable key of sample_batch_body (one atomicMax per workgroup).
// Launch 2 (k_involved_small, up to 65 536 nodes) packs the flags into bitmap words, lists flags & ~uptodate in ascending
// order (popcount per word, scan over the words, one wavefront per word and one lane per bit for the emission) and ORs
// the flags into the up-to-date bitmap.  Larger graphs split it at the scan (k_involved_pack, k_involved_emit: every
// workgroup of the second sums the totals of the workgroups in front of it).
// Integer work and comparisons only: device, host twin and numpy agree bit for bit.
#include <algorithm>
#include <cmath>
#include <vector>

#include "tg_involved_visit.h"

namespace tg {

struct InvolvedArgs {
  tg_tcsr g;
  int64_t Q;
  const int64_t* nids;
  const double* ts;
  int K;
  int two;  // second hop wanted
  uint8_t* flags;
  uint32_t* tmin_key;  // complemented order-preserving key of the earliest query time (starts at 0)
};

__device__ __forceinline__ void involved_mark(const InvolvedArgs& a, int64_t v) {
  if (v >= 0 && v < a.g.num_node) a.flags[v] = 1;
}

// the block's earliest time -> one atomic (as sample_batch_body)
__device__ __forceinline__ void involved_tmin(const InvolvedArgs& a, float tmin) {
  __shared__ float s_tmin[4];
  for (int sh = 32; sh > 0; sh >>= 1) tmin = fminf(tmin, __shfl_xor(tmin, sh, TG_WAVE));
  if (lane_id() == 0) s_tmin[threadIdx.x >> 6] = tmin;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float v = fminf(fminf(s_tmin[0], s_tmin[1]), fminf(s_tmin[2], s_tmin[3]));
    if (v < INFINITY) atomicMax(a.tmin_key, ~(uint32_t)orderable(v));
  }
}

// the marking visitor of tg_involved_visit.h: a byte per node, never stops
struct InvolvedMarker {
  const InvolvedArgs& a;
  __device__ __forceinline__ void visit(int64_t v) const { involved_mark(a, v); }
  __device__ __forceinline__ constexpr bool stop() const { return false; }
};

// recent_edges: involved_visit_edges<G>, one wavefront per query (K <= G)
template <int G>
__global__ void __launch_bounds__(256) k_involved_edges(InvolvedArgs a) {
  const int lane = lane_id();
  InvolvedMarker vis{a};
  float tmin = INFINITY;
  for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < a.Q; q += (int64_t)gridDim.x * 4) {
    const double t = a.ts[q];
    tmin = fminf(tmin, (float)t);
    involved_visit_edges<G>(a.g, a.nids[q], t, a.K, a.two != 0, lane, vis);
  }
  involved_tmin(a, tmin);
}

// recent_nodes: involved_visit_nodes, hop-1 slots parked in LDS
__global__ void __launch_bounds__(256) k_involved_nodes(InvolvedArgs a) {
  __shared__ int s_new[4][TG_WAVE];
  __shared__ float s_t[4][TG_WAVE];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  InvolvedMarker vis{a};
  float tmin = INFINITY;
  for (int64_t q = (int64_t)blockIdx.x * 4 + wv; q < a.Q; q += (int64_t)gridDim.x * 4) {
    const double t = a.ts[q];
    tmin = fminf(tmin, (float)t);
    involved_visit_nodes(a.g, a.nids[q], t, a.K, a.two != 0, lane, s_new[wv], s_t[wv], vis);
  }
  involved_tmin(a, tmin);
}

struct InvolvedEmitArgs {
  const uint8_t* flags;
  uint64_t* uptodate;
  int64_t W;  // bitmap words
  int64_t* list;
  int64_t cap;
  int32_t* count;
  float* tmin;
  const uint32_t* tmin_key;
  uint64_t* need;  // large graphs: flags & ~uptodate as bitmap words
  uint32_t* rank;  // large graphs: set bits of `need` in front of a word, within its 256-word block
  uint32_t* blk;   // large graphs: set bits of `need` per 256-word block
};

__device__ __forceinline__ float involved_tmin_value(const uint32_t* tmin_key) {
  uint32_t key = ~*tmin_key;  // inverse of orderable(float)
  key = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
  return __uint_as_float(key);
}

// one thread per word: the word of flags, what it adds to the list, and the up-to-date bitmap (one writer per word)
__device__ __forceinline__ uint64_t involved_word(const InvolvedEmitArgs& a, int64_t w) {
  const uint64_t f = pack_flag_word(a.flags + w * 64);
  const uint64_t u = a.uptodate[w];
  if (f & ~u) a.uptodate[w] = u | f;
  return f & ~u;
}

// one lane per bit of word w: the ids of its set bits, ascending, from position `base` on
__device__ __forceinline__ void involved_emit_word(const InvolvedEmitArgs& a, int64_t w, uint64_t need, uint32_t base, int lane) {
  const uint32_t mine = base + (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
  if (((need >> lane) & 1ull) && (int64_t)mine < a.cap) a.list[mine] = w * 64 + lane;
}

constexpr int IB = 1024;  // k_involved_small: threads = words
__global__ void __launch_bounds__(IB) k_involved_small(InvolvedEmitArgs a) {
  constexpr int NWV = IB / TG_WAVE;
  __shared__ uint32_t s_wave[NWV];
  __shared__ uint64_t s_need[IB];
  __shared__ uint32_t s_rank[IB];
  const int w = threadIdx.x, lane = lane_id(), wv = threadIdx.x >> 6;
  const uint64_t need = w < a.W ? involved_word(a, w) : 0ull;
  const uint32_t cnt = (uint32_t)__popcll(need);
  uint32_t inc = cnt;
#pragma unroll
  for (int o = 1; o < TG_WAVE; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, TG_WAVE);
    if (lane >= o) inc += t;
  }
  if (lane == TG_WAVE - 1) s_wave[wv] = inc;
  __syncthreads();
  uint32_t base = 0, total = 0;
#pragma unroll
  for (int i = 0; i < NWV; ++i) {
    const uint32_t x = s_wave[i];
    if (i < wv) base += x;
    total += x;
  }
  s_need[w] = need;
  s_rank[w] = base + inc - cnt;
  if (w == 0) {
    *a.count = (int32_t)total;
    *a.tmin = involved_tmin_value(a.tmin_key);
  }
  __syncthreads();
  for (int ww = wv; ww < a.W; ww += NWV) involved_emit_word(a, ww, s_need[ww], s_rank[ww], lane);
}

__global__ void __launch_bounds__(TG_SCAN_BLOCK) k_involved_pack(InvolvedEmitArgs a) {
  __shared__ uint32_t s_w[TG_SCAN_BLOCK / TG_WAVE];
  const int64_t w = (int64_t)blockIdx.x * TG_SCAN_BLOCK + threadIdx.x;
  const uint64_t need = w < a.W ? involved_word(a, w) : 0ull;
  uint32_t total;
  const uint32_t r = block_excl_scan((uint32_t)__popcll(need), s_w, &total);
  if (w < a.W) {
    a.need[w] = need;
    a.rank[w] = r;
  }
  if (threadIdx.x == 0) a.blk[blockIdx.x] = total;
}

// workgroup b lists the words of block b of k_involved_pack
__global__ void __launch_bounds__(TG_SCAN_BLOCK) k_involved_emit(InvolvedEmitArgs a) {
  __shared__ uint32_t s_w[TG_SCAN_BLOCK / TG_WAVE];
  const uint32_t base = block_sum_front(a.blk, blockIdx.x, s_w);  // set bits in front of this block
  const int lane = lane_id();
  const int64_t w0 = (int64_t)blockIdx.x * TG_SCAN_BLOCK, w1 = min(a.W, w0 + TG_SCAN_BLOCK);
  for (int64_t w = w0 + (threadIdx.x >> 6); w < w1; w += TG_SCAN_BLOCK / TG_WAVE)
    involved_emit_word(a, w, a.need[w], base + a.rank[w], lane);
  if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1) {
    *a.count = (int32_t)(base + a.blk[blockIdx.x]);
    *a.tmin = involved_tmin_value(a.tmin_key);
  }
}

static inline size_t inv_align(size_t x) { return (x + 15) & ~(size_t)15; }

struct InvolvedLayout {
  size_t flags, key, need, rank, blk, total;
};
// flags | key (zeroed together) | need | rank | blk.  No term in Q: nothing is kept per query or per slot
static InvolvedLayout involved_layout(int64_t n_nodes) {
  const int64_t W = (n_nodes + 63) / 64;
  InvolvedLayout l{};
  l.flags = 0;
  l.key = (size_t)W * 64;
  l.need = l.key + 16;
  l.rank = l.need + inv_align((size_t)W * sizeof(uint64_t));
  l.blk = l.rank + inv_align((size_t)W * sizeof(uint32_t));
  l.total = l.blk + inv_align((size_t)cdiv(W, TG_SCAN_BLOCK) * sizeof(uint32_t));
  return l;
}

static int involved_args(const tg_tcsr* g, int64_t Q, const int64_t* nids, const double* ts, int32_t K, int32_t n_layers,
                         int32_t strategy, const uint64_t* uptodate, int64_t cap, const int64_t* list, const int32_t* count,
                         const float* tmin) {
  if (!g || g->num_node <= 0 || g->num_entry < 0 || Q < 0) return TG_EINVAL;
  if (K < 1 || K > TG_INVOLVED_MAX_K || (n_layers != 1 && n_layers != 2)) return TG_EINVAL;
  if (strategy < 0 || strategy > 2) return TG_EINVAL;
  if (strategy == 2) return TG_EUNSUPPORTED;
  if (!count) return TG_EINVAL;
  if (Q == 0) return TG_OK;
  if (!nids || !ts || !uptodate || !list || !tmin || !g->indptr || (g->num_entry > 0 && (!g->ts || !g->nbr))) return TG_EINVAL;
  const int64_t per_query = 1 + (int64_t)K + (n_layers == 2 ? (int64_t)K * K : 0);
  const int64_t bound = Q > g->num_node / per_query ? g->num_node : std::min(Q * per_query, g->num_node);
  if (cap < bound) return TG_EINVAL;
  return TG_OK;
}

}  // namespace tg

using namespace tg;

extern "C" size_t tg_involved_list_workspace_bytes(int64_t n_nodes, int64_t Q, int32_t K, int32_t n_layers) {
  if (n_nodes <= 0 || Q < 0 || K < 1 || K > TG_INVOLVED_MAX_K || (n_layers != 1 && n_layers != 2)) return 0;
  return involved_layout(n_nodes).total;
}

extern "C" int tg_involved_list(const tg_tcsr* g, int64_t Q, const int64_t* nids, const double* ts, int32_t K,
                                int32_t n_layers, int32_t strategy, uint64_t* uptodate, int64_t cap, int64_t* list,
                                int32_t* count, float* tmin, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = involved_args(g, Q, nids, ts, K, n_layers, strategy, uptodate, cap, list, count, tmin)) return rc;
  hipStream_t st = as_stream(stream);
  if (Q == 0) {
    const hipError_t e = hipMemsetAsync(count, 0, sizeof(int32_t), st);
    if (e != hipSuccess) {
      set_hip_error(e, "tg_involved_list memset");
      return TG_EHIP;
    }
    return TG_OK;
  }
  const InvolvedLayout l = involved_layout(g->num_node);
  if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15)) return TG_EINVAL;
  if (ws_bytes < l.total) return TG_EINVAL;
  char* base = static_cast<char*>(ws);
  const int64_t W = (g->num_node + 63) / 64;
  const hipError_t e = hipMemsetAsync(base, 0, l.need, st);  // flags and the key
  if (e != hipSuccess) {
    set_hip_error(e, "tg_involved_list memset");
    return TG_EHIP;
  }
  InvolvedArgs a{*g, Q, nids, ts, K, n_layers == 2 ? 1 : 0, reinterpret_cast<uint8_t*>(base + l.flags),
                 reinterpret_cast<uint32_t*>(base + l.key)};
  const dim3 grid(flat_grid(Q, 4));
  if (strategy == 1)
    hipLaunchKernelGGL(k_involved_nodes, grid, dim3(256), 0, st, a);
  else if (K <= 16)
    hipLaunchKernelGGL(k_involved_edges<16>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(k_involved_edges<64>, grid, dim3(256), 0, st, a);
  if (int rc = check_launch("tg_involved_list(mark)")) return rc;
  InvolvedEmitArgs b{a.flags, uptodate, W, list, cap, count, tmin, a.tmin_key, reinterpret_cast<uint64_t*>(base + l.need),
                     reinterpret_cast<uint32_t*>(base + l.rank), reinterpret_cast<uint32_t*>(base + l.blk)};
  if (W <= IB) {
    hipLaunchKernelGGL(k_involved_small, dim3(1), dim3(IB), 0, st, b);
    return check_launch("tg_involved_list(list)");
  }
  const dim3 wgrid((unsigned)cdiv(W, TG_SCAN_BLOCK));
  hipLaunchKernelGGL(k_involved_pack, wgrid, dim3(TG_SCAN_BLOCK), 0, st, b);
  hipLaunchKernelGGL(k_involved_emit, wgrid, dim3(TG_SCAN_BLOCK), 0, st, b);
  return check_launch("tg_involved_list(list)");
}

extern "C" int tg_involved_list_host(const tg_tcsr* g, int64_t Q, const int64_t* nids_host, const double* ts_host, int32_t K,
                                     int32_t n_layers, int32_t strategy, uint64_t* uptodate_host, int64_t cap,
                                     int64_t* list_host, int32_t* count_host, float* tmin_host) {
  if (int rc = involved_args(g, Q, nids_host, ts_host, K, n_layers, strategy, uptodate_host, cap, list_host, count_host,
                             tmin_host))
    return rc;
  *count_host = 0;
  if (Q == 0) return TG_OK;
  for (int64_t q = 0; q < Q; ++q)
    if (nids_host[q] < 0 || nids_host[q] >= g->num_node) return TG_EINVAL;
  std::vector<uint8_t> flags((size_t)g->num_node, 0);
  std::vector<int64_t> hop1, hop2;
  double t_first = ts_host[0];
  for (int64_t q = 0; q < Q; ++q) {
    t_first = std::min(t_first, ts_host[q]);
    host_involved_visit(g, nids_host[q], ts_host[q], K, n_layers, strategy, hop1, hop2, [&](int64_t v) {
      flags[v] = 1;
      return false;
    });
  }
  int64_t n = 0;
  for (int64_t v = 0; v < g->num_node; ++v) {
    if (!flags[v]) continue;
    uint64_t& word = uptodate_host[v >> 6];
    const uint64_t bit = 1ull << (v & 63);
    if (!(word & bit)) {
      if (n < cap) list_host[n] = v;
      ++n;
      word |= bit;
    }
  }
  *count_host = (int32_t)n;
  *tmin_host = (float)t_first;
  return TG_OK;
}
