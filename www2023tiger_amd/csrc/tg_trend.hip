// Trending candidates (tiger_hip.h: tg_trending, tg_fill_candidates; no counterpart in the reference): which nodes were most
// active in a time window, and a shared list of such nodes appended to per-query candidate rows under the walk's rules.
//
// tg_trending.  c(v) = prefix_end(v, t_hi) - prefix_end(v, t_lo), strict float64 '<' (the cut of every sampler), over the
// eligible nodes (`among`, or every node but 0); the T best by (c descending, id ascending).
//   k_window_keys   one 16-lane group per eligible node (prefix_end_group<16>, both bounds), capped grid that loops; writes
//                   the key (c << 32) | (0xFFFFFFFF - id), 0 where c == 0, for node 0 and for an id outside the graph, into
//                   the workspace, which is padded with zero keys to whole tiles
//   k_trend_tiles   one workgroup per tile of 2 048 keys: bitonic sort (descending) in LDS, the sorted tile written back IN
//                   PLACE - its first T keys are the tile's run - and the tile's number of non-zero keys beside it.  A call
//                   of one tile writes the outputs here: two launches.
//   k_trend_merge   sixteen runs per workgroup -> one run of T keys, by RANK: the non-zero keys are distinct, so the place of
//                   a key in the union is its place in its own run plus, for every other run, the number of keys above it
//                   (a binary search: one 16-lane group per run, one lane per other run); keys ranked T or beyond are
//                   dropped, places behind the last key are zeroed, the counts are added.  Rounds until one run is left
//                   (three cover 10^7 nodes); the last one writes the outputs.
// The number of launches depends on M (or num_node) alone; nothing is read back; no atomics at all.  The order is total on
// the keys, so where a key sits in `among`, in a tile or in a run is invisible.
//
// tg_fill_candidates.  One 256-thread workgroup per query, capped grid.  The fill list is shared: a workgroup builds an
// open-addressing LDS table id -> first position ONCE (the walk's multiplicative hash, linear probing, >= 2 T slots: never
// more than half full) together with a byte per position that is set for what no query takes (id 0, an id outside
// [1, 2^31), a repeated id's later positions, positions at and behind *n_fill).  Per query: the bytes are copied into the
// query's flags; the row's ids, the source and - exclude_seen - the source's whole prefix, 256 entries per pass, flag what
// they hit; a block prefix scan over the flags in position order hands every unflagged id its place behind the row.  A
// full row leaves before any of that.  No global atomics, no workspace.  Integer work only: device, host twin and a numpy
// reference agree bit for bit.
#include <algorithm>
#include <cmath>
#include <unordered_set>
#include <vector>

#include "tg_sample.h"
#include "tg_tcsr.h"

namespace tg {

constexpr int TR_THREADS = 256;
constexpr int TR_G = 16;                      // lanes per search
constexpr int TR_GROUPS = TR_THREADS / TR_G;  // nodes per workgroup and pass
constexpr int TR_TILE = 2048;                 // keys per sorted tile
constexpr int TR_WAYS = 16;                   // runs merged per workgroup
constexpr size_t TR_STAGE_MAX = 64 * 1024;    // a merge whose runs fit into this much LDS searches them there

__host__ __device__ __forceinline__ uint64_t trend_key(int64_t c, int64_t id) {
  return ((uint64_t)(uint32_t)c << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)id);
}

struct TrendOut {
  int T;
  int64_t* ids;
  int32_t* counts;
  int32_t* n_valid;
  int32_t* n_distinct;
};

__device__ __forceinline__ void trend_emit(const TrendOut& o, int j, uint64_t key) {
  o.ids[j] = key ? (int64_t)(0xFFFFFFFFu - (uint32_t)key) : (int64_t)0;
  o.counts[j] = (int32_t)(key >> 32);
}

// keys[i] for i in [0, n_pad): eligible node i (among[i], or i itself) for i < n, zero behind
__global__ void __launch_bounds__(TR_THREADS) k_window_keys(tg_tcsr g, double t_lo, double t_hi, const int64_t* among, int64_t n,
                                                            int64_t n_pad, uint64_t* keys) {
  const int sub = threadIdx.x % TR_G, grp = threadIdx.x / TR_G;
  for (int64_t base = (int64_t)blockIdx.x * TR_GROUPS; base < n_pad; base += (int64_t)gridDim.x * TR_GROUPS) {  // (uniform)
    const int64_t i = base + grp;
    const int64_t v = i < n ? (among ? among[i] : i) : -1;  // outside the graph: no entries
    int64_t start;
    const int64_t hi = prefix_end_group<TR_G>(g, v, t_hi, &start, sub);
    const int64_t lo = prefix_end_group<TR_G>(g, v, t_lo, &start, sub);
    const int64_t c = hi - lo;  // t_lo <= t_hi: never negative
    if (sub == 0 && i < n_pad) keys[i] = (c > 0 && v > 0) ? trend_key(c, v) : 0ull;
  }
}

// tile b: keys[b 2048, (b + 1) 2048) sorted descending in place, cnt[b] = its non-zero keys; `single`: the outputs
__global__ void __launch_bounds__(TR_THREADS) k_trend_tiles(uint64_t* keys, int32_t* cnt, int single, TrendOut o) {
  __shared__ uint64_t s_keys[TR_TILE];
  __shared__ int s_n;
  const int tid = threadIdx.x;
  uint64_t* tile = keys + (int64_t)blockIdx.x * TR_TILE;
  for (int i = tid; i < TR_TILE; i += TR_THREADS) s_keys[i] = tile[i];
  __syncthreads();
  // a step has 1 024 disjoint pairs (i, i | j), four per thread: all eight keys are read before any is written, so the LDS
  // round trips of a step overlap (a loop over i that may write what its next turn reads takes them one by one)
  constexpr int PAIRS = TR_TILE / 2 / TR_THREADS;
  for (int k = 2; k <= TR_TILE; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      uint64_t lo[PAIRS], hi[PAIRS];
#pragma unroll
      for (int m = 0; m < PAIRS; ++m) {
        const int pr = tid + m * TR_THREADS;
        const int i = ((pr & ~(j - 1)) << 1) | (pr & (j - 1));  // pr with a zero bit put in at j's place
        lo[m] = s_keys[i];
        hi[m] = s_keys[i | j];
      }
#pragma unroll
      for (int m = 0; m < PAIRS; ++m) {
        const int pr = tid + m * TR_THREADS;
        const int i = ((pr & ~(j - 1)) << 1) | (pr & (j - 1));
        const bool desc = (i & k) == 0;
        const bool swap = desc ? lo[m] < hi[m] : lo[m] > hi[m];
        s_keys[i] = swap ? hi[m] : lo[m];
        s_keys[i | j] = swap ? lo[m] : hi[m];
      }
      __syncthreads();
    }
  }
  // the non-zero keys are in front: the one that has a zero (or the end) behind it is the last
  if (tid == 0 && s_keys[0] == 0ull) s_n = 0;
  for (int i = tid; i < TR_TILE; i += TR_THREADS)
    if (s_keys[i] != 0ull && (i + 1 == TR_TILE || s_keys[i + 1] == 0ull)) s_n = i + 1;
  __syncthreads();
  if (single) {
    const int n = s_n;
    for (int j = tid; j < o.T; j += TR_THREADS) trend_emit(o, j, s_keys[j]);  // T <= 2 048; zero keys behind the last
    if (tid == 0) {
      *o.n_valid = n < o.T ? n : o.T;
      *o.n_distinct = n;
    }
  } else {
    for (int i = tid; i < TR_TILE; i += TR_THREADS) tile[i] = s_keys[i];
    if (tid == 0) cnt[blockIdx.x] = s_n;
  }
}

// the number of keys above x in a run of T keys sorted descending: a search of fixed length (P = the largest power of two
// <= T) whose loads do not depend on a branch, so several of them overlap
__device__ __forceinline__ int trend_above(const uint64_t* run, int T, int P, uint64_t x) {
  int pos = 0;
  for (int step = P; step > 0; step >>= 1) {
    const int nxt = pos + step;
    const uint64_t v = run[(nxt <= T ? nxt : T) - 1];
    if (nxt <= T && v > x) pos = nxt;
  }
  return pos;
}

// sum over the 16 lanes of a group, in every lane
__device__ __forceinline__ int group_sum(int v) {
#pragma unroll
  for (int sh = TR_G / 2; sh > 0; sh >>= 1) v += __shfl_xor(v, sh, TR_G);
  return v;
}

constexpr int TR_AHEAD = 16;  // keys of a run ranked side by side: the searches of a step are in flight together

// workgroup b: runs [16 b, min(16 b + 16, n_runs)) of `in` (run r at in + r stride, T keys, cnt_in[r] candidates behind it)
// -> run b of `out` (stride T) and cnt_out[b]; `last` (one workgroup): the outputs instead.
// Group r of the workgroup's sixteen 16-lane groups walks run r from its front, lane q counting the keys of run q above the
// key at hand; the ranks of a run's keys grow along the run, so the group stops at the first key ranked T or beyond (or at
// the run's first zero).  STAGED: the launcher found room for the workgroup's runs in LDS (16 T keys: T <= 512) and gave it
// that much dynamic LDS - the runs are copied there first and searched there; longer runs are searched in place.  (Two
// instantiations, so that each searches through pointers of ONE address space: a pointer that may be either makes every
// load a flat one, and those are waited for one by one.)
extern __shared__ __attribute__((aligned(16))) unsigned char merge_lds[];

template <bool STAGED>
__global__ void __launch_bounds__(TR_THREADS) k_trend_merge(const uint64_t* in, int64_t stride, const int32_t* cnt_in,
                                                            int64_t n_runs, uint64_t* out, int32_t* cnt_out, int last,
                                                            TrendOut o) {
  static_assert(TR_WAYS == TR_G && TR_WAYS == TR_GROUPS, "one group per run, one lane per other run");
  const int T = o.T, tid = threadIdx.x, sub = tid % TR_G, grp = tid / TR_G;
  const int64_t r0 = (int64_t)blockIdx.x * TR_WAYS;
  const int nr = (int)min((int64_t)TR_WAYS, n_runs - r0);
  uint64_t* dst = out + (int64_t)blockIdx.x * T;
  if (STAGED) {
    uint64_t* s_runs = reinterpret_cast<uint64_t*>(merge_lds);
    for (int e = tid; e < nr * T; e += TR_THREADS) {
      const int r = e / T;
      s_runs[e] = in[(r0 + r) * stride + (e - r * T)];
    }
    __syncthreads();
  }
  const uint64_t* runs = STAGED ? reinterpret_cast<const uint64_t*>(merge_lds) : in + r0 * stride;
  if (STAGED) stride = T;
  int P = 1;
  while (2 * P <= T) P <<= 1;
  const bool has = sub < nr;                               // lane `sub` looks into run `sub`
  const uint64_t* mine = runs + (has ? sub : 0) * stride;
  const int live = group_sum(has ? trend_above(mine, T, P, 0ull) : 0);   // non-zero keys in the runs
  const int total = group_sum(has ? cnt_in[r0 + sub] : 0);               // candidates behind the runs
  const int nv = live < T ? live : T;  // = min(T, total): a run holds min(T, its candidates) keys
  if (grp < nr) {  // (every condition below is uniform over the group)
    const uint64_t* own = runs + grp * stride;
    bool more = true;
    for (int p = 0; p < T && more; p += TR_AHEAD) {
      uint64_t x[TR_AHEAD];
      int above[TR_AHEAD];
#pragma unroll
      for (int u = 0; u < TR_AHEAD; ++u) x[u] = p + u < T ? own[p + u] : 0ull;
      // trend_above for the sixteen keys at once, step by step: a step's loads are issued together (a lane without a run
      // of its own searches run 0 and drops the result)
#pragma unroll
      for (int u = 0; u < TR_AHEAD; ++u) above[u] = 0;
      for (int step = P; step > 0; step >>= 1) {
        uint64_t v[TR_AHEAD];
#pragma unroll
        for (int u = 0; u < TR_AHEAD; ++u) {
          const int nxt = above[u] + step;
          v[u] = mine[(nxt <= T ? nxt : T) - 1];
        }
#pragma unroll
        for (int u = 0; u < TR_AHEAD; ++u) {
          const int nxt = above[u] + step;
          if (nxt <= T && v[u] > x[u]) above[u] = nxt;
        }
      }
      if (!has || sub == grp) {
#pragma unroll
        for (int u = 0; u < TR_AHEAD; ++u) above[u] = 0;
      }
#pragma unroll
      for (int u = 0; u < TR_AHEAD; ++u) {
        const int rank = p + u + group_sum(above[u]);  // the non-zero keys are distinct: a place nobody else takes
        more = more && x[u] != 0ull && rank < T;
        if (more && sub == 0) {
          if (last) trend_emit(o, rank, x[u]);
          else dst[rank] = x[u];
        }
      }
    }
  }
  for (int j = nv + tid; j < T; j += TR_THREADS) {  // (a key's rank is below the number of non-zero keys: below nv)
    if (last) trend_emit(o, j, 0ull);
    else dst[j] = 0ull;
  }
  if (tid == 0) {
    if (last) {
      *o.n_valid = nv;
      *o.n_distinct = total;
    } else {
      cnt_out[blockIdx.x] = total;
    }
  }
}

// workspace: keys uint64 [tiles 2048] | runs B uint64 [ceil(tiles / 16) T] | runs C uint64 [ceil(tiles / 256) T] |
//            counts int32 [tiles] | [ceil(tiles / 16)] | [ceil(tiles / 256)]     (a call of one tile: the keys alone)
struct TrendPlan {
  int64_t n, tiles, nb, nc;
  size_t off_b, off_c, off_cnt, bytes;
};
static TrendPlan trend_plan(int64_t n, int T) {
  TrendPlan p{};
  p.n = n;
  p.tiles = std::max<int64_t>(1, cdiv(n, TR_TILE));
  p.off_b = (size_t)p.tiles * TR_TILE * sizeof(uint64_t);
  if (p.tiles == 1) {
    p.bytes = p.off_b;
    return p;
  }
  p.nb = cdiv(p.tiles, TR_WAYS);
  p.nc = cdiv(p.nb, TR_WAYS);
  p.off_c = p.off_b + (size_t)p.nb * T * sizeof(uint64_t);
  p.off_cnt = p.off_c + (size_t)p.nc * T * sizeof(uint64_t);
  p.bytes = (p.off_cnt + (size_t)(p.tiles + p.nb + p.nc) * sizeof(int32_t) + 15) & ~(size_t)15;
  return p;
}

// the refusals of tiger_hip.h, device entry and host twin alike -> the number of eligible slots in *n
static int trend_args(const tg_tcsr* g, double t_lo, double t_hi, const int64_t* among, int64_t M, int32_t T, const int64_t* ids,
                      const int32_t* counts, const int32_t* n_valid, const int32_t* n_distinct, int64_t* n) {
  if (!g || g->num_node <= 0 || g->num_entry < 0 || M < 0) return TG_EINVAL;
  if (T < 1 || T > TG_TREND_MAX) return TG_EINVAL;
  if (std::isnan(t_lo) || std::isnan(t_hi) || t_lo > t_hi) return TG_EINVAL;
  if (!ids || !counts || !n_valid || !n_distinct) return TG_EINVAL;
  if (!g->indptr || (g->num_entry > 0 && (!g->ts || !g->nbr))) return TG_EINVAL;
  *n = among ? M : g->num_node;
  if (cdiv(*n, TR_TILE) > 0x7fffffffLL) return TG_EINVAL;  // one workgroup per tile
  return TG_OK;
}

// ---- fill ------------------------------------------------------------------------------------------------------------------
constexpr int FL_EMPTY = -1;
constexpr int FL_CTL_BYTES = 16;  // the scan's wave sums

// LDS of one workgroup, dynamic: ctl | table ids int32 [S] | table positions int32 [S] | never uint8 [T16] | flags uint8 [T16]
struct FillPlan {
  int T, S, log2S, T16;
  size_t lds;
};
static bool fill_plan(int32_t T, FillPlan* p) {
  if (T < 1 || T > TG_TREND_MAX) return false;
  p->T = T;
  p->S = 64;
  while (p->S < 2 * T) p->S <<= 1;
  p->log2S = 0;
  while ((1 << p->log2S) < p->S) ++p->log2S;
  p->T16 = (T + 15) & ~15;
  p->lds = FL_CTL_BYTES + 2 * (size_t)p->S * sizeof(int32_t) + 2 * (size_t)p->T16;
  return true;
}

struct FillArgs {
  tg_tcsr g;
  int64_t B;
  const int64_t* src;
  const double* ts;
  int C, flags;
  int64_t* ids;
  int32_t* counts;
  int32_t* n_valid;
  const int64_t* fill_ids;
  const int32_t* n_fill;
  FillPlan p;
  int32_t* n_filled;
};

__device__ __forceinline__ uint32_t fill_hash(int id, int log2S) { return ((uint32_t)id * 2654435761u) >> (32 - log2S); }

// the first position of `id` in the fill list, -1 when the list does not hold it (ids outside [1, 2^31) are never in it)
__device__ __forceinline__ int fill_find(const int* t_id, const int* t_pos, int log2S, int64_t id) {
  if (id < 1 || id > 0x7fffffffLL) return -1;
  const uint32_t mask = (1u << log2S) - 1u;
  uint32_t h = fill_hash((int)id, log2S);
  for (;;) {
    const int cur = t_id[h];
    if (cur == FL_EMPTY) return -1;
    if (cur == (int)id) return t_pos[h];
    h = (h + 1) & mask;
  }
}

extern __shared__ __attribute__((aligned(16))) unsigned char fill_lds[];

__global__ void __launch_bounds__(TR_THREADS) k_fill_candidates(FillArgs a) {
  const tg_tcsr& g = a.g;
  const FillPlan& pl = a.p;
  uint32_t* s_wave = reinterpret_cast<uint32_t*>(fill_lds);
  int* t_id = reinterpret_cast<int*>(fill_lds + FL_CTL_BYTES);
  int* t_pos = t_id + pl.S;
  uint8_t* never = reinterpret_cast<uint8_t*>(t_pos + pl.S);
  uint8_t* flag = never + pl.T16;
  const int tid = threadIdx.x, sub = tid % TR_G;
  const int T = pl.T, S = pl.S, log2S = pl.log2S, C = a.C;
  const bool exclude_seen = a.flags & 1, keep_self = a.flags & 2;
  const int nf_raw = *a.n_fill;
  const int nf = nf_raw < 0 ? 0 : (nf_raw < T ? nf_raw : T);
  bool built = false;

  for (int64_t q = blockIdx.x; q < a.B; q += gridDim.x) {  // (every condition on q, nv, built is workgroup-uniform)
    const int nv_raw = a.n_valid[q];
    const int nv = nv_raw < 0 ? 0 : nv_raw;
    if (nv >= C) {  // a full row: nothing is touched but its count of appended ids
      if (tid == 0) a.n_filled[q] = 0;
      continue;
    }
    if (!built) {  // once per workgroup: id -> first position, and what no query takes
      for (int i = tid; i < S; i += TR_THREADS) {
        t_id[i] = FL_EMPTY;
        t_pos[i] = 0x7fffffff;
      }
      __syncthreads();
      const uint32_t mask = (1u << log2S) - 1u;
      for (int p = tid; p < nf; p += TR_THREADS) {
        const int64_t id = a.fill_ids[p];
        if (id < 1 || id > 0x7fffffffLL) continue;
        uint32_t h = fill_hash((int)id, log2S);
        for (;;) {  // at most T <= S / 2 distinct ids: an empty slot always ends the chain
          const int old = atomicCAS(&t_id[h], FL_EMPTY, (int)id);
          if (old == FL_EMPTY || old == (int)id) {
            atomicMin(&t_pos[h], p);
            break;
          }
          h = (h + 1) & mask;
        }
      }
      __syncthreads();
      for (int p = tid; p < T; p += TR_THREADS) never[p] = p >= nf || fill_find(t_id, t_pos, log2S, a.fill_ids[p]) != p;
      built = true;
      __syncthreads();
    }
    const int64_t src = a.src[q];
    const double t = a.ts[q];
    for (int p = tid; p < T; p += TR_THREADS) flag[p] = never[p];
    __syncthreads();
    // (lanes that flag the same position store the same byte)
    for (int j = tid; j < nv; j += TR_THREADS) {
      const int p = fill_find(t_id, t_pos, log2S, a.ids[q * C + j]);
      if (p >= 0) flag[p] = 1;
    }
    if (tid == 0 && !keep_self) {
      const int p = fill_find(t_id, t_pos, log2S, src);
      if (p >= 0) flag[p] = 1;
    }
    if (exclude_seen) {  // the source's whole prefix, 256 entries per pass (every group runs the same search)
      int64_t start;
      const int64_t end = prefix_end_group<TR_G>(g, src, t, &start, sub);
      for (int64_t e = start + tid; e < end; e += TR_THREADS) {
        const int p = fill_find(t_id, t_pos, log2S, (int64_t)g.nbr[e]);
        if (p >= 0) flag[p] = 1;
      }
    }
    __syncthreads();
    // ordered compaction: the first `need` unflagged positions, in position order, behind the row
    const int need = C - nv;
    int written = 0;
    for (int p0 = 0; p0 < nf && written < need; p0 += TR_THREADS) {
      const int p = p0 + tid;
      const uint32_t take = p < nf && !flag[p];
      uint32_t total;
      const int at = written + (int)block_excl_scan(take, s_wave, &total);
      if (take && at < need) {
        a.ids[q * C + nv + at] = a.fill_ids[p];
        a.counts[q * C + nv + at] = 0;
      }
      written += (int)total;
    }
    if (tid == 0) {
      const int nw = written < need ? written : need;
      a.n_filled[q] = nw;
      a.n_valid[q] = nv + nw;
    }
    __syncthreads();  // the next query rewrites the flags
  }
}

static int fill_args(const tg_tcsr* g, int64_t B, const int64_t* src, const double* ts, int32_t C, const int64_t* ids,
                     const int32_t* counts, const int32_t* n_valid, const int64_t* fill_ids, const int32_t* n_fill, int32_t T,
                     int32_t flags, const int32_t* n_filled, FillPlan* p) {
  if (!g || g->num_node <= 0 || g->num_entry < 0 || B < 0) return TG_EINVAL;
  if (C < 1 || C > TG_WALK_MAX_ENDPOINTS || flags < 0 || flags > 3) return TG_EINVAL;
  if (!fill_plan(T, p)) return TG_EINVAL;
  if (B == 0) return TG_OK;  // nothing is read or written
  if (!src || !ts || !ids || !counts || !n_valid || !fill_ids || !n_fill || !n_filled) return TG_EINVAL;
  if (!g->indptr || (g->num_entry > 0 && (!g->ts || !g->nbr))) return TG_EINVAL;
  return TG_OK;
}

}  // namespace tg

using namespace tg;

extern "C" size_t tg_trending_workspace_bytes(int64_t n, int32_t T) {
  if (n < 0 || T < 1 || T > TG_TREND_MAX) return 0;
  return trend_plan(n, T).bytes;
}

extern "C" int tg_trending(const tg_tcsr* g, double t_lo, double t_hi, const int64_t* among, int64_t M, int32_t T, int64_t* ids,
                           int32_t* counts, int32_t* n_valid, int32_t* n_distinct, void* ws, size_t ws_bytes, void* stream) {
  int64_t n = 0;
  if (int rc = trend_args(g, t_lo, t_hi, among, M, T, ids, counts, n_valid, n_distinct, &n)) return rc;
  const TrendPlan p = trend_plan(n, T);
  if (int rc = ws_check(ws, ws_bytes, p.bytes)) return rc;
  hipStream_t st = as_stream(stream);
  unsigned char* base = static_cast<unsigned char*>(ws);
  uint64_t* keys = reinterpret_cast<uint64_t*>(base);
  const int64_t n_pad = p.tiles * TR_TILE;
  const TrendOut o{T, ids, counts, n_valid, n_distinct};
  hipLaunchKernelGGL(k_window_keys, dim3(flat_grid(n_pad, TR_GROUPS)), dim3(TR_THREADS), 0, st, *g, t_lo, t_hi, among, n, n_pad,
                     keys);
  if (p.tiles == 1) {
    hipLaunchKernelGGL(k_trend_tiles, dim3(1), dim3(TR_THREADS), 0, st, keys, (int32_t*)nullptr, 1, o);
    return check_launch("tg_trending");
  }
  uint64_t* run_b = reinterpret_cast<uint64_t*>(base + p.off_b);
  uint64_t* run_c = reinterpret_cast<uint64_t*>(base + p.off_c);
  int32_t* cnt_a = reinterpret_cast<int32_t*>(base + p.off_cnt);
  int32_t* cnt_b = cnt_a + p.tiles;
  int32_t* cnt_c = cnt_b + p.nb;
  hipLaunchKernelGGL(k_trend_tiles, dim3((unsigned)p.tiles), dim3(TR_THREADS), 0, st, keys, cnt_a, 0, o);
  // rounds: tiles (stride 2 048) -> B -> C -> B -> ... ; a round's input is free again once the next one has read its output
  const uint64_t* in = keys;
  const int32_t* cnt_in = cnt_a;
  int64_t stride = TR_TILE, n_runs = p.tiles;
  for (int round = 0; n_runs > 1; ++round) {
    const int64_t n_out = cdiv(n_runs, TR_WAYS);
    uint64_t* out = (round & 1) ? run_c : run_b;
    int32_t* cnt_out = (round & 1) ? cnt_c : cnt_b;
    const size_t stage = (size_t)std::min<int64_t>(TR_WAYS, n_runs) * T * sizeof(uint64_t);
    const int staged = stage <= TR_STAGE_MAX;
    if (staged)
      hipLaunchKernelGGL(k_trend_merge<true>, dim3((unsigned)n_out), dim3(TR_THREADS), stage, st, in, stride, cnt_in, n_runs,
                         out, cnt_out, n_out == 1 ? 1 : 0, o);
    else
      hipLaunchKernelGGL(k_trend_merge<false>, dim3((unsigned)n_out), dim3(TR_THREADS), 0, st, in, stride, cnt_in, n_runs, out,
                         cnt_out, n_out == 1 ? 1 : 0, o);
    in = out;
    cnt_in = cnt_out;
    stride = T;
    n_runs = n_out;
  }
  return check_launch("tg_trending");
}

extern "C" int tg_trending_host(const tg_tcsr* g, double t_lo, double t_hi, const int64_t* among_host, int64_t M, int32_t T,
                                int64_t* ids_host, int32_t* counts_host, int32_t* n_valid_host, int32_t* n_distinct_host) {
  int64_t n = 0;
  if (int rc = trend_args(g, t_lo, t_hi, among_host, M, T, ids_host, counts_host, n_valid_host, n_distinct_host, &n)) return rc;
  std::vector<uint64_t> keys;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t v = among_host ? among_host[i] : i;
    if (v < 1 || v >= g->num_node) continue;
    const double *b = g->ts + g->indptr[v], *e = g->ts + g->indptr[v + 1];
    const int64_t c = std::lower_bound(b, e, t_hi) - std::lower_bound(b, e, t_lo);  // t_lo <= ts < t_hi
    if (c > 0) keys.push_back(trend_key(c, v));
  }
  std::sort(keys.begin(), keys.end(), [](uint64_t x, uint64_t y) { return x > y; });
  const int64_t nd = (int64_t)keys.size(), nv = std::min<int64_t>(nd, T);
  for (int32_t j = 0; j < T; ++j) {
    ids_host[j] = j < nv ? (int64_t)(0xFFFFFFFFu - (uint32_t)keys[j]) : 0;
    counts_host[j] = j < nv ? (int32_t)(keys[j] >> 32) : 0;
  }
  *n_valid_host = (int32_t)nv;
  *n_distinct_host = (int32_t)nd;
  return TG_OK;
}

extern "C" size_t tg_fill_candidates_lds_bytes(int32_t T) {
  FillPlan p{};
  return fill_plan(T, &p) ? p.lds : 0;
}

extern "C" int tg_fill_candidates(const tg_tcsr* g, int64_t B, const int64_t* src, const double* ts, int32_t C, int64_t* ids,
                                  int32_t* counts, int32_t* n_valid, const int64_t* fill_ids, const int32_t* n_fill, int32_t T,
                                  int32_t flags, int32_t* n_filled, void* stream) {
  FillPlan p{};
  if (int rc = fill_args(g, B, src, ts, C, ids, counts, n_valid, fill_ids, n_fill, T, flags, n_filled, &p)) return rc;
  if (B == 0) return TG_OK;
  FillArgs a{*g, B, src, ts, C, flags, ids, counts, n_valid, fill_ids, n_fill, p, n_filled};
  hipLaunchKernelGGL(k_fill_candidates, dim3(flat_grid(B, 1)), dim3(TR_THREADS), p.lds, as_stream(stream), a);
  return check_launch("tg_fill_candidates");
}

extern "C" int tg_fill_candidates_host(const tg_tcsr* g, int64_t B, const int64_t* src_host, const double* ts_host, int32_t C,
                                       int64_t* ids_host, int32_t* counts_host, int32_t* n_valid_host,
                                       const int64_t* fill_ids_host, const int32_t* n_fill_host, int32_t T, int32_t flags,
                                       int32_t* n_filled_host) {
  FillPlan p{};
  if (int rc = fill_args(g, B, src_host, ts_host, C, ids_host, counts_host, n_valid_host, fill_ids_host, n_fill_host, T, flags,
                         n_filled_host, &p))
    return rc;
  if (B == 0) return TG_OK;
  const int nf = std::min<int32_t>(std::max<int32_t>(*n_fill_host, 0), T);
  std::unordered_set<int64_t> out;  // what the query does not take again: its row, its source, what it has seen
  for (int64_t q = 0; q < B; ++q) {
    const int nv = std::max<int32_t>(n_valid_host[q], 0);
    n_filled_host[q] = 0;
    if (nv >= C) continue;
    const int64_t s = src_host[q];
    out.clear();
    for (int j = 0; j < nv; ++j) out.insert(ids_host[q * C + j]);
    if (!(flags & 2)) out.insert(s);
    if ((flags & 1) && s >= 0 && s < g->num_node) {
      const int64_t lo = g->indptr[s];
      const int64_t hi = std::lower_bound(g->ts + lo, g->ts + g->indptr[s + 1], ts_host[q]) - g->ts;  // ts < t
      for (int64_t e = lo; e < hi; ++e) out.insert((int64_t)g->nbr[e]);
    }
    int at = nv;
    for (int pos = 0; pos < nf && at < C; ++pos) {
      const int64_t id = fill_ids_host[pos];
      if (id < 1 || id > 0x7fffffffLL || !out.insert(id).second) continue;  // (taken ids join the set: nothing twice)
      ids_host[q * C + at] = id;
      counts_host[q * C + at] = 0;
      ++at;
    }
    n_filled_host[q] = at - nv;
    n_valid_host[q] = at;
  }
  return TG_OK;
}
