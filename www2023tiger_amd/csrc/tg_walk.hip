// Walk candidates: per-query candidate generation over the T-CSR (tiger_hip.h: tg_walk_candidates; no counterpart in the
// reference, which ranks whatever candidates its caller brings).
//
//   last(v, t, F) = the neighbour ids of the last F entries of node v with time < t (prefix_end, the recent-edges rule:
//                   strict float64 '<', duplicates kept); nothing for a node outside [0, num_node) or without entries
//   N1 = last(src, t, F1),  N(l+1) = the concatenation of last(v, t, F(l+1)) over the elements v of N(l), with multiplicity:
//   every hop is cut at the ROOT's time t.  w(v) = the multiplicity of v in the levels whose `take` bit is set = the number
//   of walks that end in v.  Candidates: w > 0 without node 0, without src (unless keep_self) and - exclude_seen - without
//   every node of src's WHOLE prefix before t.  Order (total): higher w first, equal w by ascending id; the first C.
//
// One 256-thread workgroup per query, capped grid.  Per level the searches of the frontier (1, <= F1, <= F1 F2 of them) run
// side by side, sixteen at a time: one 16-lane group per search (prefix_end_group<16>), the tail of the prefix read by the
// group's lanes.  A level that is walked further parks its ids in LDS (the expanded frontier, compacted: a group reserves
// its run with one LDS atomic); a taken level counts its ids into an open-addressing table in LDS, (int32 id, int32 weight)
// with linear probing, a power-of-two number of slots >= 2 x the endpoint bound of the call's fan-out (the table is never
// more than half full, so every probe chain ends at an empty slot).  exclude_seen: the workgroup sweeps [start, end) of the
// source, 256 entries per pass, and zeroes the weight of every neighbour it finds in the table.  Selection: the live slots
// are compacted to 64-bit keys (w << 32) | (0xFFFFFFFF - id), padded with zeros to a power of two, sorted descending by a
// bitonic network in LDS, and the first C are written.
// The result does not depend on the order of the insertions: the weights are integer sums (LDS integer atomics commute),
// the frontier is a multiset whose order only decides which group searches which element, and the final order is total on
// (w, id) - so where a key lands in the table or in the compacted list is invisible.  No global atomics, no workspace.
// Integer work and comparisons only: device, host twin and a numpy / dict reference agree bit for bit.
#include <algorithm>
#include <unordered_map>
#include <vector>

#include "tg_sample.h"

namespace tg {

constexpr int WK_THREADS = 256;
constexpr int WK_G = 16;                      // lanes per search
constexpr int WK_GROUPS = WK_THREADS / WK_G;  // searches side by side
constexpr int WK_EMPTY = -1;                  // table slot without an id
constexpr int WK_CTL_BYTES = 32;              // ctl[0], ctl[1]: sizes of the two parked frontiers; ctl[2]: live slots; +16: start, end

// LDS of one workgroup, everything dynamic (16-byte aligned carve offsets):
//   ctl | keys uint64 [KP] | table ids int32 [T] | table weights int32 [T] | frontier 1 int32 [F1] | frontier 2 int32 [F1 F2]
struct WalkPlan {
  int L, take, F[3];
  int endpoints;  // sum of the sizes of the taken levels: the bound on distinct ids
  int T, log2T;   // table slots
  int KP;         // sort keys: power of two >= endpoints
  int cap1, cap2; // parked frontiers (0: the level is the last one)
  size_t lds;
};

static inline int walk_pow2_at_least(int x) {
  int p = 1;
  while (p < x) p <<= 1;
  return p;
}

// the refusals of tiger_hip.h that do not depend on pointers; fills the plan
static int walk_plan(int32_t n_levels, const int32_t* fanout, int32_t take, int32_t C, int32_t flags, WalkPlan* p) {
  if (n_levels < 1 || n_levels > 3 || !fanout) return TG_EINVAL;
  if (take <= 0 || (take >> n_levels) != 0 || !((take >> (n_levels - 1)) & 1)) return TG_EINVAL;
  if (flags < 0 || flags > 3) return TG_EINVAL;
  int64_t size = 1, endpoints = 0;
  for (int l = 0; l < n_levels; ++l) {
    if (fanout[l] < 1 || fanout[l] > TG_WALK_MAX_FANOUT) return TG_EINVAL;
    size *= fanout[l];
    if (l < 2 && size > TG_WALK_MAX_FRONTIER) return TG_EINVAL;  // F1 and F1 F2: the expanded frontiers
    if ((take >> l) & 1) endpoints += size;
    p->F[l] = fanout[l];
  }
  if (endpoints > TG_WALK_MAX_ENDPOINTS) return TG_EINVAL;
  if (C < 1 || C > TG_WALK_MAX_ENDPOINTS) return TG_EINVAL;
  p->L = n_levels;
  p->take = take;
  p->endpoints = (int)endpoints;
  p->T = std::max(64, walk_pow2_at_least(2 * (int)endpoints));
  p->log2T = 0;
  while ((1 << p->log2T) < p->T) ++p->log2T;
  p->KP = std::max(2, walk_pow2_at_least((int)endpoints));
  p->cap1 = n_levels >= 2 ? fanout[0] : 0;
  p->cap2 = n_levels >= 3 ? fanout[0] * fanout[1] : 0;
  const size_t fr = ((size_t)(p->cap1 + p->cap2) * sizeof(int32_t) + 15) & ~(size_t)15;
  p->lds = WK_CTL_BYTES + (size_t)p->KP * sizeof(uint64_t) + 2 * (size_t)p->T * sizeof(int32_t) + fr;
  return TG_OK;
}

struct WalkArgs {
  tg_tcsr g;
  int64_t B;
  const int64_t* src;
  const double* ts;
  WalkPlan p;
  int C, flags;
  int64_t* ids;
  int32_t* counts;
  int32_t* n_valid;
  int32_t* n_distinct;
};

__device__ __forceinline__ uint32_t walk_hash(int id, int log2T) { return ((uint32_t)id * 2654435761u) >> (32 - log2T); }

// w(id) += 1.  The table holds at most `endpoints` <= T / 2 distinct ids: an empty slot always ends the chain.
__device__ __forceinline__ void walk_insert(int* t_id, int* t_w, int log2T, int id) {
  const uint32_t mask = (1u << log2T) - 1u;
  uint32_t h = walk_hash(id, log2T);
  for (;;) {
    const int old = atomicCAS(&t_id[h], WK_EMPTY, id);
    if (old == WK_EMPTY || old == id) {
      atomicAdd(&t_w[h], 1);
      return;
    }
    h = (h + 1) & mask;
  }
}

// w(id) = 0 where the table holds id (lanes that kill the same slot store the same value)
__device__ __forceinline__ void walk_kill(const int* t_id, int* t_w, int log2T, int id) {
  const uint32_t mask = (1u << log2T) - 1u;
  uint32_t h = walk_hash(id, log2T);
  for (;;) {
    const int cur = t_id[h];
    if (cur == WK_EMPTY) return;
    if (cur == id) {
      t_w[h] = 0;
      return;
    }
    h = (h + 1) & mask;
  }
}

extern __shared__ __attribute__((aligned(16))) unsigned char walk_lds[];

__global__ void __launch_bounds__(WK_THREADS) k_walk_candidates(WalkArgs a) {
  const tg_tcsr& g = a.g;
  const WalkPlan& pl = a.p;
  int* ctl = reinterpret_cast<int*>(walk_lds);
  int64_t* s_range = reinterpret_cast<int64_t*>(walk_lds + 16);  // the source's prefix [start, end)
  uint64_t* keys = reinterpret_cast<uint64_t*>(walk_lds + WK_CTL_BYTES);
  int* t_id = reinterpret_cast<int*>(keys + pl.KP);
  int* t_w = t_id + pl.T;
  int* fr1 = t_w + pl.T;
  int* fr2 = fr1 + pl.cap1;
  const int tid = threadIdx.x, lane = lane_id(), sub = tid % WK_G, grp = tid / WK_G;
  const int T = pl.T, log2T = pl.log2T, L = pl.L, C = a.C;
  const bool exclude_seen = a.flags & 1, keep_self = a.flags & 2;

  for (int64_t q = blockIdx.x; q < a.B; q += gridDim.x) {
    const int64_t src = a.src[q];
    const double t = a.ts[q];
    for (int i = tid; i < T; i += WK_THREADS) {
      t_id[i] = WK_EMPTY;
      t_w[i] = 0;
    }
    if (tid < 4) ctl[tid] = 0;
    __syncthreads();

    // ---- the walk: level l searches the n_in elements of the frontier in front of it, sixteen at a time ----
    int n_in = 1;
    const int* fin = nullptr;
    for (int l = 0; l < L; ++l) {  // (every condition on l, n_in and s0 is workgroup-uniform)
      const int F = pl.F[l];
      const bool last = l == L - 1, taken = (pl.take >> l) & 1;
      int* fout = l == 0 ? fr1 : fr2;
      for (int s0 = 0; s0 < n_in; s0 += WK_GROUPS) {
        const int s = s0 + grp;
        const int64_t nid = s < n_in ? (l == 0 ? src : (int64_t)fin[s]) : -1;  // a group without a search: no entries
        int64_t start;
        const int64_t end = prefix_end_group<WK_G>(g, nid, t, &start, sub);
        if (l == 0 && tid == 0) {
          s_range[0] = start;
          s_range[1] = end;
        }
        const int c = (int)min((int64_t)F, end - start);
        int base = 0;
        if (!last) {  // the group's run in the next frontier: at most F per search, so the level's total fits its capacity
          if (sub == 0 && c > 0) base = atomicAdd(&ctl[l], c);
          base = __shfl(base, lane & ~(WK_G - 1), TG_WAVE);
        }
        for (int i = sub; i < c; i += WK_G) {
          const int nb = g.nbr[end - c + i];
          if (!last) fout[base + i] = nb;
          if (taken && nb >= 0 && nb < g.num_node) walk_insert(t_id, t_w, log2T, nb);
        }
      }
      __syncthreads();
      if (!last) {
        n_in = ctl[l];
        fin = fout;
      }
    }

    // ---- exclude_seen: the source's whole prefix, 256 entries per pass ----
    if (exclude_seen) {
      const int64_t start = s_range[0], end = s_range[1];
      for (int64_t p = start + tid; p < end; p += WK_THREADS) {
        const int nb = g.nbr[p];
        if (nb >= 0 && nb < g.num_node) walk_kill(t_id, t_w, log2T, nb);
      }
      __syncthreads();
    }

    // ---- selection: live slots -> keys, bitonic sort (descending), the first C ----
    for (int i = tid; i < T; i += WK_THREADS) {
      const int id = t_id[i], w = t_w[i];
      if (id != WK_EMPTY && w > 0 && id != 0 && (keep_self || (int64_t)id != src)) {
        const int pos = atomicAdd(&ctl[2], 1);  // (at most `endpoints` <= KP live slots)
        keys[pos] = ((uint64_t)(uint32_t)w << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)id);
      }
    }
    __syncthreads();
    const int n = ctl[2];
    int P = 2;
    while (P < n) P <<= 1;  // <= KP
    for (int i = n + tid; i < P; i += WK_THREADS) keys[i] = 0ull;  // below every live key (w > 0)
    __syncthreads();
    if (n > 1) {
      for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int i = tid; i < P; i += WK_THREADS) {
            const int x = i ^ j;
            if (x > i) {
              const uint64_t ki = keys[i], kx = keys[x];
              const bool desc = (i & k) == 0;
              if (desc ? ki < kx : ki > kx) {
                keys[i] = kx;
                keys[x] = ki;
              }
            }
          }
          __syncthreads();
        }
      }
    }
    const int nv = n < C ? n : C;
    for (int j = tid; j < C; j += WK_THREADS) {
      const uint64_t key = j < nv ? keys[j] : 0ull;
      a.ids[q * C + j] = j < nv ? (int64_t)(0xFFFFFFFFu - (uint32_t)key) : (int64_t)0;
      a.counts[q * C + j] = (int32_t)(key >> 32);
    }
    if (tid == 0) {
      a.n_valid[q] = nv;
      a.n_distinct[q] = n;
    }
    __syncthreads();  // the next query re-initialises the table and the counters
  }
}

static int walk_args(const tg_tcsr* g, int64_t B, const int64_t* src, const double* ts, int32_t n_levels,
                     const int32_t* fanout, int32_t take, int32_t C, int32_t flags, const int64_t* ids, const int32_t* counts,
                     const int32_t* n_valid, const int32_t* n_distinct, WalkPlan* p) {
  if (!g || g->num_node <= 0 || g->num_entry < 0 || B < 0) return TG_EINVAL;
  if (int rc = walk_plan(n_levels, fanout, take, C, flags, p)) return rc;
  if (B == 0) return TG_OK;  // nothing is read or written
  if (!src || !ts || !ids || !counts || !n_valid || !n_distinct) return TG_EINVAL;
  if (!g->indptr || (g->num_entry > 0 && (!g->ts || !g->nbr))) return TG_EINVAL;
  return TG_OK;
}

// last(v, t, F) on the host arrays -> appended to `out`
static void walk_host_last(const tg_tcsr* g, int64_t v, double t, int F, std::vector<int32_t>& out) {
  if (v < 0 || v >= g->num_node) return;
  const int64_t lo = g->indptr[v];
  const int64_t hi = std::lower_bound(g->ts + lo, g->ts + g->indptr[v + 1], t) - g->ts;  // ts < t
  for (int64_t p = std::max(lo, hi - F); p < hi; ++p) out.push_back(g->nbr[p]);
}

}  // namespace tg

using namespace tg;

extern "C" size_t tg_walk_candidates_lds_bytes(int32_t n_levels, const int32_t* fanout, int32_t take) {
  WalkPlan p{};
  if (walk_plan(n_levels, fanout, take, 1, 0, &p)) return 0;
  return p.lds;
}

extern "C" int tg_walk_candidates(const tg_tcsr* g, int64_t B, const int64_t* src, const double* ts, int32_t n_levels,
                                  const int32_t* fanout, int32_t take, int32_t C, int32_t flags, int64_t* ids,
                                  int32_t* counts, int32_t* n_valid, int32_t* n_distinct, void* stream) {
  WalkPlan p{};
  if (int rc = walk_args(g, B, src, ts, n_levels, fanout, take, C, flags, ids, counts, n_valid, n_distinct, &p)) return rc;
  if (B == 0) return TG_OK;
  WalkArgs a{*g, B, src, ts, p, C, flags, ids, counts, n_valid, n_distinct};
  hipLaunchKernelGGL(k_walk_candidates, dim3(flat_grid(B, 1)), dim3(WK_THREADS), p.lds, as_stream(stream), a);
  return check_launch("tg_walk_candidates");
}

extern "C" int tg_walk_candidates_host(const tg_tcsr* g, int64_t B, const int64_t* src_host, const double* ts_host,
                                       int32_t n_levels, const int32_t* fanout, int32_t take, int32_t C, int32_t flags,
                                       int64_t* ids_host, int32_t* counts_host, int32_t* n_valid_host,
                                       int32_t* n_distinct_host) {
  WalkPlan p{};
  if (int rc = walk_args(g, B, src_host, ts_host, n_levels, fanout, take, C, flags, ids_host, counts_host, n_valid_host,
                         n_distinct_host, &p))
    return rc;
  std::vector<int32_t> cur, next;
  std::unordered_map<int32_t, int32_t> w;
  std::vector<uint64_t> keys;
  for (int64_t q = 0; q < B; ++q) {
    const int64_t s = src_host[q];
    const double t = ts_host[q];
    w.clear();
    cur.clear();
    walk_host_last(g, s, t, p.F[0], cur);
    for (int l = 0;; ++l) {
      if ((take >> l) & 1)
        for (int32_t v : cur)
          if (v >= 0 && v < g->num_node) ++w[v];
      if (l == n_levels - 1) break;
      next.clear();
      for (int32_t v : cur) walk_host_last(g, v, t, p.F[l + 1], next);
      cur.swap(next);
    }
    w.erase(0);
    if (!(flags & 2) && s >= 0 && s <= 0x7fffffffLL) w.erase((int32_t)s);
    if ((flags & 1) && s >= 0 && s < g->num_node) {
      const int64_t lo = g->indptr[s];
      const int64_t hi = std::lower_bound(g->ts + lo, g->ts + g->indptr[s + 1], t) - g->ts;
      for (int64_t e = lo; e < hi; ++e) w.erase(g->nbr[e]);
    }
    keys.clear();
    for (const auto& kv : w) keys.push_back(((uint64_t)(uint32_t)kv.second << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)kv.first));
    std::sort(keys.begin(), keys.end(), [](uint64_t x, uint64_t y) { return x > y; });
    const int32_t n = (int32_t)keys.size(), nv = std::min<int32_t>(n, C);
    for (int32_t j = 0; j < C; ++j) {
      ids_host[q * C + j] = j < nv ? (int64_t)(0xFFFFFFFFu - (uint32_t)keys[j]) : 0;
      counts_host[q * C + j] = j < nv ? (int32_t)(keys[j] >> 32) : 0;
    }
    n_valid_host[q] = nv;
    n_distinct_host[q] = n;
  }
  return TG_OK;
}
