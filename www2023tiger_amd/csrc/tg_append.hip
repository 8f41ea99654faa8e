// T-CSR extension by a time-ordered batch of new events (online ingestion; reference tiger/data/graph.py:11-42,226-241:
// the reference builds its adjacency lists over the whole stream in advance and has no counterpart of this).
//
// Contract (the caller checks, as for tg_tcsr_build_device): the batch is non-decreasing in time and starts no earlier
// than the latest entry of the old graph.  Then the stable per-node sort by time of the reference is the identity on
// [old events | new events], and the T-CSR over the concatenation is, row by row, the old row followed by the node's new
// entries in event order (entry j = 2e seen from src before j = 2e + 1 seen from dst).  So, with m = 2 n new entries:
//   1. sort the m entries stably by owner                         -> S[s] (owner), J[s] (entry), s = 0 .. m-1
//   2. INS[s] = indptr_old[S[s] + 1]: where the old array is cut  -> non-decreasing in s
//   3. indptr_out[v] = indptr_old[v] + lower_bound(S, v)
//   4. old entry p moves to p + upper_bound(INS, p)
//   5. new entry s lands at INS[s] + s
// No owner lookup for old entries, no atomics, no scan or memset over num_node.  Steps 3-5 are ONE launch (block roles);
// steps 1-2 are one launch while m <= AP_SMALL (one workgroup sorts the unique keys owner << 12 | j in LDS - unique keys:
// any sort is stable), else key formation + radix_sort_pairs (tg_build.hip) + one launch for INS.
// Cost: every old entry is read and written once (16 + 16 bytes) - the price of keeping the compact layout every sampler reads.
//
// Growth (tg_tcsr_append_grow: num_node_out >= num_node): ids in [num_node, num_node_out) own no old entry, so their old row
// is the empty row at the end of the old array - every read of indptr_old is clamped to index num_node (steps 2 and 3),
// step 3 runs over num_node_out + 1 entries and the large path sorts on the key bits of num_node_out.  Same launches, no
// pass over num_node_out beside step 3 itself; with num_node_out == num_node the clamps never bind and the grid is the old one.
//
// Late events (tg_tcsr_merge: a batch in ANY order with ANY non-NaN times; the reference has no counterpart either).  Row v of
// the output is the stable merge of the old row v with v's new entries sorted stably by time: at equal times old entries
// first, new ones in ascending j - what the stable per-node sort of tg_tcsr_build_host gives over [old events | batch].  Only
// steps 1-2 differ:
//   1'. sort the m entries by (owner, time key, j); the time key is the float64 as an orderable uint64 (sign bit flipped for
//       t >= 0, all bits for t < 0) with -0.0 read as +0.0 IN THE KEY ONLY: the two are == to the host comparator, and the
//       stored time keeps its bits.  m <= MG_SMALL: one workgroup, 128-bit unique keys in LDS; else three stable radix sorts
//       (time key low word, high word, owner) through radix_sort_pairs, the keys re-derived from the payload j in between.
//   2'. INS[s] = first p of row S[s] with ts_old[p] > t(s) (strict, on values): an upper bound galloped for from the row's
//       end, where a late event usually belongs.  Non-decreasing in s: within a row by t, across rows by the rows' order.
// Steps 3-5 are k_append_apply as it stands (old entry p -> p + #{INS <= p}: it stays behind every new entry cut in at or
// before it and before every later one).  Nothing loaded from the batch is used as an address; indptr is the parent's.
#include <algorithm>
#include <vector>

#include "tg_step.h"
#include "tg_tcsr.h"

namespace tg {

constexpr int AP_SMALL = 4096;             // new entries (2 n) the one-workgroup sort takes
constexpr int MG_SMALL = 4096;             // the same for a merge: 16 bytes of key per entry, 64 KiB of LDS - the static limit
constexpr int AP_SORT_THREADS = 1024;
constexpr int AP_THREADS = 256;
constexpr int AP_ITEMS = 8;
constexpr int AP_TILE = AP_THREADS * AP_ITEMS;  // old entries per copy block
constexpr int AP_WIN = 4096;               // cut points of one copy tile staged in LDS (more: searched in global memory)

__device__ __forceinline__ int64_t entry_owner(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, uint32_t j) {
  return (j & 1u) ? dst[j >> 1] : src[j >> 1];
}

// steps 1-2, m <= AP_SMALL: one workgroup, bitonic sort of M2 = pow2 >= m keys in LDS (padding keys sort last)
__global__ void __launch_bounds__(AP_SORT_THREADS) k_append_sort_small(uint32_t m, uint32_t M2, const int64_t* __restrict__ src,
                                                                      const int64_t* __restrict__ dst,
                                                                      const int64_t* __restrict__ indptr_old, int64_t n_old,
                                                                      uint32_t* __restrict__ S, uint32_t* __restrict__ J,
                                                                      uint32_t* __restrict__ INS) {
  __shared__ uint64_t key[AP_SMALL];
  const uint32_t t = threadIdx.x, T = blockDim.x;
  for (uint32_t j = t; j < M2; j += T)
    key[j] = j < m ? (((uint64_t)entry_owner(src, dst, j) << 12) | j) : ~0ull;
  __syncthreads();
  for (uint32_t k = 2; k <= M2; k <<= 1) {
    for (uint32_t h = k >> 1; h > 0; h >>= 1) {
      for (uint32_t i = t; i < (M2 >> 1); i += T) {
        const uint32_t a = ((i & ~(h - 1)) << 1) | (i & (h - 1)), b = a + h;
        const uint64_t x = key[a], y = key[b];
        const bool up = (a & k) == 0;
        if ((x > y) == up) {
          key[a] = y;
          key[b] = x;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t s = t; s < m; s += T) {
    const uint64_t v = key[s];
    const uint32_t own = (uint32_t)(v >> 12);
    S[s] = own;
    J[s] = (uint32_t)(v & 4095u);
    INS[s] = (uint32_t)indptr_old[min((int64_t)own + 1, n_old)];  // (an owner the old graph lacks: the end of the old array)
  }
}

// large path: keys for radix_sort_pairs, and INS from the sorted owners
__global__ void k_append_keys(uint32_t m, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                              uint32_t* __restrict__ k, uint32_t* __restrict__ v) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < m) {
    k[j] = (uint32_t)entry_owner(src, dst, (uint32_t)j);
    v[j] = (uint32_t)j;
  }
}
__global__ void k_append_ins(uint32_t m, const uint32_t* __restrict__ S, const int64_t* __restrict__ indptr_old, int64_t n_old,
                             uint32_t* __restrict__ INS) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < m) INS[s] = (uint32_t)indptr_old[min((int64_t)S[s] + 1, n_old)];
}

// steps 3-5.  Blocks [0, nb_new): the new entries; [nb_new, nb_new + nb_ptr): indptr; the rest: one tile of old entries each.
struct AppendArgs {
  tg_tcsr g;
  int64_t num_node_out;  // >= g.num_node: rows of indptr_out - 1
  uint32_t m;
  const uint32_t *S, *J, *INS;
  const int64_t *src, *dst, *eid;
  const double* ts;
  int64_t* indptr_out;
  double* ts_out;
  int32_t *nbr_out, *eid_out;
  uint32_t nb_new, nb_ptr;
};
__global__ void __launch_bounds__(AP_THREADS) k_append_apply(AppendArgs a) {
  __shared__ uint32_t win[AP_WIN];
  const uint32_t t = threadIdx.x;
  uint32_t b = blockIdx.x;
  if (b < a.nb_new) {  // step 5
    const uint64_t s = (uint64_t)b * AP_THREADS + t;
    if (s < a.m) {
      const uint32_t j = a.J[s], e = j >> 1, f = j & 1u;
      const uint64_t pos = (uint64_t)a.INS[s] + s;
      a.ts_out[pos] = a.ts[e];
      a.nbr_out[pos] = (int32_t)(f ? a.src[e] : a.dst[e]);
      a.eid_out[pos] = (int32_t)((uint32_t)a.eid[e] | (f << 31));
    }
    return;
  }
  b -= a.nb_new;
  if (b < a.nb_ptr) {  // step 3 (v = num_node_out included: lower_bound = m; v > num_node: the old prefix is the old total)
    const int64_t v = (int64_t)b * AP_THREADS + t;
    if (v <= a.num_node_out)
      a.indptr_out[v] = a.g.indptr[min(v, a.g.num_node)] + (int64_t)lower_bound_u32(a.S, 0u, a.m, (uint32_t)v);
    return;
  }
  b -= a.nb_ptr;  // step 4: old entries [p0, p1)
  const uint64_t P = (uint64_t)a.g.num_entry;
  const uint64_t p0 = (uint64_t)b * AP_TILE, p1 = min(p0 + AP_TILE, P);
  // cut points at or before p0 shift the whole tile; those inside (p0, p1 - 1] shift its tail: INS[lo .. hi)
  const uint32_t lo = upper_bound_u32(a.INS, 0u, a.m, (uint32_t)p0);
  // (2 n << 2 E: most tiles hold no cut point or a few, so the end of the window is galloped for from its start)
  uint32_t reach = 1;
  while (lo + reach < a.m && a.INS[lo + reach - 1] <= (uint32_t)(p1 - 1)) reach <<= 1;
  const uint32_t hi = lo < a.m ? upper_bound_u32(a.INS, lo, min(lo + reach, a.m), (uint32_t)(p1 - 1)) : lo;
  const uint32_t nwin = hi - lo;
  const bool staged = nwin <= (uint32_t)AP_WIN;  // block-uniform
  if (staged && nwin) {
    for (uint32_t i = t; i < nwin; i += AP_THREADS) win[i] = a.INS[lo + i];
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < AP_ITEMS; ++i) {
    const uint64_t p = p0 + (uint64_t)i * AP_THREADS + t;  // lane l takes entry base + l: loads and stores coalesce
    if (p >= p1) break;
    uint32_t shift = lo;
    if (nwin) shift += staged ? upper_bound_u32(win, 0u, nwin, (uint32_t)p) : upper_bound_u32(a.INS, lo, hi, (uint32_t)p) - lo;
    move_entry(a.g, (int64_t)p, a.ts_out, a.nbr_out, a.eid_out, (int64_t)(p + shift));
  }
}

static int append_key_bits(int64_t num_node) {
  int b = 1;
  while (((int64_t)1 << b) < num_node) ++b;
  return (b + 3) / 4 * 4;
}

// ---- late events: steps 1'-2' ----
// float64 -> uint64 whose unsigned order is the order of '<' on non-NaN values, with -0.0 and +0.0 on one key
__device__ __forceinline__ uint64_t time_key(double t) {
  if (t == 0.0) t = 0.0;  // (-0.0 == 0.0: the key of +0.0)
  const uint64_t b = (uint64_t)__double_as_longlong(t);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// INS of one new entry: the upper bound of t in the old row of `own` (an owner the old graph lacks: the empty row at the end)
__device__ __forceinline__ uint32_t merge_cut(const tg_tcsr& g, uint32_t own, double t) {
  const int64_t b = g.indptr[min((int64_t)own, g.num_node)], e = g.indptr[min((int64_t)own + 1, g.num_node)];
  int64_t lo = b, hi = e, step = 1;  // entries at or after hi are > t; the answer lies in [lo, hi]
  while (hi - step >= b) {
    if (g.ts[hi - step] > t) {
      hi -= step;
      step <<= 1;
    } else {
      lo = hi - step + 1;
      break;
    }
  }
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (g.ts[mid] > t) hi = mid;
    else lo = mid + 1;
  }
  return (uint32_t)lo;
}

// m <= MG_SMALL: one workgroup, bitonic sort of M2 = pow2 >= m unique keys (owner : time key : j) in LDS, then INS
__global__ void __launch_bounds__(AP_SORT_THREADS) k_merge_sort_small(uint32_t m, uint32_t M2, const int64_t* __restrict__ src,
                                                                     const int64_t* __restrict__ dst,
                                                                     const double* __restrict__ ts, tg_tcsr g,
                                                                     uint32_t* __restrict__ S, uint32_t* __restrict__ J,
                                                                     uint32_t* __restrict__ INS) {
  __shared__ uint64_t khi[MG_SMALL];  // owner << 32 | time key >> 32
  __shared__ uint64_t klo[MG_SMALL];  // time key << 32 | j
  const uint32_t t = threadIdx.x, T = blockDim.x;
  for (uint32_t j = t; j < M2; j += T) {
    uint64_t h = ~0ull, l = ~0ull;  // padding keys sort last
    if (j < m) {
      const uint64_t tk = time_key(ts[j >> 1]);
      h = ((uint64_t)entry_owner(src, dst, j) << 32) | (tk >> 32);
      l = (tk << 32) | j;
    }
    khi[j] = h;
    klo[j] = l;
  }
  __syncthreads();
  for (uint32_t k = 2; k <= M2; k <<= 1) {
    for (uint32_t h = k >> 1; h > 0; h >>= 1) {
      for (uint32_t i = t; i < (M2 >> 1); i += T) {
        const uint32_t a = ((i & ~(h - 1)) << 1) | (i & (h - 1)), b = a + h;
        const uint64_t xh = khi[a], yh = khi[b], xl = klo[a], yl = klo[b];
        const bool up = (a & k) == 0;
        if ((xh > yh || (xh == yh && xl > yl)) == up) {
          khi[a] = yh;
          khi[b] = xh;
          klo[a] = yl;
          klo[b] = xl;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t s = t; s < m; s += T) {
    const uint32_t own = (uint32_t)(khi[s] >> 32), j = (uint32_t)klo[s];
    S[s] = own;
    J[s] = j;
    INS[s] = merge_cut(g, own, ts[j >> 1]);
  }
}

// large path: the key of a pass from the payload j (WORD 0: time key, low word - also writes the payload; 1: high word; 2: owner)
template <int WORD>
__global__ void k_merge_keys(uint32_t m, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                             const double* __restrict__ ts, uint32_t* __restrict__ k, uint32_t* __restrict__ v) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t j = WORD == 0 ? (uint32_t)i : v[i];
  if (WORD == 0) v[i] = j;
  if (WORD == 2) k[i] = (uint32_t)entry_owner(src, dst, j);
  else k[i] = (uint32_t)(time_key(ts[j >> 1]) >> (WORD == 1 ? 32 : 0));
}
__global__ void k_merge_ins(uint32_t m, const uint32_t* __restrict__ S, const uint32_t* __restrict__ J,
                            const double* __restrict__ ts, tg_tcsr g, uint32_t* __restrict__ INS) {
  const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < m) INS[s] = merge_cut(g, S[s], ts[J[s] >> 1]);
}

// steps 3-5 for either entry: one launch of k_append_apply
static int launch_apply(const char* what, const tg_tcsr* g, int64_t num_node_out, uint32_t m, const uint32_t* S,
                        const uint32_t* J, const uint32_t* INS, const int64_t* src, const int64_t* dst, const double* ts,
                        const int64_t* eid, int64_t* indptr_out, double* ts_out, int32_t* nbr_out, int32_t* eid_out,
                        hipStream_t st) {
  AppendArgs a{};
  a.g = *g;
  a.num_node_out = num_node_out;
  a.m = m;
  a.S = S;
  a.J = J;
  a.INS = INS;
  a.src = src;
  a.dst = dst;
  a.eid = eid;
  a.ts = ts;
  a.indptr_out = indptr_out;
  a.ts_out = ts_out;
  a.nbr_out = nbr_out;
  a.eid_out = eid_out;
  a.nb_new = (uint32_t)cdiv(m, AP_THREADS);
  a.nb_ptr = (uint32_t)cdiv(num_node_out + 1, AP_THREADS);
  const uint32_t nb_copy = (uint32_t)cdiv(g->num_entry, AP_TILE);
  hipLaunchKernelGGL(k_append_apply, dim3(a.nb_new + a.nb_ptr + nb_copy), dim3(AP_THREADS), 0, st, a);
  return check_launch(what);
}

// what both entries refuse before anything else (device pointers are not read)
static int append_args(const tg_tcsr* g, int64_t num_node_out, int64_t n_new, const void* src, const void* dst, const void* ts,
                       const void* eid, const void* indptr_out, const void* ts_out, const void* nbr_out, const void* eid_out) {
  if (!g || n_new < 0 || g->num_node <= 0 || g->num_node > 0x7fffffffLL || g->num_entry < 0 || !g->indptr || !indptr_out)
    return TG_EINVAL;
  if (num_node_out < g->num_node || num_node_out > 0x7fffffffLL) return TG_EINVAL;
  if ((uint64_t)g->num_entry + 2 * (uint64_t)n_new > 0xffffffffull) return TG_EINVAL;
  if (g->num_entry > 0 && (!g->ts || !g->nbr || !g->eid)) return TG_EINVAL;
  if (g->num_entry + 2 * n_new > 0 && (!ts_out || !nbr_out || !eid_out)) return TG_EINVAL;
  if (n_new > 0 && (!src || !dst || !ts || !eid)) return TG_EINVAL;
  return TG_OK;
}

}  // namespace tg

using namespace tg;

extern "C" size_t tg_tcsr_append_grow_workspace_bytes(int64_t num_entry_old, int64_t n_new, int64_t num_node,
                                                      int64_t num_node_out) {
  if (num_entry_old < 0 || n_new < 0 || num_node <= 0 || num_node_out < num_node || num_node_out > 0x7fffffffLL) return 0;
  const size_t m = 2 * (size_t)n_new;
  if (m == 0) return 0;
  if (m <= (size_t)AP_SMALL) return 3 * align16(m * 4) + 256;
  return 5 * align16(m * 4) + radix_sort_scratch_bytes((uint32_t)m) + 256;
}

extern "C" size_t tg_tcsr_append_workspace_bytes(int64_t num_entry_old, int64_t n_new, int64_t num_node) {
  return tg_tcsr_append_grow_workspace_bytes(num_entry_old, n_new, num_node, num_node);
}

extern "C" int tg_tcsr_append_grow(const tg_tcsr* g, int64_t num_node_out, int64_t n_new, const int64_t* src, const int64_t* dst,
                                   const double* ts, const int64_t* eid, int64_t* indptr_out, double* ts_out, int32_t* nbr_out,
                                   int32_t* eid_out, void* ws, size_t ws_bytes, void* stream) {
  const int bad = append_args(g, num_node_out, n_new, src, dst, ts, eid, indptr_out, ts_out, nbr_out, eid_out);
  if (bad != TG_OK) return bad;
  hipStream_t st = as_stream(stream);
  const uint32_t m = (uint32_t)(2 * n_new);
  uint32_t *S = nullptr, *J = nullptr, *INS = nullptr;
  if (m) {  // every workspace check comes before the first launch
    Carver cv(ws, ws_bytes);
    if (m <= (uint32_t)AP_SMALL) {
      S = cv.take<uint32_t>(m);
      J = cv.take<uint32_t>(m);
      INS = cv.take<uint32_t>(m);
      if (!cv.ok) return TG_EWORKSPACE;
      uint32_t M2 = 128;
      while (M2 < m) M2 <<= 1;
      const unsigned threads = std::min<unsigned>(AP_SORT_THREADS, M2 / 2);
      hipLaunchKernelGGL(k_append_sort_small, dim3(1), dim3(threads), 0, st, m, M2, src, dst, g->indptr, g->num_node, S, J, INS);
    } else {
      uint32_t* k0 = cv.take<uint32_t>(m);
      uint32_t* v0 = cv.take<uint32_t>(m);
      uint32_t* k1 = cv.take<uint32_t>(m);
      uint32_t* v1 = cv.take<uint32_t>(m);
      INS = cv.take<uint32_t>(m);
      const size_t sb = radix_sort_scratch_bytes(m);
      char* scratch = cv.take<char>(sb);
      if (!cv.ok) return TG_EWORKSPACE;
      hipLaunchKernelGGL(k_append_keys, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, st, m, src, dst, k0, v0);
      const int rc = radix_sort_pairs(m, append_key_bits(num_node_out), k0, v0, k1, v1, scratch, sb, st);
      if (rc != TG_OK) return rc;
      S = k0;
      J = v0;
      hipLaunchKernelGGL(k_append_ins, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, st, m, S, g->indptr, g->num_node, INS);
    }
  }
  return launch_apply("tg_tcsr_append_grow", g, num_node_out, m, S, J, INS, src, dst, ts, eid, indptr_out, ts_out, nbr_out, eid_out,
                      st);
}

extern "C" int tg_tcsr_append(const tg_tcsr* g, int64_t n_new, const int64_t* src, const int64_t* dst, const double* ts,
                              const int64_t* eid, int64_t* indptr_out, double* ts_out, int32_t* nbr_out, int32_t* eid_out,
                              void* ws, size_t ws_bytes, void* stream) {
  if (!g) return TG_EINVAL;
  return tg_tcsr_append_grow(g, g->num_node, n_new, src, dst, ts, eid, indptr_out, ts_out, nbr_out, eid_out, ws, ws_bytes, stream);
}

// The host twin: plain C++ over host pointers, the same arrays as tg_tcsr_build_host over [old events | new events] with
// num_node_out nodes.
extern "C" int tg_tcsr_append_grow_host(const tg_tcsr* g, int64_t num_node_out, int64_t n_new, const int64_t* src,
                                        const int64_t* dst, const double* ts, const int64_t* eid, int64_t* indptr_out,
                                        double* ts_out, int32_t* nbr_out, int32_t* eid_out) {
  if (!g || n_new < 0 || g->num_node <= 0 || g->num_node > 0x7fffffffLL || g->num_entry < 0 || !g->indptr || !indptr_out)
    return TG_EINVAL;
  if (num_node_out < g->num_node || num_node_out > 0x7fffffffLL) return TG_EINVAL;
  if ((uint64_t)g->num_entry + 2 * (uint64_t)n_new > 0xffffffffull) return TG_EINVAL;
  const int64_t N0 = g->num_node, N = num_node_out;
  for (int64_t i = 0; i < n_new; ++i) {
    if (src[i] < 0 || src[i] >= N || dst[i] < 0 || dst[i] >= N) return TG_EINVAL;
    if (eid[i] < 0 || eid[i] > 0x7fffffffLL) return TG_EINVAL;
  }
  std::vector<int64_t> add(N + 1, 0);
  for (int64_t i = 0; i < n_new; ++i) {
    add[src[i] + 1]++;
    add[dst[i] + 1]++;
  }
  for (int64_t v = 0; v < N; ++v) add[v + 1] += add[v];  // add[v]: new entries of nodes below v
  for (int64_t v = 0; v <= N; ++v) indptr_out[v] = g->indptr[std::min(v, N0)] + add[v];  // (a new id: the old total)
  std::vector<int64_t> cur(N);
  for (int64_t v = 0; v < N; ++v) {
    const int64_t lo = g->indptr[std::min(v, N0)], len = g->indptr[std::min(v + 1, N0)] - lo, q = indptr_out[v];
    std::copy(g->ts + lo, g->ts + lo + len, ts_out + q);
    std::copy(g->nbr + lo, g->nbr + lo + len, nbr_out + q);
    std::copy(g->eid + lo, g->eid + lo + len, eid_out + q);
    cur[v] = q + len;
  }
  for (int64_t i = 0; i < n_new; ++i) {
    int64_t p = cur[src[i]]++;
    ts_out[p] = ts[i];
    nbr_out[p] = (int32_t)dst[i];
    eid_out[p] = (int32_t)eid[i];
    p = cur[dst[i]]++;
    ts_out[p] = ts[i];
    nbr_out[p] = (int32_t)src[i];
    eid_out[p] = (int32_t)((uint32_t)eid[i] | 0x80000000u);
  }
  return TG_OK;
}

extern "C" int tg_tcsr_append_host(const tg_tcsr* g, int64_t n_new, const int64_t* src, const int64_t* dst, const double* ts,
                                   const int64_t* eid, int64_t* indptr_out, double* ts_out, int32_t* nbr_out,
                                   int32_t* eid_out) {
  if (!g) return TG_EINVAL;
  return tg_tcsr_append_grow_host(g, g->num_node, n_new, src, dst, ts, eid, indptr_out, ts_out, nbr_out, eid_out);
}

// ---- late events: a batch in any order, with any non-NaN times (steps 1'-2' above, then the append's apply launch) ----
extern "C" size_t tg_tcsr_merge_workspace_bytes(int64_t num_entry_old, int64_t n_new, int64_t num_node, int64_t num_node_out) {
  if (num_entry_old < 0 || n_new < 0 || num_node <= 0 || num_node_out < num_node || num_node_out > 0x7fffffffLL) return 0;
  const size_t m = 2 * (size_t)n_new;
  if (m == 0) return 0;
  if (m <= (size_t)MG_SMALL) return 3 * align16(m * 4) + 256;
  // two (key, payload) ping-pong pairs serve all three sorts: each pass derives its keys from the payload in place
  return 5 * align16(m * 4) + radix_sort_scratch_bytes((uint32_t)m) + 256;
}

extern "C" int tg_tcsr_merge(const tg_tcsr* g, int64_t num_node_out, int64_t n_new, const int64_t* src, const int64_t* dst,
                             const double* ts, const int64_t* eid, int64_t* indptr_out, double* ts_out, int32_t* nbr_out,
                             int32_t* eid_out, void* ws, size_t ws_bytes, void* stream) {
  const int bad = append_args(g, num_node_out, n_new, src, dst, ts, eid, indptr_out, ts_out, nbr_out, eid_out);
  if (bad != TG_OK) return bad;
  hipStream_t st = as_stream(stream);
  const uint32_t m = (uint32_t)(2 * n_new);
  uint32_t *S = nullptr, *J = nullptr, *INS = nullptr;
  if (m) {  // every workspace check comes before the first launch
    Carver cv(ws, ws_bytes);
    if (m <= (uint32_t)MG_SMALL) {
      S = cv.take<uint32_t>(m);
      J = cv.take<uint32_t>(m);
      INS = cv.take<uint32_t>(m);
      if (!cv.ok) return TG_EWORKSPACE;
      uint32_t M2 = 128;
      while (M2 < m) M2 <<= 1;
      const unsigned threads = std::min<unsigned>(AP_SORT_THREADS, M2 / 2);
      hipLaunchKernelGGL(k_merge_sort_small, dim3(1), dim3(threads), 0, st, m, M2, src, dst, ts, *g, S, J, INS);
    } else {
      uint32_t* k0 = cv.take<uint32_t>(m);
      uint32_t* v0 = cv.take<uint32_t>(m);
      uint32_t* k1 = cv.take<uint32_t>(m);
      uint32_t* v1 = cv.take<uint32_t>(m);
      INS = cv.take<uint32_t>(m);
      const size_t sb = radix_sort_scratch_bytes(m);
      char* scratch = cv.take<char>(sb);
      if (!cv.ok) return TG_EWORKSPACE;
      const dim3 grid((unsigned)cdiv(m, 256)), block(256);
      // least significant key first; every sort is stable, and the payload starts in ascending j
      hipLaunchKernelGGL(k_merge_keys<0>, grid, block, 0, st, m, src, dst, ts, k0, v0);
      int rc = radix_sort_pairs(m, 32, k0, v0, k1, v1, scratch, sb, st);
      if (rc != TG_OK) return rc;
      hipLaunchKernelGGL(k_merge_keys<1>, grid, block, 0, st, m, src, dst, ts, k0, v0);
      rc = radix_sort_pairs(m, 32, k0, v0, k1, v1, scratch, sb, st);
      if (rc != TG_OK) return rc;
      hipLaunchKernelGGL(k_merge_keys<2>, grid, block, 0, st, m, src, dst, ts, k0, v0);
      rc = radix_sort_pairs(m, append_key_bits(num_node_out), k0, v0, k1, v1, scratch, sb, st);
      if (rc != TG_OK) return rc;
      S = k0;
      J = v0;
      hipLaunchKernelGGL(k_merge_ins, grid, block, 0, st, m, S, J, ts, *g, INS);
    }
  }
  return launch_apply("tg_tcsr_merge", g, num_node_out, m, S, J, INS, src, dst, ts, eid, indptr_out, ts_out, nbr_out, eid_out, st);
}

// The host twin: per row, the old row merged with the node's new entries (taken in ascending j, sorted stably by time);
// a new entry goes first only where its time is strictly below the old one's.
extern "C" int tg_tcsr_merge_host(const tg_tcsr* g, int64_t num_node_out, int64_t n_new, const int64_t* src, const int64_t* dst,
                                  const double* ts, const int64_t* eid, int64_t* indptr_out, double* ts_out, int32_t* nbr_out,
                                  int32_t* eid_out) {
  if (!g || n_new < 0 || g->num_node <= 0 || g->num_node > 0x7fffffffLL || g->num_entry < 0 || !g->indptr || !indptr_out)
    return TG_EINVAL;
  if (num_node_out < g->num_node || num_node_out > 0x7fffffffLL) return TG_EINVAL;
  if ((uint64_t)g->num_entry + 2 * (uint64_t)n_new > 0xffffffffull) return TG_EINVAL;
  const int64_t N0 = g->num_node, N = num_node_out;
  for (int64_t i = 0; i < n_new; ++i) {
    if (src[i] < 0 || src[i] >= N || dst[i] < 0 || dst[i] >= N) return TG_EINVAL;
    if (eid[i] < 0 || eid[i] > 0x7fffffffLL) return TG_EINVAL;
    if (ts[i] != ts[i]) return TG_EINVAL;  // (a NaN has no place in a row)
  }
  std::vector<int64_t> add(N + 1, 0);
  for (int64_t i = 0; i < n_new; ++i) {
    add[src[i] + 1]++;
    add[dst[i] + 1]++;
  }
  for (int64_t v = 0; v < N; ++v) add[v + 1] += add[v];  // add[v]: new entries of nodes below v
  for (int64_t v = 0; v <= N; ++v) indptr_out[v] = g->indptr[std::min(v, N0)] + add[v];
  std::vector<int64_t> bucket(2 * n_new), cur(add.begin(), add.end() - 1);  // the entries j of every owner, ascending
  for (int64_t j = 0; j < 2 * n_new; ++j) bucket[cur[(j & 1) ? dst[j >> 1] : src[j >> 1]]++] = j;
  for (int64_t v = 0; v < N; ++v) {
    int64_t p = g->indptr[std::min(v, N0)], q = indptr_out[v];
    const int64_t p1 = g->indptr[std::min(v + 1, N0)];
    int64_t* b0 = bucket.data() + add[v];
    int64_t* b1 = bucket.data() + add[v + 1];
    std::stable_sort(b0, b1, [&](int64_t a, int64_t b) { return ts[a >> 1] < ts[b >> 1]; });
    while (p < p1 || b0 < b1) {
      if (b0 < b1 && (p == p1 || ts[*b0 >> 1] < g->ts[p])) {
        const int64_t j = *b0++, e = j >> 1;
        ts_out[q] = ts[e];
        nbr_out[q] = (int32_t)((j & 1) ? src[e] : dst[e]);
        eid_out[q] = (int32_t)((uint32_t)eid[e] | ((uint32_t)(j & 1) << 31));
      } else {
        ts_out[q] = g->ts[p];
        nbr_out[q] = g->nbr[p];
        eid_out[q] = g->eid[p];
        ++p;
      }
      ++q;
    }
  }
  return TG_OK;
}
