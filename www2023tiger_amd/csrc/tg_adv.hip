// Historical / inductive negative sampling (Poursafaei et al., NeurIPS 2022) over the T-CSR.
// Reference: tiger/data/adversarial.py:36-117 (AdversarialEdgeSampler).  The reference rebuilds, for every chunk of
// queries, the edge sets of the whole stream up to the chunk's time in a Python loop.  Here a query is a filter over
// the node's time-sorted entries before t0 (the prefix the recent-edges sampler searches, tg_sample.h: prefix_end),
// with a per-entry predicate read from a pair index built once (tiger_hip.h: tg_adv_index):
//   hist:  next_ts[e] > t1                              (the pair does not recur in [t0, t1])
//   ind:   next_ts[e] > t1  and  first_ts[e] > ts_hist_end
// Integer work and comparisons only: host and device results are bit-exact.
#include <algorithm>
#include <cmath>
#include <vector>

#include "tg_step.h"
#include "tg_sample.h"

namespace tg {

// ---- counter-based draws (tiger_hip.h: tg_adv_hash; a stream of its own, dropout's drop_keep is separate) ----------
enum { ADV_PICK = 7, ADV_FALLBACK = 8 };
__host__ __device__ __forceinline__ uint32_t adv_mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
__host__ __device__ __forceinline__ uint32_t adv_hash(uint64_t seed, uint64_t counter, uint64_t q, uint32_t s) {
  const uint64_t k = seed ^ (counter * 0x9E3779B97F4A7C15ull);
  uint32_t h = adv_mix32((uint32_t)q ^ (uint32_t)k);
  h = adv_mix32(h + (uint32_t)(q >> 32) * 0x9e3779b9u + (uint32_t)(k >> 32));
  return adv_mix32(h ^ (s * 0x85ebca6bu));
}
__host__ __device__ __forceinline__ uint64_t mulhi32(uint32_t h, uint64_t c) { return ((uint64_t)h * c) >> 32; }

__host__ __device__ __forceinline__ bool adv_pass(const double* __restrict__ next_ts, const double* __restrict__ first_ts,
                                                  int64_t e, double t1, int mode, double hist_end) {
  return next_ts[e] > t1 && (mode == TG_ADV_HIST || first_ts[e] > hist_end);
}

// ---- pair index, device build ---------------------------------------------------------------------------------------
constexpr uint32_t ADV_IN_ENTRY = 0xffffffffu;  // placeholder neighbour key of an entry seen from the destination side

// per entry: its owner (upper bound over indptr) and the first sort key - the neighbour, or num_node for entries seen
// from the destination side, so that they follow every out-entry of their node
__global__ void k_adv_keys(tg_tcsr g, uint32_t* __restrict__ key, uint32_t* __restrict__ val, uint32_t* __restrict__ owner) {
  const uint64_t P = (uint64_t)g.num_entry;
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (uint64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = g.num_node;  // last node n with indptr[n] <= p
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (g.indptr[mid] <= (int64_t)p)
        lo = mid;
      else
        hi = mid;
    }
    owner[p] = (uint32_t)lo;
    const bool in_entry = (uint32_t)g.eid[p] >> 31;
    key[p] = in_entry ? (uint32_t)g.num_node : (uint32_t)g.nbr[p];
    val[p] = (uint32_t)p;
  }
}

__global__ void k_adv_owner_keys(uint32_t P, const uint32_t* __restrict__ val, const uint32_t* __restrict__ owner,
                                 uint32_t* __restrict__ key) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (uint64_t)gridDim.x * blockDim.x)
    key[i] = owner[val[i]];
}

__device__ __forceinline__ uint32_t adv_pair_key(const tg_tcsr& g, uint32_t p) {
  return ((uint32_t)g.eid[p] >> 31) ? ADV_IN_ENTRY : (uint32_t)g.nbr[p];
}

// sorted position i (entry p = order[i] of node `o`): the node's run in sorted order is [indptr[o], indptr[o + 1]) and
// holds its out-entries grouped by neighbour in T-CSR order, then its in-entries
__global__ void k_adv_fill(tg_tcsr g, const uint32_t* __restrict__ order, const uint32_t* __restrict__ own,
                           double* __restrict__ next_ts, double* __restrict__ first_ts) {
  const uint64_t P = (uint64_t)g.num_entry;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t p = order[i];
    const uint32_t k = adv_pair_key(g, p);
    if (k == ADV_IN_ENTRY) {
      next_ts[p] = -INFINITY;
      first_ts[p] = -INFINITY;
      continue;
    }
    const int64_t lo = g.indptr[own[i]], hi = g.indptr[own[i] + 1];
    double nx = INFINITY;
    if ((int64_t)i + 1 < hi && adv_pair_key(g, order[i + 1]) == k) nx = g.ts[order[i + 1]];
    int64_t a = lo, b = (int64_t)i;  // first sorted position of the group: lower bound of k in [lo, i]
    while (a < b) {
      const int64_t mid = (a + b) >> 1;
      if (adv_pair_key(g, order[mid]) < k)
        a = mid + 1;
      else
        b = mid;
    }
    next_ts[p] = nx;
    first_ts[p] = g.ts[order[a]];
  }
}

static int bits_for(uint64_t max_key) {
  int b = 4;
  while (b < 32 && (max_key >> b) != 0) b += 4;
  return b;
}

// ---- the sampler: one wavefront per query ----------------------------------------------------------------------------
struct AdvArgs {
  tg_tcsr g;
  tg_adv_index ix;
  int64_t n;
  const int64_t* srcs;
  const double *t0, *t1;
  int mode;
  double hist_end;
  const int64_t* dst_distinct;
  int64_t n_dd;
  uint64_t seed, counter;
  int64_t *out_dst, *out_count;
};

__global__ void __launch_bounds__(256) k_adv_neg_sample(AdvArgs a) {
  const int lane = lane_id();
  const int64_t wpb = blockDim.x / TG_WAVE;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t q = (int64_t)blockIdx.x * wpb + threadIdx.x / TG_WAVE; q < a.n; q += (int64_t)gridDim.x * wpb) {
    const int64_t s = a.srcs[q];
    const double t0 = a.t0[q], t1 = a.t1[q];
    if (!(t0 <= t1)) {  // wave-uniform
      if (lane == 0) {
        a.out_dst[q] = -1;
        if (a.out_count) a.out_count[q] = -1;
      }
      continue;
    }
    int64_t start;
    const int64_t end = prefix_end_group<64>(a.g, s, t0, &start, lane);  // entries [start, end): ts < t0
    // pass 1: count the candidates, 64 entries per round
    uint64_t count = 0;
    for (int64_t base = start; base < end; base += TG_WAVE) {
      const int64_t e = base + lane;
      const bool ok = e < end && adv_pass(a.ix.next_ts, a.ix.first_ts, e, t1, a.mode, a.hist_end);
      count += (uint64_t)__popcll(__ballot(ok));
    }
    if (count == 0) {
      if (lane == 0) {
        a.out_dst[q] = a.dst_distinct[mulhi32(adv_hash(a.seed, a.counter, (uint64_t)q, ADV_FALLBACK), (uint64_t)a.n_dd)];
        if (a.out_count) a.out_count[q] = 0;
      }
      continue;
    }
    // pass 2: the k-th candidate in entry order
    const uint64_t k = mulhi32(adv_hash(a.seed, a.counter, (uint64_t)q, ADV_PICK), count);
    uint64_t seen = 0;
    for (int64_t base = start; base < end; base += TG_WAVE) {
      const int64_t e = base + lane;
      const bool ok = e < end && adv_pass(a.ix.next_ts, a.ix.first_ts, e, t1, a.mode, a.hist_end);
      const unsigned long long m = __ballot(ok);
      const uint64_t c = (uint64_t)__popcll(m);
      if (k < seen + c) {  // wave-uniform
        if (ok && seen + (uint64_t)__popcll(m & below) == k) a.out_dst[q] = (int64_t)a.g.nbr[e];
        break;
      }
      seen += c;
    }
    if (lane == 0 && a.out_count) a.out_count[q] = (int64_t)count;
  }
}

static bool adv_args_ok(int64_t n, int32_t mode, int64_t n_dd) {
  return n >= 0 && (mode == TG_ADV_HIST || mode == TG_ADV_IND) && n_dd >= 1 && n_dd <= 0xffffffffLL;
}

}  // namespace tg

using namespace tg;

// ---- host twins -------------------------------------------------------------------------------------------------------
extern "C" int tg_adv_index_build_host(const tg_tcsr* g, double* next_ts, double* first_ts) {
  if (!g || g->num_node <= 0 || g->num_entry < 0) return TG_EINVAL;
  if (g->num_entry == 0) return TG_OK;
  if (!g->indptr || !g->ts || !g->nbr || !g->eid || !next_ts || !first_ts) return TG_EINVAL;
  std::vector<int64_t> out;
  for (int64_t s = 0; s < g->num_node; ++s) {
    const int64_t lo = g->indptr[s], hi = g->indptr[s + 1];
    out.clear();
    for (int64_t e = lo; e < hi; ++e) {
      if ((uint32_t)g->eid[e] >> 31) {
        next_ts[e] = first_ts[e] = -INFINITY;
      } else {
        out.push_back(e);
      }
    }
    // group the out-entries by neighbour, T-CSR order inside a group
    std::stable_sort(out.begin(), out.end(), [&](int64_t x, int64_t y) { return g->nbr[x] < g->nbr[y]; });
    for (size_t i = 0; i < out.size();) {
      size_t j = i;
      while (j < out.size() && g->nbr[out[j]] == g->nbr[out[i]]) ++j;
      const double first = g->ts[out[i]];
      for (size_t r = i; r < j; ++r) {
        next_ts[out[r]] = r + 1 < j ? g->ts[out[r + 1]] : INFINITY;
        first_ts[out[r]] = first;
      }
      i = j;
    }
  }
  return TG_OK;
}

extern "C" int tg_adv_neg_sample_host(const tg_tcsr* g, const tg_adv_index* ix, int64_t n, const int64_t* srcs,
                                      const double* t0, const double* t1, int32_t mode, double hist_end,
                                      const int64_t* dst_distinct, int64_t n_dd, uint64_t seed, uint64_t counter,
                                      int64_t* out_dst, int64_t* out_count) {
  if (!g || !ix || !adv_args_ok(n, mode, n_dd)) return TG_EINVAL;
  if (n == 0) return TG_OK;
  if (!srcs || !t0 || !t1 || !dst_distinct || !out_dst) return TG_EINVAL;
  for (int64_t q = 0; q < n; ++q)
    if (!(t0[q] <= t1[q])) return TG_EINVAL;
  for (int64_t q = 0; q < n; ++q) {
    const int64_t s = srcs[q];
    int64_t start = 0, end = 0;
    if (s >= 0 && s < g->num_node) {
      start = g->indptr[s];
      end = std::lower_bound(g->ts + start, g->ts + g->indptr[s + 1], t0[q]) - g->ts;  // ts < t0
    }
    uint64_t count = 0;
    for (int64_t e = start; e < end; ++e) count += adv_pass(ix->next_ts, ix->first_ts, e, t1[q], mode, hist_end);
    if (count == 0) {
      out_dst[q] = dst_distinct[mulhi32(adv_hash(seed, counter, (uint64_t)q, ADV_FALLBACK), (uint64_t)n_dd)];
    } else {
      const uint64_t k = mulhi32(adv_hash(seed, counter, (uint64_t)q, ADV_PICK), count);
      uint64_t seen = 0;
      for (int64_t e = start; e < end; ++e) {
        if (!adv_pass(ix->next_ts, ix->first_ts, e, t1[q], mode, hist_end)) continue;
        if (seen++ == k) {
          out_dst[q] = (int64_t)g->nbr[e];
          break;
        }
      }
    }
    if (out_count) out_count[q] = (int64_t)count;
  }
  return TG_OK;
}

// ---- device entries ---------------------------------------------------------------------------------------------------
extern "C" size_t tg_adv_index_build_device_workspace_bytes(int64_t num_entry, int64_t num_node) {
  if (num_entry < 0 || num_node <= 0 || num_entry > 0xffffffffLL) return 0;
  const size_t P = (size_t)num_entry;
  return align16(P * 4) * 5 + radix_sort_scratch_bytes((uint32_t)P) + 256;
}

extern "C" int tg_adv_index_build_device(const tg_tcsr* g, double* next_ts, double* first_ts, void* ws, size_t ws_bytes,
                                         void* stream) {
  if (!g || g->num_node <= 0 || g->num_node > 0x7fffffffLL || g->num_entry < 0 || g->num_entry > 0xffffffffLL)
    return TG_EINVAL;
  if (g->num_entry == 0) return TG_OK;
  if (!g->indptr || !g->ts || !g->nbr || !g->eid || !next_ts || !first_ts) return TG_EINVAL;
  hipStream_t st = as_stream(stream);
  const uint32_t P = (uint32_t)g->num_entry;
  Carver cv(ws, ws_bytes);
  uint32_t* k = cv.take<uint32_t>(P);
  uint32_t* v = cv.take<uint32_t>(P);
  uint32_t* k_alt = cv.take<uint32_t>(P);
  uint32_t* v_alt = cv.take<uint32_t>(P);
  uint32_t* owner = cv.take<uint32_t>(P);
  const size_t sbytes = radix_sort_scratch_bytes(P);
  void* scratch = cv.take<uint8_t>(sbytes);
  if (!cv.ok) return TG_EWORKSPACE;
  const tg_tcsr gv = *g;
  hipLaunchKernelGGL(k_adv_keys, dim3(flat_grid(P, 256)), dim3(256), 0, st, gv, k, v, owner);
  // stable on the neighbour key, then stable on the owner: (owner, neighbour, entry) order
  int rc = radix_sort_pairs(P, bits_for((uint64_t)g->num_node), k, v, k_alt, v_alt, scratch, sbytes, st);
  if (rc != TG_OK) return rc;
  hipLaunchKernelGGL(k_adv_owner_keys, dim3(flat_grid(P, 256)), dim3(256), 0, st, P, v, owner, k);
  rc = radix_sort_pairs(P, bits_for((uint64_t)(g->num_node - 1)), k, v, k_alt, v_alt, scratch, sbytes, st);
  if (rc != TG_OK) return rc;
  hipLaunchKernelGGL(k_adv_fill, dim3(flat_grid(P, 256)), dim3(256), 0, st, gv, v, k, next_ts, first_ts);
  return check_launch("tg_adv_index_build_device");
}

extern "C" int tg_adv_neg_sample(const tg_tcsr* g, const tg_adv_index* ix, int64_t n, const int64_t* srcs, const double* t0,
                                 const double* t1, int32_t mode, double hist_end, const int64_t* dst_distinct, int64_t n_dd,
                                 uint64_t seed, uint64_t counter, int64_t* out_dst, int64_t* out_count, void* stream) {
  if (!g || !ix || !adv_args_ok(n, mode, n_dd)) return TG_EINVAL;
  if (n == 0) return TG_OK;
  if (!srcs || !t0 || !t1 || !dst_distinct || !out_dst) return TG_EINVAL;
  if (g->num_entry > 0 && (!ix->next_ts || !ix->first_ts || !g->indptr || !g->ts || !g->nbr)) return TG_EINVAL;
  AdvArgs a{*g, *ix, n, srcs, t0, t1, mode, hist_end, dst_distinct, n_dd, seed, counter, out_dst, out_count};
  hipLaunchKernelGGL(k_adv_neg_sample, dim3(flat_grid(n, 4)), dim3(256), 0, as_stream(stream), a);
  return check_launch("tg_adv_neg_sample");
}
