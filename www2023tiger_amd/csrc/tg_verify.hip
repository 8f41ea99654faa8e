// Is this a T-CSR the library may read?  (Loading a saved online graph: Graph.from_state_dict; reference tiger/data/graph.py:
// 11-42 builds its adjacency lists in the same process that reads them and has no counterpart of this.)
//
// Every sampler, tg_seen_mask, the walk, trending and the restarters' histories use indptr, nbr and eid as addresses
// without checking them.  Arrays that do not come from this library's own kernels are checked here first, in one pass over
// the 20 bytes of every entry and the 8 bytes of every row bound.  Classes (tiger_hip.h: TG_VERIFY_*), first[c] = the
// SMALLEST violating index:
//   ENDS       indptr[0] != 0 (index 0) or indptr[N] != num_entry (index N)
//   PTR_ORDER  v with indptr[v + 1] < indptr[v]
//   TS_ORDER   p > 0, no row start, with ts[p] < ts[p - 1] (float64 '<': a comparison with a NaN is no violation);
//              a row start is a p with owner(p) != owner(p - 1) (tg_tcsr.h).  Reported only when ENDS and PTR_ORDER are
//              clean - the rows mean nothing otherwise: bit 0 and index -1 then.
//   TS_NAN     p with ts[p] != ts[p]
//   NBR_RANGE  p with nbr[p] < 0 or nbr[p] >= N
//   EID_RANGE  p with (eid[p] & 0x7fffffff) >= eid_rows; off with eid_rows < 0
// and the largest non-NaN ts (-inf without one; +0 above -0).
//   entries (k_verify_entries, one workgroup per tile of VF_TILE = 2048 entries): lane l takes entries base + l + 256 i:
//           loads coalesce.  An entry also loads the time in front of it (the tile's first entry the last one of the tile
//           before: a tile reads its own predecessor, no second pass over the seams).  The rows of [p0 - 1, p_last] come
//           from row_window (tg_tcsr.h: up to VF_WIN rows in LDS; a tile that spans more - thousands of empty rows -
//           searches global memory).  An owner is looked for only where the time goes DOWN: in a clean graph that is at row
//           starts alone, so the common entry costs no search.
//   nodes   (k_verify_nodes, one workgroup per 256 of the num_node + 1 row bounds): ENDS and PTR_ORDER.
//   fold    (k_verify_fold, ONE workgroup): every workgroup of the two passes above wrote one partial record (8 words: four
//           / two minima as offsets into its tile, the maximum); the fold takes the minima and the maximum over all
//           records, applies the TS_ORDER rule and writes out8.
// No atomics (the result does not depend on the launch geometry), no grid is capped, nothing is read back: the caller
// reads the 8 words when it wants them.
//
// SAFETY, by construction: every address formed below comes from a loop index bounded by num_node or num_entry AS PASSED
// IN (p < num_entry, v <= num_node, and row_window's searches, which stay inside indptr[1 .. N - 1] whatever it holds).  A
// value LOADED from the four arrays is only ever compared - with another loaded value, with a bound, with p - and never
// becomes an index or an offset.  (RowWindow::slot / searched compare p with loaded row bounds and return a POSITION of the
// search, in [0, nwin] / [lo, hi].)  So the kernels are safe on any array contents, a non-monotone indptr included; on such
// an indptr the owners are meaningless, and the fold drops what was concluded from them.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "tg_tcsr.h"

namespace tg {

constexpr int VF_THREADS = 256;
constexpr int VF_ITEMS = 8;
constexpr int VF_TILE = VF_THREADS * VF_ITEMS;  // entries per workgroup
constexpr int VF_WAVES = VF_THREADS / TG_WAVE;
constexpr int VF_WIN = 2048;                    // rows of one tile staged in LDS (more: searched in global memory)
constexpr int VF_REC = 8;                       // words of a partial record
constexpr uint32_t VF_NONE = 0xffffffffu;
constexpr int64_t VF_NONE64 = std::numeric_limits<int64_t>::max();
// orderable(-inf): the maximum over no time at all
constexpr uint64_t VF_KEY_NEG_INF = ~0xfff0000000000000ull;

// record of an entry tile: {kind 0, p0, off TS_ORDER, off TS_NAN, off NBR_RANGE, off EID_RANGE, max key, 0}
// record of a node chunk:  {kind 1, v0, off ENDS, off PTR_ORDER, 0, 0, VF_KEY_NEG_INF, 0}       (off: VF_NONE = clean)

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int o = TG_WAVE / 2; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, TG_WAVE));
  return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = TG_WAVE / 2; o > 0; o >>= 1) v = max(v, (uint64_t)__shfl_xor((long long)v, o, TG_WAVE));
  return v;
}
__device__ __forceinline__ int64_t wave_min_i64(int64_t v) {
#pragma unroll
  for (int o = TG_WAVE / 2; o > 0; o >>= 1) v = min(v, (int64_t)__shfl_xor((long long)v, o, TG_WAVE));
  return v;
}

__global__ void __launch_bounds__(VF_THREADS) k_verify_entries(tg_tcsr g, int64_t eid_rows, uint64_t* __restrict__ rec) {
  __shared__ uint32_t win[VF_WIN];  // indptr[lo + 1 .. hi]: where the rows after the first one of [p0 - 1, p_last] begin
  __shared__ uint32_t s_min[4][VF_WAVES];
  __shared__ uint64_t s_max[VF_WAVES];
  const uint32_t t = threadIdx.x, lane = t & (TG_WAVE - 1), wv = t / TG_WAVE;
  const int64_t N = g.num_node, P = g.num_entry;
  const int64_t p0 = (int64_t)blockIdx.x * VF_TILE, p1 = min(p0 + VF_TILE, P);
  const RowWindow w = row_window<VF_THREADS>(g.indptr, N, max(p0 - 1, (int64_t)0), p1 - 1, win, VF_WIN);
  if (w.staged) __syncthreads();
  uint32_t m_ord = VF_NONE, m_nan = VF_NONE, m_nbr = VF_NONE, m_eid = VF_NONE;
  uint64_t key = VF_KEY_NEG_INF;
#pragma unroll
  for (int i = 0; i < VF_ITEMS; ++i) {
    const uint32_t off = (uint32_t)i * VF_THREADS + t;  // ascending in i: the first hit of a lane is its smallest
    const int64_t p = p0 + off;
    if (p >= p1) break;
    const double x = g.ts[p];
    const double x_front = p > 0 ? g.ts[p - 1] : x;
    const int64_t u = (int64_t)g.nbr[p];
    const int64_t e = (int64_t)((uint32_t)g.eid[p] & 0x7fffffffu);
    if (x != x) m_nan = min(m_nan, off);
    else key = max(key, orderable(x));
    if (u < 0 || u >= N) m_nbr = min(m_nbr, off);
    if (eid_rows >= 0 && e >= eid_rows) m_eid = min(m_eid, off);
    if (x < x_front && w.owner(p) == w.owner(p - 1)) m_ord = min(m_ord, off);  // (x < x_front: p > 0)
  }
  m_ord = wave_min_u32(m_ord);
  m_nan = wave_min_u32(m_nan);
  m_nbr = wave_min_u32(m_nbr);
  m_eid = wave_min_u32(m_eid);
  key = wave_max_u64(key);
  if (lane == 0) {
    s_min[0][wv] = m_ord;
    s_min[1][wv] = m_nan;
    s_min[2][wv] = m_nbr;
    s_min[3][wv] = m_eid;
    s_max[wv] = key;
  }
  __syncthreads();
  if (t == 0) {
    uint64_t* r = rec + (int64_t)blockIdx.x * VF_REC;
    r[0] = 0;
    r[1] = (uint64_t)p0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      uint32_t m = s_min[c][0];
#pragma unroll
      for (int j = 1; j < VF_WAVES; ++j) m = min(m, s_min[c][j]);
      r[2 + c] = m;
    }
    uint64_t k = s_max[0];
#pragma unroll
    for (int j = 1; j < VF_WAVES; ++j) k = max(k, s_max[j]);
    r[6] = k;
    r[7] = 0;
  }
}

// workgroup b: row bounds [256 b, 256 b + 256) of indptr[0 .. num_node]
__global__ void __launch_bounds__(VF_THREADS) k_verify_nodes(tg_tcsr g, uint64_t* __restrict__ rec) {
  __shared__ uint32_t s_min[2][VF_WAVES];
  const uint32_t t = threadIdx.x, lane = t & (TG_WAVE - 1), wv = t / TG_WAVE;
  const int64_t N = g.num_node;
  const int64_t v0 = (int64_t)blockIdx.x * VF_THREADS, v = v0 + t;
  uint32_t m_end = VF_NONE, m_ptr = VF_NONE;
  if (v <= N) {
    const int64_t b = g.indptr[v];
    if ((v == 0 && b != 0) || (v == N && b != g.num_entry)) m_end = t;
    if (v < N && g.indptr[v + 1] < b) m_ptr = t;
  }
  m_end = wave_min_u32(m_end);
  m_ptr = wave_min_u32(m_ptr);
  if (lane == 0) {
    s_min[0][wv] = m_end;
    s_min[1][wv] = m_ptr;
  }
  __syncthreads();
  if (t == 0) {
    uint64_t* r = rec + (int64_t)blockIdx.x * VF_REC;
    r[0] = 1;
    r[1] = (uint64_t)v0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      uint32_t m = s_min[c][0];
#pragma unroll
      for (int j = 1; j < VF_WAVES; ++j) m = min(m, s_min[c][j]);
      r[2 + c] = m;
    }
    r[4] = r[5] = VF_NONE;
    r[6] = VF_KEY_NEG_INF;
    r[7] = 0;
  }
}

// one workgroup over the n_rec partial records
__global__ void __launch_bounds__(VF_THREADS) k_verify_fold(const uint64_t* __restrict__ rec, int64_t n_rec,
                                                            int64_t* __restrict__ out8) {
  __shared__ int64_t s_first[6][VF_WAVES];
  __shared__ uint64_t s_max[VF_WAVES];
  const uint32_t t = threadIdx.x, lane = t & (TG_WAVE - 1), wv = t / TG_WAVE;
  int64_t first[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) first[c] = VF_NONE64;
  uint64_t key = VF_KEY_NEG_INF;
  for (int64_t i = t; i < n_rec; i += VF_THREADS) {
    const uint64_t* r = rec + i * VF_REC;
    const bool nodes = r[0] != 0;  // (block-divergent, but the record's kind is only compared: no address depends on it)
    const int64_t base = (int64_t)r[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint64_t off = r[2 + j];
      if (off == VF_NONE) continue;
      if (nodes && j < 2) first[j] = min(first[j], base + (int64_t)off);
      if (!nodes) first[2 + j] = min(first[2 + j], base + (int64_t)off);
    }
    key = max(key, r[6]);
  }
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const int64_t m = wave_min_i64(first[c]);
    if (lane == 0) s_first[c][wv] = m;
  }
  key = wave_max_u64(key);
  if (lane == 0) s_max[wv] = key;
  __syncthreads();
  if (t == 0) {
    int64_t code = 0;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      int64_t m = s_first[c][0];
#pragma unroll
      for (int j = 1; j < VF_WAVES; ++j) m = min(m, s_first[c][j]);
      first[c] = m == VF_NONE64 ? -1 : m;
    }
    if (first[0] >= 0 || first[1] >= 0) first[2] = -1;  // TS_ORDER needs row bounds
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      if (first[c] >= 0) code |= (int64_t)1 << c;
      out8[1 + c] = first[c];
    }
    uint64_t k = s_max[0];
#pragma unroll
    for (int j = 1; j < VF_WAVES; ++j) k = max(k, s_max[j]);
    out8[0] = code;
    out8[7] = (int64_t)((k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k);  // orderable^-1: the time's bits
  }
}

struct VerifyLayout {
  int64_t n_tile, n_chunk;
  size_t total;
};
static VerifyLayout verify_layout(int64_t num_entry, int64_t num_node) {
  VerifyLayout l{};
  l.n_tile = cdiv(num_entry, VF_TILE);
  l.n_chunk = cdiv(num_node + 1, VF_THREADS);
  l.total = (size_t)(l.n_tile + l.n_chunk) * VF_REC * sizeof(uint64_t);
  return l;
}

}  // namespace tg

using namespace tg;

extern "C" size_t tg_tcsr_verify_workspace_bytes(int64_t num_entry, int64_t num_node) {
  if (num_node <= 0 || num_node > 0x7fffffffLL || num_entry < 0 || num_entry > 0xffffffffLL) return 0;
  return verify_layout(num_entry, num_node).total;
}

extern "C" int tg_tcsr_verify(const tg_tcsr* g, int64_t eid_rows, int64_t* out8, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = tcsr_args(g)) return rc;
  if (!out8) return TG_EINVAL;
  const VerifyLayout l = verify_layout(g->num_entry, g->num_node);
  if (int rc = ws_check(ws, ws_bytes, l.total)) return rc;  // before the first launch
  hipStream_t st = as_stream(stream);
  uint64_t* rec = static_cast<uint64_t*>(ws);
  if (l.n_tile > 0) hipLaunchKernelGGL(k_verify_entries, dim3((unsigned)l.n_tile), dim3(VF_THREADS), 0, st, *g, eid_rows, rec);
  hipLaunchKernelGGL(k_verify_nodes, dim3((unsigned)l.n_chunk), dim3(VF_THREADS), 0, st, *g, rec + l.n_tile * VF_REC);
  hipLaunchKernelGGL(k_verify_fold, dim3(1), dim3(VF_THREADS), 0, st, rec, l.n_tile + l.n_chunk, out8);
  return check_launch("tg_tcsr_verify");
}

// The host twin: plain C++ over host pointers, row by row.  Like the kernels it uses no loaded value as an address: the row
// bounds are walked only once ENDS and PTR_ORDER are clean, when they are known to lie in [0, num_entry].
extern "C" int tg_tcsr_verify_host(const tg_tcsr* g, int64_t eid_rows, int64_t* out8) {
  if (int rc = tcsr_args(g)) return rc;
  if (!out8) return TG_EINVAL;
  const int64_t N = g->num_node, P = g->num_entry;
  int64_t first[6] = {-1, -1, -1, -1, -1, -1};
  if (g->indptr[0] != 0) first[0] = 0;
  else if (g->indptr[N] != P) first[0] = N;
  for (int64_t v = 0; v < N; ++v)
    if (g->indptr[v + 1] < g->indptr[v]) {
      first[1] = v;
      break;
    }
  double t_max = -INFINITY;
  bool pos_zero = false;
  for (int64_t p = 0; p < P; ++p) {
    const double x = g->ts[p];
    if (x != x) {
      if (first[3] < 0) first[3] = p;
    } else {
      if (x > t_max) t_max = x;
      if (x == 0.0 && !std::signbit(x)) pos_zero = true;
    }
    if (first[4] < 0 && (g->nbr[p] < 0 || (int64_t)g->nbr[p] >= N)) first[4] = p;
    if (first[5] < 0 && eid_rows >= 0 && (int64_t)((uint32_t)g->eid[p] & 0x7fffffffu) >= eid_rows) first[5] = p;
  }
  if (t_max == 0.0) t_max = pos_zero ? 0.0 : -0.0;
  if (first[0] < 0 && first[1] < 0)
    for (int64_t v = 0; v < N && first[2] < 0; ++v)
      for (int64_t p = g->indptr[v] + 1; p < g->indptr[v + 1]; ++p)
        if (g->ts[p] < g->ts[p - 1]) {
          first[2] = p;
          break;
        }
  int64_t code = 0;
  for (int c = 0; c < 6; ++c) {
    if (first[c] >= 0) code |= (int64_t)1 << c;
    out8[1 + c] = first[c];
  }
  out8[0] = code;
  std::memcpy(&out8[7], &t_max, sizeof(double));
  return TG_OK;
}
