// Incremental refresh of a catalogue snapshot (TIGE.refresh_catalogue): which rows of a snapshot read a node
// that changed since they were embedded, and the merge of the re-embedded rows into the child snapshot.
//
// tg_catalogue_dirty
//   flags (k_cd_flag_edges / k_cd_flag_nodes, one wavefront per catalogue row): the row's own bit first (no search at all
//          when it is set), then the enumeration of tg_involved_list - the SAME template, tg_involved_visit.h - with a
//          visitor that tests a bit of `touched` per node and leaves the row at the first hit.  One byte per row:
//          bit 0 = reads a touched node, bit 1 = older than max_age.
//   count  (k_cd_count, one workgroup per tile of 2 048 rows): a thread loads its 8 flags as one 8-byte word; the tile's
//          dirty rows and its rows dirty by age alone -> tot_d[tile], tot_a[tile].
//   emit   (k_cd_emit, same tiles): workgroup b sums the totals in front of it (block_sum_front), scans its tile again and
//          writes rank[j] and cols[...]; the last workgroup writes count.
//   No atomics, no workgroup waits for another; workspace = C flag bytes + 8 bytes per tile.
// tg_catalogue_merge (k_cat_merge): G lanes per row (G = the power of two that holds a row's 16-byte words, 8 .. 64); the
//   group reads rank[j] once and moves h, P, nb and t_row of the row from the new or the old table.
// tg_bitmap_mark_degree_diff (k_degree_diff): one wavefront per bitmap word, lane i compares the row lengths of id 64 w + i,
//   the ballot is the word's new bits, lane 0 ORs them in (the word's only writer).
// Integer work and comparisons only: device, host twin and numpy agree bit for bit.
#include <cmath>

#include "tg_involved_visit.h"
#include "tg_tcsr.h"

namespace tg {

constexpr int CD_TILE = 2048;  // rows per scan tile: 8 per thread of a TG_SCAN_BLOCK workgroup
constexpr uint8_t CD_TOUCHED = 1, CD_AGED = 2;

struct DirtyArgs {
  tg_tcsr g;
  int64_t C;
  const int64_t* ids;
  const double* t_row;  // nullable: every row at t_all
  double t_all;
  int K;
  int two;  // second hop wanted
  const uint64_t* touched;
  double t_new, max_age;  // max_age NaN: the comparison below is false for every row
  uint8_t* flags;
};

// the testing visitor of tg_involved_visit.h: a bit per node, stops at the first hit of any lane
struct TouchedTester {
  const uint64_t* bits;
  int64_t n;
  bool hit;
  __device__ __forceinline__ void visit(int64_t v) {
    if (v >= 0 && v < n) hit = hit || bm_test(bits, v);
  }
  __device__ __forceinline__ bool stop() const { return __any(hit); }
};

__device__ __forceinline__ bool dirty_own_bit(const DirtyArgs& a, int64_t nid) {
  return nid >= 0 && nid < a.g.num_node && bm_test(a.touched, nid);
}
__device__ __forceinline__ void dirty_store(const DirtyArgs& a, int64_t j, double t, bool touched, int lane) {
  const bool aged = a.t_new - t > a.max_age;
  if (lane == 0) a.flags[j] = (uint8_t)((touched ? CD_TOUCHED : 0) | (aged ? CD_AGED : 0));
}

template <int G>
__global__ void __launch_bounds__(256) k_cd_flag_edges(DirtyArgs a) {
  const int lane = lane_id();
  for (int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < a.C; j += (int64_t)gridDim.x * 4) {
    const int64_t nid = a.ids[j];
    const double t = a.t_row ? a.t_row[j] : a.t_all;
    bool touched = dirty_own_bit(a, nid);  // (wave-uniform)
    if (!touched) {
      TouchedTester vis{a.touched, a.g.num_node, false};
      involved_visit_edges<G>(a.g, nid, t, a.K, a.two != 0, lane, vis);
      touched = vis.stop();
    }
    dirty_store(a, j, t, touched, lane);
  }
}

__global__ void __launch_bounds__(256) k_cd_flag_nodes(DirtyArgs a) {
  __shared__ int s_new[4][TG_WAVE];
  __shared__ float s_t[4][TG_WAVE];
  const int lane = lane_id(), wv = threadIdx.x >> 6;
  for (int64_t j = (int64_t)blockIdx.x * 4 + wv; j < a.C; j += (int64_t)gridDim.x * 4) {
    const int64_t nid = a.ids[j];
    const double t = a.t_row ? a.t_row[j] : a.t_all;
    bool touched = dirty_own_bit(a, nid);  // (wave-uniform)
    if (!touched) {
      TouchedTester vis{a.touched, a.g.num_node, false};
      involved_visit_nodes(a.g, nid, t, a.K, a.two != 0, lane, s_new[wv], s_t[wv], vis);
      touched = vis.stop();
    }
    dirty_store(a, j, t, touched, lane);
  }
}

struct DirtyScanArgs {
  const uint8_t* flags;  // 16-byte aligned
  int64_t C;
  uint32_t *tot_d, *tot_a;  // [tiles]
  int32_t *rank, *cols, *count;
};

// the 8 flags of rows r0 .. r0 + 7 (r0 a multiple of 8) -> bit i of *dm: row r0 + i is dirty, of *am: dirty by age alone
__device__ __forceinline__ void dirty_masks(const DirtyScanArgs& a, int64_t r0, uint32_t* dm, uint32_t* am) {
  uint64_t w = 0;
  if (r0 + 8 <= a.C) {
    w = *reinterpret_cast<const uint64_t*>(a.flags + r0);
  } else {
    for (int i = 0; i < 8; ++i)
      if (r0 + i < a.C) w |= (uint64_t)a.flags[r0 + i] << (8 * i);
  }
  const uint64_t touched = w & 0x0101010101010101ull, aged = (w >> 1) & 0x0101010101010101ull;
  *dm = (uint32_t)pack8(touched | aged);
  *am = (uint32_t)pack8(aged & ~touched);
}

__global__ void __launch_bounds__(TG_SCAN_BLOCK) k_cd_count(DirtyScanArgs a) {
  __shared__ uint32_t s_w[TG_SCAN_BLOCK / TG_WAVE];
  uint32_t dm, am;
  dirty_masks(a, (int64_t)blockIdx.x * CD_TILE + 8 * (int64_t)threadIdx.x, &dm, &am);
  uint32_t total;  // both counts are at most 2 048: they share one word
  block_excl_scan((uint32_t)__popc(dm) | ((uint32_t)__popc(am) << 16), s_w, &total);
  if (threadIdx.x == 0) {
    a.tot_d[blockIdx.x] = total & 0xffffu;
    a.tot_a[blockIdx.x] = total >> 16;
  }
}

__global__ void __launch_bounds__(TG_SCAN_BLOCK) k_cd_emit(DirtyScanArgs a) {
  __shared__ uint32_t s_w[TG_SCAN_BLOCK / TG_WAVE];
  const uint32_t base = block_sum_front(a.tot_d, blockIdx.x, s_w);  // dirty rows in front of this tile
  const int64_t r0 = (int64_t)blockIdx.x * CD_TILE + 8 * (int64_t)threadIdx.x;
  uint32_t dm, am;
  dirty_masks(a, r0, &dm, &am);
  uint32_t total;
  uint32_t r = base + block_excl_scan((uint32_t)__popc(dm), s_w, &total);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int64_t j = r0 + i;
    if (j >= a.C) break;
    if ((dm >> i) & 1u) {
      a.rank[j] = (int32_t)r;
      a.cols[r] = (int32_t)j;  // r < n_dirty <= C
      ++r;
    } else {
      a.rank[j] = -1;
    }
  }
  if (blockIdx.x == gridDim.x - 1) {  // (block-uniform)
    const uint32_t aged = block_sum_front(a.tot_a, gridDim.x, s_w);
    if (threadIdx.x == 0) {
      a.count[0] = (int32_t)(base + total);
      a.count[1] = (int32_t)aged;
    }
  }
}

static inline size_t sr_align(size_t x) { return (x + 15) & ~(size_t)15; }
struct DirtyLayout {
  size_t flags, tot_d, tot_a, total;
};
static DirtyLayout dirty_layout(int64_t C) {
  const size_t tiles = (size_t)cdiv(C, CD_TILE);
  DirtyLayout l{};
  l.flags = 0;
  l.tot_d = sr_align((size_t)C);
  l.tot_a = l.tot_d + sr_align(tiles * sizeof(uint32_t));
  l.total = l.tot_a + sr_align(tiles * sizeof(uint32_t));
  return l;
}

static int dirty_args(const tg_tcsr* g, int64_t C, const int64_t* ids, double t_all, const double* t_row, int32_t K,
                      int32_t n_layers, int32_t strategy, const uint64_t* touched, double t_new, double max_age,
                      const int32_t* rank, const int32_t* cols, const int32_t* count) {
  if (!g || g->num_node <= 0 || g->num_entry < 0 || C < 0 || C > 0x7fffffffLL) return TG_EINVAL;
  if (K < 1 || K > TG_INVOLVED_MAX_K || (n_layers != 1 && n_layers != 2)) return TG_EINVAL;
  if (strategy < 0 || strategy > 2) return TG_EINVAL;
  if (strategy == 2) return TG_EUNSUPPORTED;
  if (!count || t_new != t_new || (!t_row && t_all != t_all) || max_age < 0.0) return TG_EINVAL;
  if (C == 0) return TG_OK;
  if (!ids || !touched || !rank || !cols || !g->indptr || (g->num_entry > 0 && (!g->ts || !g->nbr))) return TG_EINVAL;
  return TG_OK;
}

// ---- merge ------------------------------------------------------------------------------------------------------------------
struct MergeArgs {
  int64_t C, n_new;
  int d4, K;  // 16-byte words per float row, int64 per nb row
  int lg;     // log2 of the lanes per row
  const int32_t* rank;
  const float4 *h_old, *h_new;
  float4* h_out;
  const float4 *P_old, *P_new;  // nullable (with P_out)
  float4* P_out;
  const int64_t *nb_old, *nb_new;  // nullable (with nb_out)
  int64_t* nb_out;
  const double* t_old;  // nullable: t_old_all
  double t_old_all, t_new;
  double* t_out;
};

__global__ void __launch_bounds__(256) k_cat_merge(MergeArgs a) {
  const int G = 1 << a.lg;
  const int sub = threadIdx.x & (G - 1);
  const int64_t rows_per_pass = ((int64_t)gridDim.x * 256) >> a.lg;
  for (int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> a.lg; j < a.C; j += rows_per_pass) {
    const int64_t r = a.rank[j];
    const bool fresh = r >= 0 && r < a.n_new;
    const int64_t src = fresh ? r : j;
    const float4* h = (fresh ? a.h_new : a.h_old) + src * a.d4;
    for (int u = sub; u < a.d4; u += G) a.h_out[j * a.d4 + u] = h[u];
    if (a.P_out) {
      const float4* P = (fresh ? a.P_new : a.P_old) + src * a.d4;
      for (int u = sub; u < a.d4; u += G) a.P_out[j * a.d4 + u] = P[u];
    }
    if (a.nb_out) {
      const int64_t* nb = (fresh ? a.nb_new : a.nb_old) + src * a.K;
      for (int u = sub; u < a.K; u += G) a.nb_out[j * a.K + u] = nb[u];
    }
    if (sub == 0) a.t_out[j] = fresh ? a.t_new : (a.t_old ? a.t_old[j] : a.t_old_all);
  }
}

static int merge_args(int64_t C, int64_t n_new, int32_t d, int32_t K, const int32_t* rank, const float* h_old,
                      const float* h_new, const float* h_out, const float* P_old, const float* P_new, const float* P_out,
                      const int64_t* nb_old, const int64_t* nb_new, const int64_t* nb_out, const double* t_out) {
  if (C < 0 || C > 0x7fffffffLL || n_new < 0 || n_new > C || d < 4 || d % 4 || K < 0) return TG_EINVAL;
  const int nP = (P_old != nullptr) + (P_new != nullptr) + (P_out != nullptr);
  const int nN = (nb_old != nullptr) + (nb_new != nullptr) + (nb_out != nullptr);
  if (C == 0) return TG_OK;
  // (x_new may be NULL when no row is new, x_old when every row is)
  if (!rank || !h_out || !t_out || (!h_old && n_new < C) || (!h_new && n_new > 0)) return TG_EINVAL;
  if (P_out ? ((!P_old && n_new < C) || (!P_new && n_new > 0)) : nP != 0) return TG_EINVAL;
  if (nb_out ? (K == 0 || (!nb_old && n_new < C) || (!nb_new && n_new > 0)) : nN != 0) return TG_EINVAL;
  for (const void* p : {(const void*)h_old, (const void*)h_new, (const void*)h_out, (const void*)P_old, (const void*)P_new,
                        (const void*)P_out})
    if (reinterpret_cast<uintptr_t>(p) & 15) return TG_EINVAL;
  return TG_OK;
}

// ---- degree difference --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t row_len(const tg_tcsr& g, int64_t v) {
  return v < g.num_node ? g.indptr[v + 1] - g.indptr[v] : 0;
}
__global__ void __launch_bounds__(256) k_degree_diff(tg_tcsr a, tg_tcsr b, uint64_t* bits, int64_t W) {
  const int lane = lane_id();
  for (int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < W; w += (int64_t)gridDim.x * 4) {
    const int64_t v = w * 64 + lane;
    const uint64_t m = __ballot(row_len(a, v) != row_len(b, v));
    if (lane == 0 && m) bits[w] |= m;  // this wavefront is the word's only writer
  }
}

static int degree_diff_args(const tg_tcsr* a, const tg_tcsr* b, const uint64_t* bits, int64_t bit_words) {
  if (!a || !b || !bits || !a->indptr || !b->indptr) return TG_EINVAL;
  if (a->num_node <= 0 || a->num_node > 0x7fffffffLL || b->num_node <= 0 || b->num_node > 0x7fffffffLL) return TG_EINVAL;
  if (bit_words < (std::max(a->num_node, b->num_node) + 63) / 64) return TG_EINVAL;
  return TG_OK;
}

}  // namespace tg

using namespace tg;

extern "C" size_t tg_catalogue_dirty_workspace_bytes(int64_t C) {
  if (C < 0 || C > 0x7fffffffLL) return 0;
  return std::max(dirty_layout(C).total, (size_t)16);
}

extern "C" int tg_catalogue_dirty(const tg_tcsr* g, int64_t C, const int64_t* ids, const double* t_row, double t_all,
                                  int32_t K, int32_t n_layers, int32_t strategy, const uint64_t* touched, double t_new,
                                  double max_age, int32_t* rank, int32_t* cols, int32_t* count, void* ws, size_t ws_bytes,
                                  void* stream) {
  if (int rc = dirty_args(g, C, ids, t_all, t_row, K, n_layers, strategy, touched, t_new, max_age, rank, cols, count))
    return rc;
  hipStream_t st = as_stream(stream);
  if (C == 0) {
    const hipError_t e = hipMemsetAsync(count, 0, 2 * sizeof(int32_t), st);
    if (e != hipSuccess) {
      set_hip_error(e, "tg_catalogue_dirty memset");
      return TG_EHIP;
    }
    return TG_OK;
  }
  const DirtyLayout l = dirty_layout(C);
  if (int rc = ws_check(ws, ws_bytes, l.total)) return rc;
  char* base = static_cast<char*>(ws);
  DirtyArgs a{*g, C, ids, t_row, t_all, K, n_layers == 2 ? 1 : 0, touched, t_new, max_age,
              reinterpret_cast<uint8_t*>(base + l.flags)};
  const dim3 grid(flat_grid(C, 4));
  if (strategy == 1)
    hipLaunchKernelGGL(k_cd_flag_nodes, grid, dim3(256), 0, st, a);
  else if (K <= 16)
    hipLaunchKernelGGL(k_cd_flag_edges<16>, grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(k_cd_flag_edges<64>, grid, dim3(256), 0, st, a);
  if (int rc = check_launch("tg_catalogue_dirty(flags)")) return rc;
  DirtyScanArgs b{a.flags, C, reinterpret_cast<uint32_t*>(base + l.tot_d), reinterpret_cast<uint32_t*>(base + l.tot_a),
                  rank, cols, count};
  const dim3 tiles((unsigned)cdiv(C, CD_TILE));
  hipLaunchKernelGGL(k_cd_count, tiles, dim3(TG_SCAN_BLOCK), 0, st, b);
  hipLaunchKernelGGL(k_cd_emit, tiles, dim3(TG_SCAN_BLOCK), 0, st, b);
  return check_launch("tg_catalogue_dirty(scan)");
}

extern "C" int tg_catalogue_dirty_host(const tg_tcsr* g, int64_t C, const int64_t* ids_host, const double* t_row_host,
                                       double t_all, int32_t K, int32_t n_layers, int32_t strategy,
                                       const uint64_t* touched_host, double t_new, double max_age, int32_t* rank_host,
                                       int32_t* cols_host, int32_t* count_host) {
  if (int rc = dirty_args(g, C, ids_host, t_all, t_row_host, K, n_layers, strategy, touched_host, t_new, max_age, rank_host,
                          cols_host, count_host))
    return rc;
  count_host[0] = count_host[1] = 0;
  for (int64_t j = 0; j < C; ++j)
    if (ids_host[j] < 0 || ids_host[j] >= g->num_node) return TG_EINVAL;
  std::vector<int64_t> hop1, hop2;
  int32_t n = 0, aged_only = 0;
  for (int64_t j = 0; j < C; ++j) {
    const double t = t_row_host ? t_row_host[j] : t_all;
    const bool touched = host_involved_visit(g, ids_host[j], t, K, n_layers, strategy, hop1, hop2, [&](int64_t v) {
      return ((touched_host[v >> 6] >> (v & 63)) & 1ull) != 0;
    });
    const bool aged = t_new - t > max_age;
    if (touched || aged) {
      rank_host[j] = n;
      cols_host[n++] = (int32_t)j;
      aged_only += !touched;
    } else {
      rank_host[j] = -1;
    }
  }
  count_host[0] = n;
  count_host[1] = aged_only;
  return TG_OK;
}

extern "C" int tg_catalogue_merge(int64_t C, int64_t n_new, int32_t d, int32_t K, const int32_t* rank, const float* h_old,
                                  const float* h_new, float* h_out, const float* P_old, const float* P_new, float* P_out,
                                  const int64_t* nb_old, const int64_t* nb_new, int64_t* nb_out, const double* t_old,
                                  double t_old_all, double t_new, double* t_out, void* stream) {
  if (int rc = merge_args(C, n_new, d, K, rank, h_old, h_new, h_out, P_old, P_new, P_out, nb_old, nb_new, nb_out, t_out))
    return rc;
  if (C == 0) return TG_OK;
  const int units = std::max(d / 4, nb_out ? (int)K : 1);
  int lg = 3;
  while (lg < 6 && (1 << lg) < units) ++lg;
  MergeArgs a{C, n_new, d / 4, nb_out ? (int)K : 0, lg, rank,
              reinterpret_cast<const float4*>(h_old), reinterpret_cast<const float4*>(h_new), reinterpret_cast<float4*>(h_out),
              reinterpret_cast<const float4*>(P_old), reinterpret_cast<const float4*>(P_new), reinterpret_cast<float4*>(P_out),
              nb_old, nb_new, nb_out, t_old, t_old_all, t_new, t_out};
  hipLaunchKernelGGL(k_cat_merge, dim3(flat_grid(C << lg, 256)), dim3(256), 0, as_stream(stream), a);
  return check_launch("tg_catalogue_merge");
}

extern "C" int tg_catalogue_merge_host(int64_t C, int64_t n_new, int32_t d, int32_t K, const int32_t* rank, const float* h_old,
                                       const float* h_new, float* h_out, const float* P_old, const float* P_new,
                                       float* P_out, const int64_t* nb_old, const int64_t* nb_new, int64_t* nb_out,
                                       const double* t_old, double t_old_all, double t_new, double* t_out) {
  if (int rc = merge_args(C, n_new, d, K, rank, h_old, h_new, h_out, P_old, P_new, P_out, nb_old, nb_new, nb_out, t_out))
    return rc;
  for (int64_t j = 0; j < C; ++j)
    if (rank[j] >= n_new) return TG_EINVAL;
  for (int64_t j = 0; j < C; ++j) {
    const int64_t r = rank[j];
    const bool fresh = r >= 0;
    const int64_t src = fresh ? r : j;
    std::copy_n((fresh ? h_new : h_old) + src * d, d, h_out + j * d);
    if (P_out) std::copy_n((fresh ? P_new : P_old) + src * d, d, P_out + j * d);
    if (nb_out) std::copy_n((fresh ? nb_new : nb_old) + src * K, K, nb_out + j * K);
    t_out[j] = fresh ? t_new : (t_old ? t_old[j] : t_old_all);
  }
  return TG_OK;
}

extern "C" int tg_bitmap_mark_degree_diff(const tg_tcsr* a, const tg_tcsr* b, uint64_t* bits, int64_t bit_words,
                                          void* stream) {
  if (int rc = degree_diff_args(a, b, bits, bit_words)) return rc;
  const int64_t W = (std::max(a->num_node, b->num_node) + 63) / 64;
  hipLaunchKernelGGL(k_degree_diff, dim3(flat_grid(W, 4)), dim3(256), 0, as_stream(stream), *a, *b, bits, W);
  return check_launch("tg_bitmap_mark_degree_diff");
}

extern "C" int tg_bitmap_mark_degree_diff_host(const tg_tcsr* a, const tg_tcsr* b, uint64_t* bits_host, int64_t bit_words) {
  if (int rc = degree_diff_args(a, b, bits_host, bit_words)) return rc;
  const int64_t N = std::max(a->num_node, b->num_node);
  for (int64_t v = 0; v < N; ++v) {
    const int64_t la = v < a->num_node ? a->indptr[v + 1] - a->indptr[v] : 0;
    const int64_t lb = v < b->num_node ? b->indptr[v + 1] - b->indptr[v] : 0;
    if (la != lb) bits_host[v >> 6] |= 1ull << (v & 63);
  }
  return TG_OK;
}
