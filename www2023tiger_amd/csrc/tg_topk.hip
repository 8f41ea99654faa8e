// Top-k recommendation: per-row top-k selection over a [B, C] score matrix, and the seen-item filter over the T-CSR.
// No reference counterpart (the reference scores one negative per event); the leave-out rules are tg_rank_stats's.
//
// tg_topk_rows.  The order is TOTAL: a column left in is the 64-bit key
//   (order-preserving bits of its float32 score, -0.0 folded onto +0.0) << 32 | ~column
// so a larger key is a better column - higher score first, equal scores by ascending column - and no two columns of a
// row share a key.  Key 0 is "nothing": a finite score's ordered bits are never 0.  One wavefront per (row, segment of
// columns) keeps its best 64 keys sorted across the lanes, lane p the p-th best.  A step loads TK_U x 64 columns
// coalesced and builds their keys (left-out columns: 0); a ballot finds the lanes whose key beats the current k-th, and
// only those are inserted, one cross-lane shift each.  Once the list has warmed up insertions are rare (about
// k ln(C / k) over a row of random scores), so the pass is one streaming read of the scores, ids and mask.  A row of
// ascending scores inserts every column: correct, and slow.
// With n_seg > 1 every segment leaves its best k keys in the workspace and a second launch merges a row's n_seg * k keys
// with the same insertion.  The top k of a union is the top k of the union of the parts' top k, and the order is total,
// so the result does not depend on n_seg - nor on which lane met which column.  Integer work and comparisons only:
// device, host twin and a sort agree bit for bit.
//
// tg_seen_mask.  One wavefront per event searches the source's time-sorted entries for the prefix before the event's
// time (tg_sample.h: prefix_end_group, the sampler's strict float64 cut) and clears the mask byte of every neighbour of
// that prefix that has a column in the catalogue.
#include <algorithm>
#include <cmath>
#include <vector>

#include "tg_sample.h"
#include "tg_topk_keys.h"

namespace tg {

constexpr int TK_U = 4;    // 64-column chunks in flight per step
constexpr int TK_WPB = 4;  // wavefronts of a workgroup

__host__ __device__ __forceinline__ bool topk_left_in(const int64_t* cand, const uint8_t* mask, int64_t j) {
  return cand[j] != 0 && (!mask || mask[j]);
}

struct TopkArgs {
  int64_t B, C, ld, seg_len;
  int k, n_seg, shared;
  const float* scores;
  const int64_t* cand;
  const uint8_t* mask;
  int64_t* out_ids;
  float* out_scores;
  int32_t* out_cols;
  int32_t* n_valid;
  int64_t* n_nonfinite;
  uint64_t* ws_keys;  // [B, n_seg, k]
  int32_t* ws_cnt;    // [B, n_seg, 2]: columns left in, non-finite scores met
};

__device__ __forceinline__ void topk_finish(const TopkArgs& a, int64_t row, uint64_t best, int nv, int bad, int lane) {
  if (lane < a.k) {
    int64_t id = 0;
    float s = -INFINITY;
    int32_t col = -1;
    if (best) {
      col = (int32_t)~(uint32_t)best;
      id = a.cand[(a.shared ? 0 : row * a.C) + col];
      s = a.scores[row * a.ld + col];  // the stored bits (the key has lost the sign of a zero)
    }
    a.out_ids[row * a.k + lane] = id;
    a.out_scores[row * a.k + lane] = s;
    a.out_cols[row * a.k + lane] = col;
  }
  if (lane == 0) {
    a.n_valid[row] = nv;
    if (bad) atomicAdd(reinterpret_cast<unsigned long long*>(a.n_nonfinite), (unsigned long long)bad);
  }
}

__global__ void __launch_bounds__(TK_WPB * TG_WAVE) k_topk_segments(TopkArgs a) {
  const int lane = lane_id();
  const int64_t w = (int64_t)blockIdx.x * TK_WPB + threadIdx.x / TG_WAVE;
  if (w >= a.B * a.n_seg) return;  // wave-uniform
  const int64_t row = w / a.n_seg;
  const int64_t seg = w - row * a.n_seg;
  const int64_t c_lo = min(a.C, seg * a.seg_len), c_hi = min(a.C, c_lo + a.seg_len);
  const float* srow = a.scores + row * a.ld;
  const int64_t* crow = a.cand + (a.shared ? 0 : row * a.C);
  const uint8_t* mrow = a.mask ? a.mask + row * a.C : nullptr;
  uint64_t best = 0;
  int nv = 0, bad = 0;
  for (int64_t c0 = c_lo; c0 < c_hi; c0 += TK_U * TG_WAVE) {
    uint64_t key[TK_U];
#pragma unroll
    for (int u = 0; u < TK_U; ++u) {
      const int64_t col = c0 + u * TG_WAVE + lane;
      bool in = false, fin = false;
      uint32_t s = 0;
      if (col < c_hi) {
        s = __float_as_uint(srow[col]);
        in = topk_left_in(crow, mrow, col);
        fin = topk_finite(s);
      }
      key[u] = (in && fin) ? topk_key(s, (uint32_t)col) : 0ull;
      nv += __popcll(__ballot(in && fin));
      bad += __popcll(__ballot(in && !fin));
    }
#pragma unroll
    for (int u = 0; u < TK_U; ++u) topk_insert(best, key[u], a.k - 1, lane);
  }
  if (a.n_seg == 1) {
    topk_finish(a, row, best, nv, bad, lane);
    return;
  }
  if (lane < a.k) a.ws_keys[w * a.k + lane] = best;
  if (lane == 0) {
    a.ws_cnt[2 * w] = nv;
    a.ws_cnt[2 * w + 1] = bad;
  }
}

__global__ void __launch_bounds__(TK_WPB * TG_WAVE) k_topk_merge(TopkArgs a) {
  const int lane = lane_id();
  const int64_t row = (int64_t)blockIdx.x * TK_WPB + threadIdx.x / TG_WAVE;
  if (row >= a.B) return;  // wave-uniform
  const int64_t n = (int64_t)a.n_seg * a.k;
  const uint64_t* keys = a.ws_keys + row * n;
  uint64_t best = 0;
  for (int64_t i0 = 0; i0 < n; i0 += TK_U * TG_WAVE) {
    uint64_t key[TK_U];
#pragma unroll
    for (int u = 0; u < TK_U; ++u) {
      const int64_t i = i0 + u * TG_WAVE + lane;
      key[u] = i < n ? keys[i] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < TK_U; ++u) topk_insert(best, key[u], a.k - 1, lane);
  }
  int nv = 0, bad = 0;
  for (int64_t s = lane; s < a.n_seg; s += TG_WAVE) {
    nv += a.ws_cnt[2 * (row * a.n_seg + s)];
    bad += a.ws_cnt[2 * (row * a.n_seg + s) + 1];
  }
  for (int off = TG_WAVE / 2; off >= 1; off >>= 1) {
    nv += __shfl_xor(nv, off);
    bad += __shfl_xor(bad, off);
  }
  topk_finish(a, row, best, nv, bad, lane);
}

// segments chosen by the library: enough wavefronts to fill the chip (16 per CU), at least 256 columns each, and no
// more than sqrt(C / k) - beyond that the merging wavefront of a row reads more keys than a segment reads columns
static int64_t topk_choose_segs(int64_t B, int64_t C, int32_t k) {
  if (B <= 0 || C <= 0) return 1;
  int64_t n = 4096 / B;
  n = std::min(n, C / 256);
  n = std::min(n, (int64_t)std::sqrt((double)C / (double)k));
  return std::max<int64_t>(n, 1);
}

static bool topk_args_ok(int64_t B, int64_t C, int32_t k, int64_t ld, int32_t n_seg) {
  if (k < 1 || k > TG_TOPK_MAX_K || B < 0 || C < 0 || C > 0x7fffffffLL || ld < C || n_seg < 0) return false;
  if (B > 0 && std::max<int64_t>(n_seg, 1) > 0x7fffffffLL / B) return false;  // B * n_seg wavefronts in one grid
  return true;
}

static int64_t topk_segs(int64_t B, int64_t C, int32_t k, int32_t n_seg) {
  return (B == 0 || C == 0) ? 1 : (n_seg > 0 ? (int64_t)n_seg : topk_choose_segs(B, C, k));
}

// ---- seen-item filter ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_seen_mask(tg_tcsr g, int64_t B, const int64_t* __restrict__ src,
                                                   const double* __restrict__ ts, int64_t C,
                                                   const int32_t* __restrict__ col_of, uint8_t* __restrict__ mask) {
  const int lane = lane_id();
  const int64_t wpb = blockDim.x / TG_WAVE;
  for (int64_t i = (int64_t)blockIdx.x * wpb + threadIdx.x / TG_WAVE; i < B; i += (int64_t)gridDim.x * wpb) {
    int64_t start;
    const int64_t end = prefix_end_group<64>(g, src[i], ts[i], &start, lane);  // entries [start, end): ts < ts[i]
    for (int64_t e = start + lane; e < end; e += TG_WAVE) {
      const int64_t nb = g.nbr[e];
      if (nb < 0 || nb >= g.num_node) continue;
      const int64_t c = col_of[nb];
      if (c >= 0 && c < C) mask[i * C + c] = 0;  // lanes clearing the same byte write the same value
    }
  }
}

}  // namespace tg

using namespace tg;

extern "C" size_t tg_topk_rows_workspace_bytes(int64_t B, int64_t C, int32_t k, int32_t n_seg) {
  if (!topk_args_ok(B, C, k, C, n_seg)) return 0;
  const int64_t ns = topk_segs(B, C, k, n_seg);
  return ns == 1 ? 0 : (size_t)B * (size_t)ns * ((size_t)k * sizeof(uint64_t) + 2 * sizeof(int32_t));
}

extern "C" int tg_topk_rows(int64_t B, int64_t C, int32_t k, const float* scores, int64_t ld, const int64_t* cand_ids,
                            int32_t cand_shared, const uint8_t* mask, int32_t n_seg, int64_t* out_ids, float* out_scores,
                            int32_t* out_cols, int32_t* n_valid, int64_t* n_nonfinite, void* ws, size_t ws_bytes,
                            void* stream) {
  if (!topk_args_ok(B, C, k, ld, n_seg)) return TG_EINVAL;
  if (B == 0) return TG_OK;
  if (!out_ids || !out_scores || !out_cols || !n_valid || !n_nonfinite || (C > 0 && (!scores || !cand_ids))) return TG_EINVAL;
  const int64_t ns = topk_segs(B, C, k, n_seg);
  const size_t need = tg_topk_rows_workspace_bytes(B, C, k, n_seg);
  if (need && (!ws || ws_bytes < need)) return TG_EWORKSPACE;
  if (need && (reinterpret_cast<uintptr_t>(ws) & 7)) return TG_EINVAL;
  hipStream_t st = as_stream(stream);
  TopkArgs a{};
  a.B = B; a.C = C; a.ld = ld;
  a.seg_len = cdiv(std::max<int64_t>(C, 1), ns);
  a.k = k; a.n_seg = (int)ns; a.shared = cand_shared != 0;
  a.scores = scores; a.cand = cand_ids; a.mask = mask;
  a.out_ids = out_ids; a.out_scores = out_scores; a.out_cols = out_cols; a.n_valid = n_valid; a.n_nonfinite = n_nonfinite;
  a.ws_keys = static_cast<uint64_t*>(ws);
  a.ws_cnt = reinterpret_cast<int32_t*>(a.ws_keys + B * ns * k);
  hipLaunchKernelGGL(k_topk_segments, dim3((unsigned)cdiv(B * ns, TK_WPB)), dim3(TK_WPB * TG_WAVE), 0, st, a);
  if (ns == 1) return check_launch("tg_topk_rows");
  if (int rc = check_launch("tg_topk_rows(segments)")) return rc;
  hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)cdiv(B, TK_WPB)), dim3(TK_WPB * TG_WAVE), 0, st, a);
  return check_launch("tg_topk_rows(merge)");
}

extern "C" int tg_topk_rows_host(int64_t B, int64_t C, int32_t k, const float* scores_host, int64_t ld,
                                 const int64_t* cand_ids_host, int32_t cand_shared, const uint8_t* mask_host, int32_t n_seg,
                                 int64_t* out_ids_host, float* out_scores_host, int32_t* out_cols_host, int32_t* n_valid_host,
                                 int64_t* n_nonfinite_host) {
  if (!topk_args_ok(B, C, k, ld, n_seg)) return TG_EINVAL;
  if (B == 0) return TG_OK;
  if (!out_ids_host || !out_scores_host || !out_cols_host || !n_valid_host || !n_nonfinite_host ||
      (C > 0 && (!scores_host || !cand_ids_host)))
    return TG_EINVAL;
  std::vector<uint64_t> keys;
  for (int64_t i = 0; i < B; ++i) {
    const float* srow = scores_host + i * ld;
    const int64_t* crow = cand_ids_host + (cand_shared ? 0 : i * C);
    const uint8_t* mrow = mask_host ? mask_host + i * C : nullptr;
    keys.clear();
    int64_t bad = 0;
    for (int64_t j = 0; j < C; ++j) {
      if (!topk_left_in(crow, mrow, j)) continue;
      const uint32_t u = __builtin_bit_cast(uint32_t, srow[j]);
      if (topk_finite(u))
        keys.push_back(topk_key(u, (uint32_t)j));
      else
        ++bad;
    }
    const size_t top = std::min<size_t>((size_t)k, keys.size());
    std::partial_sort(keys.begin(), keys.begin() + top, keys.end(), [](uint64_t x, uint64_t y) { return x > y; });
    for (int32_t p = 0; p < k; ++p) {
      const bool live = (size_t)p < top;
      const int32_t col = live ? (int32_t)~(uint32_t)keys[p] : -1;
      out_ids_host[i * k + p] = live ? crow[col] : 0;
      out_scores_host[i * k + p] = live ? srow[col] : -INFINITY;
      out_cols_host[i * k + p] = col;
    }
    n_valid_host[i] = (int32_t)keys.size();
    *n_nonfinite_host += bad;
  }
  return TG_OK;
}

static bool seen_args_ok(const tg_tcsr* g, int64_t B, int64_t C) {
  return g && g->num_node > 0 && g->num_entry >= 0 && B >= 0 && C >= 0;
}

extern "C" int tg_seen_mask(const tg_tcsr* g, int64_t B, const int64_t* src, const double* ts, int64_t C,
                            const int32_t* col_of, uint8_t* mask, void* stream) {
  if (!seen_args_ok(g, B, C)) return TG_EINVAL;
  if (B == 0 || C == 0 || g->num_entry == 0) return TG_OK;
  if (!src || !ts || !col_of || !mask || !g->indptr || !g->ts || !g->nbr) return TG_EINVAL;
  hipLaunchKernelGGL(k_seen_mask, dim3(flat_grid(B, 4)), dim3(256), 0, as_stream(stream), *g, B, src, ts, C, col_of, mask);
  return check_launch("tg_seen_mask");
}

extern "C" int tg_seen_mask_host(const tg_tcsr* g, int64_t B, const int64_t* src_host, const double* ts_host, int64_t C,
                                 const int32_t* col_of_host, uint8_t* mask_host) {
  if (!seen_args_ok(g, B, C)) return TG_EINVAL;
  if (B == 0) return TG_OK;
  if (!src_host || !ts_host) return TG_EINVAL;
  for (int64_t i = 0; i < B; ++i)
    if (src_host[i] < 0 || src_host[i] >= g->num_node) return TG_EINVAL;
  if (C == 0 || g->num_entry == 0) return TG_OK;
  if (!col_of_host || !mask_host || !g->indptr || !g->ts || !g->nbr) return TG_EINVAL;
  for (int64_t i = 0; i < B; ++i) {
    const int64_t start = g->indptr[src_host[i]];
    const int64_t end = std::lower_bound(g->ts + start, g->ts + g->indptr[src_host[i] + 1], ts_host[i]) - g->ts;  // ts < t
    for (int64_t e = start; e < end; ++e) {
      const int64_t nb = g->nbr[e];
      if (nb < 0 || nb >= g->num_node) continue;
      const int64_t c = col_of_host[nb];
      if (c >= 0 && c < C) mask_host[i * C + c] = 0;
    }
  }
  return TG_OK;
}
