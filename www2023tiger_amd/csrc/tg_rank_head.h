// The score head score(i, j) = fc2(relu(fc1([xp | yp]))), fc1 = [d, 2W], as the rank units evaluate it (tg_rank.hip: one
// row per (source, candidate) pair; tg_rank_snapshot.hip: a catalogue snapshot, shared by all sources or gathered per
// query).  fc1's product is split by operand:
//   source half   S[i, :] = W1[:, :d] x_i + b1                             (head_half, wofs = 0)
//   item half     P[j, :] = W1[:, W:W+d] y_j                               (head_half, wofs = W; per pair row in tg_rank.hip)
//   hit classes   T_s[c, :] = W1[:, :W] e(c), T_d[c, :] = W1[:, W:] e(c)   ('bin' / 'count': n_hit_rows rows each, head_tables)
//   hit columns   'vec': the K hit columns of either side as 2K more operand columns [dst hits | src hits]
// Order contract: a pair's bits are the same through every entry point.  It holds because every piece
// of the chain is defined once, here: per hidden column v = P[j, n] + S[i, n] (+ T_s[cs][n] + T_d[cd][n]); wavefront slot w
// and lane fr add relu(v) * fc2.weight[n] over the columns nc + 32 w + fr for nc = 0, 128, ... in ascending order,
// fold_slot folds a slot, head_score folds the slots.  The two kernels live in tg_rank.hip (the build has no relocatable
// device code) and are reached through the host launchers below.  Included by the rank units only.
#pragma once
#include "tg_mfma.h"

namespace tg {

constexpr int RH_BM = 32;   // rows of an MFMA tile
constexpr int RH_BN = 128;  // hidden columns of a column pass (4 wavefronts x 32)

// The arguments of a pair kernel.  item = snapshot row: P, nbr_item and item have C rows; Cq pairs per source (shared form:
// Cq = C, col unset).  tg_rank.hip derives its own struct (item = candidate, one row per pair) and leaves C .. ld, P and col
// unset.  The order is k_gather_pairs's need: what a block reads first stands in the first 64 bytes, one scalar load.
struct HeadArgs {
  int64_t B, C, Cq, ld;
  int d, K, W;  // hidden width; neighbours; operand width of one side
  int hit_type, n_hit_rows;
  const float *w1, *b1, *w2, *b2;
  const float* P;
  float *srow, *tab_s, *tab_d;  // S | T_s | T_d: the workspace, in this order
  const int64_t *nbr_src, *nbr_item, *src, *item;
  const int32_t* col;
  float* scores;
};

static inline bool head_emb(const tg_score_params* sp) { return sp->hit_type == TG_HIT_BIN || sp->hit_type == TG_HIT_COUNT; }

static inline bool head_params_ok(const tg_score_params* sp, int32_t K) {
  if (!sp || !sp->fc1.w || !sp->fc1.b || !sp->fc2.w || !sp->fc2.b) return false;
  if (sp->hit_type < TG_HIT_NONE || sp->hit_type > TG_HIT_COUNT) return false;
  if (head_emb(sp) && (!sp->hit_emb || sp->n_hit_rows < (sp->hit_type == TG_HIT_BIN ? 2 : K + 1))) return false;
  return true;
}

static inline size_t head_workspace_bytes(int64_t B, int32_t d, const tg_score_params* sp) {
  if (B < 0 || d <= 0 || !sp) return 0;
  const int64_t rows = B + (head_emb(sp) ? 2 * (int64_t)sp->n_hit_rows : 0);
  return (size_t)(rows * d) * sizeof(float) + 16;
}

static inline void head_fill(HeadArgs& a, int64_t B, int32_t d, int32_t K, const tg_score_params* sp, const int64_t* nbr_src,
                             const int64_t* nbr_item, const int64_t* src, const int64_t* item, float* scores, void* ws) {
  a.B = B;
  a.d = d;
  a.K = K;
  a.W = d + (sp->hit_type == TG_HIT_VEC ? K : 0);
  a.hit_type = sp->hit_type;
  a.n_hit_rows = head_emb(sp) ? sp->n_hit_rows : 0;
  a.w1 = sp->fc1.w; a.b1 = sp->fc1.b; a.w2 = sp->fc2.w; a.b2 = sp->fc2.b;
  a.srow = static_cast<float*>(ws);
  a.tab_s = a.srow + B * d;
  a.tab_d = a.tab_s + (int64_t)a.n_hit_rows * d;
  a.nbr_src = nbr_src; a.nbr_item = nbr_item; a.src = src; a.item = item;
  a.scores = scores;
}

// T_s / T_d of a filled HeadArgs ('bin' / 'count'); one launch
int head_tables(const HeadArgs& a, const float* emb, hipStream_t st, const char* what);
// out[r, n] = sum_k w1[n, wofs + k] h[r, k] (+ bias[n], may be null) over R rows, w1 rows ldw apart; one launch
int head_half(int64_t R, int d, int ldw, int wofs, const float* h, const float* w1, const float* bias, float* out,
              hipStream_t st, const char* what);

// (class of the src hits, class of the dst hits) * d of the pair (source row i, item row j of the id and neighbour arrays)
__device__ __forceinline__ int2 hit_class_off(const HeadArgs& a, int64_t i, int64_t j) {
  const int64_t s = a.src[i], c = a.item[j];
  const int K = a.K;
  int cs = 0, cd = 0;
  for (int k = 0; k < K; ++k) {
    cs += a.nbr_item[j * K + k] == s ? 1 : 0;  // the source among the item's neighbours (src hits)
    cd += a.nbr_src[i * K + k] == c ? 1 : 0;   // the item among the source's neighbours (dst hits)
  }
  if (a.hit_type == TG_HIT_BIN) {
    cs = cs > 0;
    cd = cd > 0;
  }
  return make_int2(min(cs, a.n_hit_rows - 1) * a.d, min(cd, a.n_hit_rows - 1) * a.d);
}

// 'vec': operand column k of the pair's 2K one-hot hit columns [dst hits | src hits]; 0 past them
__device__ __forceinline__ float hit_operand(int k, int K, const int64_t* ns, const int64_t* nc, int64_t s, int64_t c) {
  if (k < K) return ns[k] == c ? 1.f : 0.f;
  if (k < 2 * K) return nc[k - K] == s ? 1.f : 0.f;
  return 0.f;
}

// fc1's weight of operand column k of a pair row [y | dst hits | src hits] in the row wrow of hidden column n: W1[n, W:]
// holds the first two in place, the src hits stand in W1[n, d:W].  The 'vec' hit columns alone are k = d ... d + 2K - 1.
__device__ __forceinline__ float pair_weight(const float* wrow, int k, int W, int d) {
  return k < W ? wrow[W + k] : wrow[d + (k - W)];
}

// a slot's sum: an xor butterfly over the 32 lanes of one fk half, which hold the columns of the same pair
__device__ __forceinline__ void fold_slot(float v, int fr, float* slot) {
#pragma unroll
  for (int off = 16; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  if (fr == 0) *slot = v;
}

template <int N>
__device__ __forceinline__ float head_score(const float (&red)[4][N], int t, const float* b2) {
  return ((red[0][t] + red[1][t]) + (red[2][t] + red[3][t])) + b2[0];
}

}  // namespace tg
