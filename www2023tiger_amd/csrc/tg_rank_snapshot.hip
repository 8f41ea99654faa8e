// Catalogue snapshots: the score head (tg_rank_head.h) over (source, item) pairs whose items are rows of one snapshot.
// tg_rank_scores (tg_rank.hip) repeats the item half W1[:, W:W+d] y per pair row; on a snapshot that half is a function of
// the item alone and exists once per item:
//   tg_rank_cand_half         P[j, :] = W1[:, W:W+d] h_cat[j]      one 32-row MFMA tile pass over the C items (k_head_half)
//   tg_rank_scores_shared     B x C pairs: every source against every row of the snapshot
//   tg_rank_scores_gathered   B x Cq pairs: col[i, q] names the snapshot row of pair (i, q), a PER-QUERY subset
// Both score forms take S (source half + b1) and T_s / T_d from the kernels tg_rank_scores takes them from, then per pair
// v_n = P[j, n] + S[i, n] (+ T_s[cs][n] + T_d[cd][n]), relu, * fc2.weight, summed - O(d) VALU work, nothing embedded.
// Order contract: a pair's bits equal tg_rank_scores's on the broadcast inputs, and the gathered form's
// equal what the shared form writes at [i, col[i, q]].  P is k_rank_tile's accumulator after its first d operand columns
// (an accumulator stored as f32 and loaded again continues the chain exactly), and the sum over the hidden columns is taken
// as that kernel's epilogue takes it, through the same fold_slot / head_score.
//   'none' / 'bin' / 'count', shared (k_shared_pairs): a 256-thread block owns 16 sources and a strip of 64 items; thread
//   (wavefront w, lane fr, half fk) owns hidden column nc + 32 w + fr of the sources 2 ii + fk.  It holds the P values of
//   8 items in registers, reads one S value per 8 pairs and keeps an 8 x 8 tile of partial sums.
//   'none' / 'bin' / 'count', gathered (k_gather_pairs): items are not shared between sources, so a 256-thread block owns
//   ONE source and a strip of 32 of its columns: 32 threads read col and count the classes of the strip once, then the strip
//   runs in chunks of 16 without a barrier - the fk halves of a wavefront take alternate items of a chunk (item 2 jj + fk),
//   a thread keeps 8 partial sums - and one barrier stands before the 32 stores.  S[i, n] and fc2.weight[n] are read once
//   per column pass; an item's P row is read as 128 consecutive floats per pass, so a gathered row is fully coalesced.
//   'vec' (k_snap_vec<COL>): the 2K hit columns of a pair still go through fc1, so the pair rows (pair p = i Cq + q) take
//   k_rank_tile's tile with the accumulators preloaded from P and only the hit operand columns multiplied.  d must be even:
//   an odd d would split one two-column MFMA between P and the hits.
// Gathered: a pair with col < 0 computes on row 0 and stores 0.0f.  col >= C is the caller's error and is not checked.
#include <cmath>

#include "tg_rank_head.h"

namespace tg {

constexpr int SH_TI = 16;  // sources of a shared pair block: 8 per half wavefront, interleaved (source 2 ii + fk)
constexpr int SH_TJ = 8;   // items of a chunk: their P values live in registers
constexpr int SH_JS = 64;  // items of a block's strip (8 chunks)
constexpr int GA_TJ = 8;   // items of a gathered chunk per fk half: their partial sums live in registers
constexpr int GA_CH = 16;  // items of a chunk (item 2 jj + fk)
constexpr int GA_JS = 32;  // columns of a block's strip (2 chunks)

// 'none' / 'bin' / 'count', shared.  EMB: class tables are added.
template <bool EMB>
__global__ void __launch_bounds__(256) k_shared_pairs(HeadArgs a) {
  __shared__ float red[4][SH_TI * SH_TJ];
  __shared__ int2 off[SH_TI * SH_TJ];  // (class of the src hits, class of the dst hits) * d per pair of the chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fk = lane >> 5;
  const int d = a.d;
  const int64_t nbj = (a.C + SH_JS - 1) / SH_JS;
  const int64_t i0 = (int64_t)(blockIdx.x / nbj) * SH_TI, js = (int64_t)(blockIdx.x % nbj) * SH_JS;
  const int64_t je = min(a.C, js + SH_JS);
  const int nii = ((int)min((int64_t)SH_TI, a.B - i0) + 1) / 2;  // rows of the 8 x 8 tile with a live source in either half
  // the pair this thread classifies and stores (tid < 128): source tid / 8, item tid % 8 of the chunk
  const int pl = tid >> 3, pj = tid & 7;
  for (int64_t j0 = js; j0 < je; j0 += SH_TJ) {
    const int nj = (int)min((int64_t)SH_TJ, je - j0);
    if (EMB) {
      if (tid < SH_TI * SH_TJ) {
        const int64_t i = min(i0 + pl, a.B - 1), j = min(j0 + pj, a.C - 1);  // pairs past the end repeat; never stored
        off[tid] = hit_class_off(a, i, j);
      }
      __syncthreads();
    }
    float part[SH_TI / 2][SH_TJ];
#pragma unroll
    for (int ii = 0; ii < SH_TI / 2; ++ii)
#pragma unroll
      for (int jj = 0; jj < SH_TJ; ++jj) part[ii][jj] = 0.f;
    for (int nc = 0; nc < d; nc += RH_BN) {
      if (nc + wave * 32 >= d) break;  // wave-uniform: no hidden column of this pass (nor of a later one)
      const int n = nc + wave * 32 + fr;
      const bool on = n < d;
      const int nn = min(n, d - 1);
      const float w2 = a.w2[nn];
      float p[SH_TJ];
#pragma unroll
      for (int jj = 0; jj < SH_TJ; ++jj) p[jj] = a.P[min(j0 + jj, a.C - 1) * d + nn];
#pragma unroll
      for (int ii = 0; ii < SH_TI / 2; ++ii) {
        if (ii < nii) {  // block-uniform
          const float s = a.srow[min(i0 + 2 * ii + fk, a.B - 1) * d + nn];
#pragma unroll
          for (int jj = 0; jj < SH_TJ; ++jj) {
            if (jj < nj) {  // block-uniform
              float v = p[jj] + s;
              if (EMB) {
                const int2 o = off[(2 * ii + fk) * SH_TJ + jj];
                v += a.tab_s[o.x + nn] + a.tab_d[o.y + nn];
              }
              if (on) part[ii][jj] += fmaxf(v, 0.f) * w2;  // a column >= d adds nothing
            }
          }
        }
      }
    }
#pragma unroll
    for (int ii = 0; ii < SH_TI / 2; ++ii) {
      if (ii < nii) {
#pragma unroll
        for (int jj = 0; jj < SH_TJ; ++jj) {
          if (jj < nj) fold_slot(part[ii][jj], fr, &red[wave][(2 * ii + fk) * SH_TJ + jj]);
        }
      }
    }
    __syncthreads();
    if (tid < SH_TI * SH_TJ && i0 + pl < a.B && pj < nj) a.scores[(i0 + pl) * a.ld + j0 + pj] = head_score(red, tid, a.b2);
    __syncthreads();  // red and off are free for the next chunk
  }
}

// gathered, C = 0: every column is "not in the catalogue"
__global__ void k_gather_zero(int64_t B, int64_t Cq, int64_t ld, float* __restrict__ scores) {
  const int64_t total = B * Cq;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x)
    scores[(t / Cq) * ld + t % Cq] = 0.f;
}

// 'none' / 'bin' / 'count', gathered.  EMB: class tables are added.
template <bool EMB>
__global__ void __launch_bounds__(256) k_gather_pairs(HeadArgs a) {
  __shared__ float red[4][GA_JS];
  __shared__ int2 off[GA_JS];  // (class of the src hits, class of the dst hits) * d per pair of the strip
  __shared__ int jrow[GA_JS];  // the strip's snapshot rows as read from col (negative: not in the catalogue)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fk = lane >> 5;
  const int d = a.d;
  const int64_t nbq = (a.Cq + GA_JS - 1) / GA_JS;
  const int64_t i = blockIdx.x / nbq, qs = (int64_t)(blockIdx.x % nbq) * GA_JS;
  const int ns = (int)min((int64_t)GA_JS, a.Cq - qs);  // live columns of the strip
  const float* srow = a.srow + i * d;
  if (tid < GA_JS) {  // the pair this thread classifies and stores: column qs + tid.  Once per strip: the chunks below
                      // do not wait for another round trip through col, cat_ids and nbr_cat
    const int jc = a.col[i * a.Cq + min(qs + tid, a.Cq - 1)];  // columns past the end repeat the last; never stored
    jrow[tid] = jc;
    if (EMB) {
      const int64_t j = max(jc, 0);
      off[tid] = hit_class_off(a, i, j);
    }
  }
  __syncthreads();
  for (int c0 = 0; c0 < ns; c0 += GA_CH) {
    const int nq = min(GA_CH, ns - c0);
    const int njj = (nq - fk + 1) / 2;  // items of this half: 2 jj + fk < nq
    const float* prow[GA_TJ];
    int2 o[GA_TJ];
#pragma unroll
    for (int jj = 0; jj < GA_TJ; ++jj) {
      prow[jj] = a.P + (int64_t)max(jrow[c0 + 2 * jj + fk], 0) * d;
      if (EMB) o[jj] = off[c0 + 2 * jj + fk];
    }
    float part[GA_TJ];
#pragma unroll
    for (int jj = 0; jj < GA_TJ; ++jj) part[jj] = 0.f;
    for (int nc = 0; nc < d; nc += RH_BN) {
      if (nc + wave * 32 >= d) break;  // wave-uniform: no hidden column of this pass (nor of a later one)
      const int n = nc + wave * 32 + fr;
      const bool on = n < d;
      const int nn = min(n, d - 1);
      const float w2 = a.w2[nn];
      const float s = srow[nn];
#pragma unroll
      for (int jj = 0; jj < GA_TJ; ++jj) {
        if (jj < njj) {  // uniform over the 32 lanes of a half
          float v = prow[jj][nn] + s;
          if (EMB) v += a.tab_s[o[jj].x + nn] + a.tab_d[o[jj].y + nn];
          if (on) part[jj] += fmaxf(v, 0.f) * w2;  // a column >= d adds nothing
        }
      }
    }
    // every lane takes part in every shuffle
#pragma unroll
    for (int jj = 0; jj < GA_TJ; ++jj) fold_slot(part[jj], fr, &red[wave][c0 + 2 * jj + fk]);
  }
  __syncthreads();
  if (tid < ns) a.scores[i * a.ld + qs + tid] = jrow[tid] < 0 ? 0.f : head_score(red, tid, a.b2);
}

// 'vec': 32 pair rows (pair p = i Cq + q) per block; accumulators from P, operand columns = [dst hits | src hits].
// COL: the pair's snapshot row is col[p] (negative: computes on row 0, stores 0.0f); else it is q.
template <bool COL>
__global__ void __launch_bounds__(256) k_snap_vec(HeadArgs a) {
  __shared__ float As[RH_BM][LDK];
  __shared__ float Bs[RH_BN][LDK];
  __shared__ float red[4][RH_BM];
  __shared__ int ev_i[RH_BM], ev_j[RH_BM], ev_c[COL ? RH_BM : 1];  // source, snapshot row (clamped), col as read
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fk = lane >> 5;
  const int d = a.d, K = a.K, W = a.W, KX = 2 * a.K;
  const int64_t NP = a.B * a.Cq;
  const int64_t m0 = (int64_t)blockIdx.x * RH_BM;
  if (tid < RH_BM) {
    const int64_t p = min(m0 + tid, NP - 1);  // rows past the end repeat the last one; they are never stored
    ev_i[tid] = (int)(p / a.Cq);
    if (COL) {
      const int jc = a.col[p];
      ev_c[tid] = jc;
      ev_j[tid] = max(jc, 0);
    } else {
      ev_j[tid] = (int)(p % a.Cq);
    }
  }
  const int sr = tid >> 3, sk = (tid & 7) * 4;
  const int64_t ap = min(m0 + sr, NP - 1);
  const int64_t ai = ap / a.Cq, aj = COL ? max(a.col[ap], 0) : ap % a.Cq;
  const int64_t a_src = a.src[ai], a_cat = a.item[aj];
  float part[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) part[r] = 0.f;
  __syncthreads();  // ev_i / ev_j are written
  const int nkt = (KX + BK - 1) / BK;
  for (int nc = 0; nc < d; nc += RH_BN) {
    const bool live = nc + wave * 32 < d;  // wave-uniform
    const int n = nc + wave * 32 + fr;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * fk;
      acc[r] = (live && n < d) ? a.P[(int64_t)ev_j[row] * d + n] : 0.f;
    }
    for (int kt = 0; kt < nkt; ++kt) {
      __syncthreads();  // the previous tile has been read
#pragma unroll
      for (int e = 0; e < 4; ++e)
        As[sr][sk + e] = hit_operand(kt * BK + sk + e, K, a.nbr_src + ai * K, a.nbr_item + aj * K, a_src, a_cat);
#pragma unroll
      for (int rr = 0; rr < RH_BN / 32; ++rr) {
        const int nw = nc + sr + 32 * rr;
        const float* wrow = a.w1 + (int64_t)min(nw, d - 1) * 2 * W;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = kt * BK + sk + e;
          Bs[sr + 32 * rr][sk + e] = (nw < d && k < KX) ? pair_weight(wrow, d + k, W, d) : 0.f;
        }
      }
      __syncthreads();
      if (live) {
        const float* pa = &As[fr][fk];
        const float* pb = &Bs[wave * 32 + fr][fk];
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * s], pb[2 * s], acc, 0, 0, 0);
      }
    }
    if (live && n < d) {
      const float w2 = a.w2[n];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * fk;
        const float v = acc[r] + a.srow[(int64_t)ev_i[row] * d + n];
        part[r] += fmaxf(v, 0.f) * w2;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) fold_slot(part[r], fr, &red[wave][(r & 3) + 8 * (r >> 2) + 4 * fk]);
  __syncthreads();
  if (tid < RH_BM && m0 + tid < NP) {
    const int64_t i = ev_i[tid];
    a.scores[i * a.ld + (m0 + tid - i * a.Cq)] = (COL && ev_c[tid] < 0) ? 0.f : head_score(red, tid, a.b2);
  }
}

static bool snap_vec_unsupported(const tg_score_params* sp, int32_t d, int32_t K) {
  return sp->hit_type == TG_HIT_VEC && ((d & 1) || (2 * (d + K)) % 4);
}

// what both score forms check once their own shapes and outputs are in order
static bool snap_inputs_ok(int64_t B, int32_t d, int32_t K, const tg_score_params* sp, const float* h_src, const float* P,
                           const int64_t* nbr_src, const int64_t* nbr_cat, const int64_t* src, const int64_t* cat_ids,
                           const void* ws, size_t ws_bytes) {
  if (!h_src || !P || !ws) return false;
  if (sp->hit_type != TG_HIT_NONE && (K <= 0 || !nbr_src || !nbr_cat || !src || !cat_ids)) return false;
  return ws_bytes >= head_workspace_bytes(B, d, sp);
}

}  // namespace tg

using namespace tg;

extern "C" int tg_rank_cand_half(int64_t C, int32_t d, int32_t K, const tg_score_params* sp, const float* h_cat, float* P,
                                 void* stream) {
  if (C < 0 || C >= 0x7fffffffLL || d <= 0 || K < 0 || !head_params_ok(sp, K)) return TG_EINVAL;
  if (snap_vec_unsupported(sp, d, K)) return TG_EUNSUPPORTED;
  if (C == 0) return TG_OK;
  if (!h_cat || !P) return TG_EINVAL;
  const int W = d + (sp->hit_type == TG_HIT_VEC ? K : 0);
  return head_half(C, d, 2 * W, W, h_cat, sp->fc1.w, nullptr, P, as_stream(stream), "tg_rank_cand_half");
}

extern "C" size_t tg_rank_scores_shared_workspace_bytes(int64_t B, int32_t d, const tg_score_params* sp) {
  return head_workspace_bytes(B, d, sp);
}

extern "C" size_t tg_rank_scores_gathered_workspace_bytes(int64_t B, int32_t d, const tg_score_params* sp) {
  return head_workspace_bytes(B, d, sp);  // S [B, d] and the two class tables, as there
}

// C == Cq and col == nullptr: the shared form.  Both forms: T_s / T_d, S, then the pair kernel of the hit type.
static int snap_scores(int64_t B, int64_t C, int64_t Cq, int32_t d, int32_t K, const tg_score_params* sp, const float* h_src,
                       const float* P, const int64_t* nbr_src, const int64_t* nbr_cat, const int64_t* src,
                       const int64_t* cat_ids, const int32_t* col, float* scores, int64_t ld, void* ws, hipStream_t st,
                       const char* what_tables, const char* what_half, const char* what) {
  HeadArgs a{};
  head_fill(a, B, d, K, sp, nbr_src, nbr_cat, src, cat_ids, scores, ws);
  a.C = C; a.Cq = Cq; a.ld = ld;
  a.P = P;
  a.col = col;
  const bool emb = head_emb(sp);
  if (emb)
    if (int rc = head_tables(a, sp->hit_emb, st, what_tables)) return rc;
  if (int rc = head_half(B, d, 2 * a.W, 0, h_src, a.w1, a.b1, a.srow, st, what_half)) return rc;
  const dim3 vgrid((unsigned)cdiv(B * Cq, RH_BM)), block(256);
  if (col) {
    const dim3 grid((unsigned)(B * cdiv(Cq, GA_JS)));
    if (sp->hit_type == TG_HIT_VEC)
      hipLaunchKernelGGL(k_snap_vec<true>, vgrid, block, 0, st, a);
    else if (emb)
      hipLaunchKernelGGL(k_gather_pairs<true>, grid, block, 0, st, a);
    else
      hipLaunchKernelGGL(k_gather_pairs<false>, grid, block, 0, st, a);
  } else {
    const dim3 grid((unsigned)(cdiv(B, SH_TI) * cdiv(C, SH_JS)));
    if (sp->hit_type == TG_HIT_VEC)
      hipLaunchKernelGGL(k_snap_vec<false>, vgrid, block, 0, st, a);
    else if (emb)
      hipLaunchKernelGGL(k_shared_pairs<true>, grid, block, 0, st, a);
    else
      hipLaunchKernelGGL(k_shared_pairs<false>, grid, block, 0, st, a);
  }
  return check_launch(what);
}

extern "C" int tg_rank_scores_shared(int64_t B, int64_t C, int32_t d, int32_t K, const tg_score_params* sp,
                                     const float* h_src, const float* P, const int64_t* nbr_src, const int64_t* nbr_cat,
                                     const int64_t* src, const int64_t* cat_ids, float* scores, int64_t ld, void* ws,
                                     size_t ws_bytes, void* stream) {
  if (B < 0 || C < 0 || d <= 0 || K < 0 || !head_params_ok(sp, K)) return TG_EINVAL;
  if (B > 0 && C > 0 && C > 0x7fffffffLL / B) return TG_EINVAL;  // B C < 2^31
  if (ld < C) return TG_EINVAL;
  if (snap_vec_unsupported(sp, d, K)) return TG_EUNSUPPORTED;
  if (B == 0 || C == 0) return TG_OK;
  if (!scores || !snap_inputs_ok(B, d, K, sp, h_src, P, nbr_src, nbr_cat, src, cat_ids, ws, ws_bytes)) return TG_EINVAL;
  return snap_scores(B, C, C, d, K, sp, h_src, P, nbr_src, nbr_cat, src, cat_ids, nullptr, scores, ld, ws, as_stream(stream),
                     "tg_rank_scores_shared(tables)", "tg_rank_scores_shared(source half)", "tg_rank_scores_shared");
}

extern "C" int tg_rank_scores_gathered(int64_t B, int64_t C, int64_t Cq, int32_t d, int32_t K, const tg_score_params* sp,
                                       const float* h_src, const float* P, const int64_t* nbr_src, const int64_t* nbr_cat,
                                       const int64_t* src, const int64_t* cat_ids, const int32_t* col, float* scores,
                                       int64_t ld, void* ws, size_t ws_bytes, void* stream) {
  if (B < 0 || C < 0 || C >= 0x7fffffffLL || Cq < 0 || d <= 0 || K < 0 || !head_params_ok(sp, K)) return TG_EINVAL;
  if (B > 0 && Cq > 0 && Cq > 0x7fffffffLL / B) return TG_EINVAL;  // B Cq < 2^31
  if (ld < Cq) return TG_EINVAL;
  if (snap_vec_unsupported(sp, d, K)) return TG_EUNSUPPORTED;
  if (B == 0 || Cq == 0) return TG_OK;
  if (!col || !scores) return TG_EINVAL;
  hipStream_t st = as_stream(stream);
  if (C == 0) {  // no row to gather: every col is negative
    hipLaunchKernelGGL(k_gather_zero, dim3(flat_grid(B * Cq, 256)), dim3(256), 0, st, B, Cq, ld, scores);
    return check_launch("tg_rank_scores_gathered(empty catalogue)");
  }
  if (!snap_inputs_ok(B, d, K, sp, h_src, P, nbr_src, nbr_cat, src, cat_ids, ws, ws_bytes)) return TG_EINVAL;
  return snap_scores(B, C, Cq, d, K, sp, h_src, P, nbr_src, nbr_cat, src, cat_ids, col, scores, ld, ws, st,
                     "tg_rank_scores_gathered(tables)", "tg_rank_scores_gathered(source half)", "tg_rank_scores_gathered");
}
