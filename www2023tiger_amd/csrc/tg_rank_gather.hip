// Retrieve, then rank on a catalogue snapshot: the score head over B x Cq (source, item) pairs whose items are a PER-QUERY
// subset of a snapshot's C rows (tiger_hip.h: tg_rank_scores_gathered).  col[i, q] names the snapshot row of pair (i, q);
// the items' half of fc1, P [C, d] (tg_rank_cand_half), exists once per item, so a pair costs one gathered P row and the
// O(d) epilogue of tg_rank_scores_shared - nothing is embedded or multiplied per pair ('vec': the 2K hit columns).
// Order contract (inherited): a pair's bits are those tg_rank_scores_shared writes at [i, col[i, q]].  S (source
// half + b1) and T_s / T_d come from the loops of tg_rank_shared.hip, copied here as that unit copied them from tg_rank.hip
// (k_gather_tables = k_shared_tables, k_gather_half = k_half_tile); per hidden column v = P[j, n] + S[i, n] (+ T_s[cs][n] +
// T_d[cd][n]); wavefront slot w and lane fr add relu(v) * fc2.weight[n] over the columns nc + 32 w + fr for nc = 0, 128, ...
// in ascending order, an xor butterfly over fr (16, 8, 4, 2, 1) folds a slot, ((R0 + R1) + (R2 + R3)) + b2 folds the slots.
//   'none' / 'bin' / 'count' (k_gather_pairs): items are not shared between sources, so a 256-thread block owns ONE source
//   and a strip of 32 of its columns: 32 threads read col and count the classes of the strip once, then the strip runs in
//   chunks of 16 without a barrier - the fk halves of a wavefront take alternate items of a chunk (item 2 jj + fk), a
//   thread keeps 8 partial sums - and one barrier stands before the 32 stores.  S[i, n] and fc2.weight[n] are read once per column pass; an item's P row is
//   read as 128 consecutive floats per pass (32 per wavefront), so a gathered row is fully coalesced.
//   'vec' (k_gather_vec): k_shared_vec's 32-pair-row MFMA tile with pair p = i Cq + q; the accumulators are preloaded from
//   P[col], the hit operand columns come from nbr_src[i], nbr_cat[col] and cat_ids[col].
// A pair with col < 0 computes on row 0 and stores 0.0f.  col >= C is the caller's error and is not checked.
#include <cmath>

#include "tg_mfma.h"

namespace tg {

constexpr int GA_BM = 32;   // rows of an MFMA tile (sources of the half product, pair rows of 'vec')
constexpr int GA_BN = 128;  // hidden columns of a column pass (4 wavefronts x 32)
constexpr int GA_TJ = 8;    // items of a chunk per fk half: their partial sums live in registers
constexpr int GA_CH = 16;   // items of a chunk (item 2 jj + fk)
constexpr int GA_JS = 32;   // columns of a block's strip (2 chunks)

struct GatherArgs {
  int64_t B, C, Cq, ld;
  int d, K, W;  // hidden width; neighbours; operand width of one side (fc1 is [d, 2W])
  int hit_type, n_hit_rows;
  const float *w1, *b1, *w2, *b2;
  const float *P, *srow, *tab_s, *tab_d;
  const int64_t *nbr_src, *nbr_cat, *src, *cat;
  const int32_t* col;
  float* scores;
};

// T_s / T_d as k_shared_tables (tg_rank_shared.hip) forms them: the same loop, so the same bits
__global__ void k_gather_tables(int n_hit_rows, int d, int W, const float* __restrict__ w1, const float* __restrict__ emb,
                                float* __restrict__ tab_s, float* __restrict__ tab_d) {
  const int total = n_hit_rows * d;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    const int c = t / d, n = t - c * d;
    const float* w = w1 + (int64_t)n * 2 * W;
    const float* e = emb + (int64_t)c * d;
    float s = 0.f, q = 0.f;
    for (int k = 0; k < d; ++k) {
      s += w[k] * e[k];
      q += w[W + k] * e[k];
    }
    tab_s[t] = s;
    tab_d[t] = q;
  }
}

// out[r, n] = sum_k w1[n, k] h[r, k] + bias[n]: k_half_tile (tg_rank_shared.hip) on the source block of fc1 - accumulator
// from 0, k ascending, two per MFMA
__global__ void __launch_bounds__(256) k_gather_half(int64_t R, int d, int ldw, const float* __restrict__ h,
                                                     const float* __restrict__ w1, const float* __restrict__ bias,
                                                     float* __restrict__ out) {
  __shared__ float As[GA_BM][LDK];
  __shared__ float Bs[GA_BN][LDK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fk = lane >> 5;
  const int64_t m0 = (int64_t)blockIdx.x * GA_BM;
  const int sr = tid >> 3, sk = (tid & 7) * 4;  // staging: 8 threads per 32-float row, 4 consecutive k each
  const float* arow = h + min(m0 + sr, R - 1) * d;  // rows past the end repeat the last one; they are never stored
  const int nkt = (d + BK - 1) / BK;
  for (int nc = 0; nc < d; nc += GA_BN) {
    const bool live = nc + wave * 32 < d;  // wave-uniform
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int kt = 0; kt < nkt; ++kt) {
      __syncthreads();  // the previous tile has been read
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = kt * BK + sk + e;
        As[sr][sk + e] = k < d ? arow[k] : 0.f;
      }
#pragma unroll
      for (int rr = 0; rr < GA_BN / 32; ++rr) {
        const int n = nc + sr + 32 * rr;
        const float* wrow = w1 + (int64_t)min(n, d - 1) * ldw;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = kt * BK + sk + e;
          Bs[sr + 32 * rr][sk + e] = (n < d && k < d) ? wrow[k] : 0.f;
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
    const int n = nc + wave * 32 + fr;
    if (live && n < d) {
      const float b = bias[n];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * fk;
        if (m0 + row < R) out[(m0 + row) * d + n] = acc[r] + b;
      }
    }
  }
}

// C = 0: every column is "not in the catalogue"
__global__ void k_gather_zero(int64_t B, int64_t Cq, int64_t ld, float* __restrict__ scores) {
  const int64_t total = B * Cq;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x)
    scores[(t / Cq) * ld + t % Cq] = 0.f;
}

// 'none' / 'bin' / 'count'.  EMB: class tables are added.
template <bool EMB>
__global__ void __launch_bounds__(256) k_gather_pairs(GatherArgs a) {
  __shared__ float red[4][GA_JS];
  __shared__ int2 off[GA_JS];  // (class of the src hits, class of the dst hits) * d per pair of the strip
  __shared__ int jrow[GA_JS];  // the strip's snapshot rows as read from col (negative: not in the catalogue)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fk = lane >> 5;
  const int d = a.d, K = a.K;
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
      const int64_t s = a.src[i], c = a.cat[j];
      int cs = 0, cd = 0;
      for (int k = 0; k < K; ++k) {
        cs += a.nbr_cat[j * K + k] == s ? 1 : 0;  // the source among the item's neighbours (src hits)
        cd += a.nbr_src[i * K + k] == c ? 1 : 0;  // the item among the source's neighbours (dst hits)
      }
      if (a.hit_type == TG_HIT_BIN) {
        cs = cs > 0;
        cd = cd > 0;
      }
      off[tid] = make_int2(min(cs, a.n_hit_rows - 1) * d, min(cd, a.n_hit_rows - 1) * d);
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
    for (int nc = 0; nc < d; nc += GA_BN) {
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
    // the 32 lanes of one fk half hold the columns of the same pairs; every lane takes part in every shuffle
#pragma unroll
    for (int jj = 0; jj < GA_TJ; ++jj) {
      float v = part[jj];
#pragma unroll
      for (int x = 16; x >= 1; x >>= 1) v += __shfl_xor(v, x);
      if (fr == 0) red[wave][c0 + 2 * jj + fk] = v;
    }
  }
  __syncthreads();
  if (tid < ns)
    a.scores[i * a.ld + qs + tid] = jrow[tid] < 0 ? 0.f : ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) + a.b2[0];
}

// 'vec': 32 pair rows (pair p = i Cq + q) per block; accumulators from P[col], operand columns = [dst hits | src hits]
__global__ void __launch_bounds__(256) k_gather_vec(GatherArgs a) {
  __shared__ float As[GA_BM][LDK];
  __shared__ float Bs[GA_BN][LDK];
  __shared__ float red[4][GA_BM];
  __shared__ int ev_i[GA_BM], ev_j[GA_BM], ev_c[GA_BM];  // source, snapshot row (clamped), col as read
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fk = lane >> 5;
  const int d = a.d, K = a.K, W = a.W, KX = 2 * a.K;
  const int64_t NP = a.B * a.Cq;
  const int64_t m0 = (int64_t)blockIdx.x * GA_BM;
  if (tid < GA_BM) {
    const int64_t p = min(m0 + tid, NP - 1);  // rows past the end repeat the last one; they are never stored
    const int jc = a.col[p];
    ev_i[tid] = (int)(p / a.Cq);
    ev_c[tid] = jc;
    ev_j[tid] = max(jc, 0);
  }
  const int sr = tid >> 3, sk = (tid & 7) * 4;
  const int64_t ap = min(m0 + sr, NP - 1);
  const int64_t ai = ap / a.Cq, aj = max(a.col[ap], 0);
  const int64_t a_src = a.src[ai], a_cat = a.cat[aj];
  float part[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) part[r] = 0.f;
  __syncthreads();  // ev_i / ev_j are written
  const int nkt = (KX + BK - 1) / BK;
  for (int nc = 0; nc < d; nc += GA_BN) {
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
      for (int e = 0; e < 4; ++e) {
        const int k = kt * BK + sk + e;
        float v = 0.f;
        if (k < K) {
          v = a.nbr_src[ai * K + k] == a_cat ? 1.f : 0.f;
        } else if (k < KX) {
          v = a.nbr_cat[aj * K + (k - K)] == a_src ? 1.f : 0.f;
        }
        As[sr][sk + e] = v;
      }
#pragma unroll
      for (int rr = 0; rr < GA_BN / 32; ++rr) {
        const int nw = nc + sr + 32 * rr;
        const float* wrow = a.w1 + (int64_t)min(nw, d - 1) * 2 * W;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = kt * BK + sk + e;
          float v = 0.f;
          if (nw < d && k < KX) v = k < K ? wrow[W + d + k] : wrow[d + (k - K)];
          Bs[sr + 32 * rr][sk + e] = v;
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
  for (int r = 0; r < 16; ++r) {
    float v = part[r];
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    if (fr == 0) red[wave][(r & 3) + 8 * (r >> 2) + 4 * fk] = v;
  }
  __syncthreads();
  if (tid < GA_BM && m0 + tid < NP) {
    const int64_t p = m0 + tid;
    a.scores[(int64_t)ev_i[tid] * a.ld + (p - (int64_t)ev_i[tid] * a.Cq)] =
        ev_c[tid] < 0 ? 0.f : ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) + a.b2[0];
  }
}

static bool gather_params_ok(const tg_score_params* sp, int32_t K) {
  if (!sp || !sp->fc1.w || !sp->fc1.b || !sp->fc2.w || !sp->fc2.b) return false;
  if (sp->hit_type < TG_HIT_NONE || sp->hit_type > TG_HIT_COUNT) return false;
  const bool emb = sp->hit_type == TG_HIT_BIN || sp->hit_type == TG_HIT_COUNT;
  if (emb && (!sp->hit_emb || sp->n_hit_rows < (sp->hit_type == TG_HIT_BIN ? 2 : K + 1))) return false;
  return true;
}

}  // namespace tg

using namespace tg;

extern "C" size_t tg_rank_scores_gathered_workspace_bytes(int64_t B, int32_t d, const tg_score_params* sp) {
  return tg_rank_scores_shared_workspace_bytes(B, d, sp);  // S [B, d] and the two class tables, as there
}

extern "C" int tg_rank_scores_gathered(int64_t B, int64_t C, int64_t Cq, int32_t d, int32_t K, const tg_score_params* sp,
                                       const float* h_src, const float* P, const int64_t* nbr_src, const int64_t* nbr_cat,
                                       const int64_t* src, const int64_t* cat_ids, const int32_t* col, float* scores,
                                       int64_t ld, void* ws, size_t ws_bytes, void* stream) {
  if (B < 0 || C < 0 || C >= 0x7fffffffLL || Cq < 0 || d <= 0 || K < 0 || !gather_params_ok(sp, K)) return TG_EINVAL;
  if (B > 0 && Cq > 0 && Cq > 0x7fffffffLL / B) return TG_EINVAL;  // B Cq < 2^31
  if (ld < Cq) return TG_EINVAL;
  if (sp->hit_type == TG_HIT_VEC && ((d & 1) || (2 * (d + K)) % 4)) return TG_EUNSUPPORTED;
  if (B == 0 || Cq == 0) return TG_OK;
  if (!col || !scores) return TG_EINVAL;
  hipStream_t st = as_stream(stream);
  if (C == 0) {  // no row to gather: every col is negative
    hipLaunchKernelGGL(k_gather_zero, dim3(flat_grid(B * Cq, 256)), dim3(256), 0, st, B, Cq, ld, scores);
    return check_launch("tg_rank_scores_gathered(empty catalogue)");
  }
  if (!h_src || !P || !ws) return TG_EINVAL;
  const bool hits = sp->hit_type != TG_HIT_NONE;
  if (hits && (K <= 0 || !nbr_src || !nbr_cat || !src || !cat_ids)) return TG_EINVAL;
  if (ws_bytes < tg_rank_scores_gathered_workspace_bytes(B, d, sp)) return TG_EINVAL;
  const bool emb = sp->hit_type == TG_HIT_BIN || sp->hit_type == TG_HIT_COUNT;
  GatherArgs a{};
  a.B = B; a.C = C; a.Cq = Cq; a.ld = ld;
  a.d = d; a.K = K;
  a.W = d + (sp->hit_type == TG_HIT_VEC ? K : 0);
  a.hit_type = sp->hit_type;
  a.n_hit_rows = emb ? sp->n_hit_rows : 0;
  a.w1 = sp->fc1.w; a.b1 = sp->fc1.b; a.w2 = sp->fc2.w; a.b2 = sp->fc2.b;
  float* srow = static_cast<float*>(ws);
  float* tab_s = srow + B * d;
  float* tab_d = tab_s + (int64_t)a.n_hit_rows * d;
  a.P = P; a.srow = srow; a.tab_s = tab_s; a.tab_d = tab_d;
  a.nbr_src = nbr_src; a.nbr_cat = nbr_cat; a.src = src; a.cat = cat_ids;
  a.col = col;
  a.scores = scores;
  if (emb) {
    hipLaunchKernelGGL(k_gather_tables, dim3(flat_grid((int64_t)a.n_hit_rows * d, 256)), dim3(256), 0, st, a.n_hit_rows, (int)d,
                       a.W, a.w1, sp->hit_emb, tab_s, tab_d);
    if (int rc = check_launch("tg_rank_scores_gathered(tables)")) return rc;
  }
  hipLaunchKernelGGL(k_gather_half, dim3((unsigned)cdiv(B, GA_BM)), dim3(256), 0, st, B, (int)d, 2 * a.W, h_src, a.w1, a.b1,
                     srow);
  if (int rc = check_launch("tg_rank_scores_gathered(source half)")) return rc;
  if (sp->hit_type == TG_HIT_VEC) {
    hipLaunchKernelGGL(k_gather_vec, dim3((unsigned)cdiv(B * Cq, GA_BM)), dim3(256), 0, st, a);
  } else {
    const unsigned grid = (unsigned)(B * cdiv(Cq, GA_JS));
    if (emb)
      hipLaunchKernelGGL(k_gather_pairs<true>, dim3(grid), dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL(k_gather_pairs<false>, dim3(grid), dim3(256), 0, st, a);
  }
  return check_launch("tg_rank_scores_gathered");
}
