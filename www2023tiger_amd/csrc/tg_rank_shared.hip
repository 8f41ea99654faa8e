// Catalogue snapshots: the score head over B x C (source, item) pairs whose C items are the SAME for every source.
// tg_rank_scores (tg_rank.hip) splits fc1 by operand and repeats the candidate half W1[:, W:W+d] y per pair row; with a
// shared catalogue that half is a function of the item alone:
//   tg_rank_cand_half       P[j, :] = W1[:, W:W+d] h_cat[j]       one 32-row MFMA tile pass over the C items (k_half_tile)
//   tg_rank_scores_shared   S (source half + b1) and T_s / T_d as tg_rank_scores computes them, then per pair
//                           v_n = P[j, n] + S[i, n] (+ T_s[cs][n] + T_d[cd][n]), relu, * fc2.weight, summed - O(d) VALU work.
// Order contract: a pair's bits equal tg_rank_scores's on the broadcast inputs.  P is k_rank_tile<false>'s
// accumulator after its first d operand columns (the chain starts from 0 and takes the columns in ascending order, two
// per v_mfma_f32_32x32x2_f32; an accumulator stored as f32 and loaded again continues the chain exactly), and the sum over
// the hidden columns is taken as that kernel's epilogue takes it: wavefront slot w and lane fr add the terms of columns
// nc + 32 w + fr for nc = 0, 128, ... in ascending order, an xor butterfly over fr (16, 8, 4, 2, 1) folds a slot,
// ((R0 + R1) + (R2 + R3)) + b2 folds the slots.
//   'none' / 'bin' / 'count' (k_shared_pairs): no matrix product is left.  A 256-thread block owns 16 sources and a strip of
//   64 items; thread (wavefront w, lane fr, half fk) owns hidden column nc + 32 w + fr of the sources 2 ii + fk.  It holds
//   the P values of 8 items in registers, reads one S value per 8 pairs and keeps an 8 x 8 tile of partial sums.
//   'vec' (k_shared_vec): the 2K hit columns of a pair still go through fc1, so the pair rows take k_rank_tile<false>'s
//   tile with the accumulators preloaded from P and only the hit operand columns multiplied.  d must be even: an odd d
//   would split one two-column MFMA between P and the hits.
#include <cmath>

#include "tg_mfma.h"

namespace tg {

constexpr int SH_BM = 32;   // rows of an MFMA tile (items / sources of a half product, pair rows of 'vec')
constexpr int SH_BN = 128;  // hidden columns of a column pass (4 wavefronts x 32)
constexpr int SH_TI = 16;   // sources of a pair block: 8 per half wavefront, interleaved (source 2 ii + fk)
constexpr int SH_TJ = 8;    // items of a chunk: their P values live in registers
constexpr int SH_JS = 64;   // items of a block's strip (8 chunks)

struct SharedArgs {
  int64_t B, C, ld;
  int d, K, W;  // hidden width; neighbours; operand width of one side (fc1 is [d, 2W])
  int hit_type, n_hit_rows;
  const float *w1, *b1, *w2, *b2;
  const float *P, *srow, *tab_s, *tab_d;
  const int64_t *nbr_src, *nbr_cat, *src, *cat;
  float* scores;
};

// T_s / T_d as k_rank_tables (tg_rank.hip) forms them: the same loop, so the same bits
__global__ void k_shared_tables(int n_hit_rows, int d, int W, const float* __restrict__ w1, const float* __restrict__ emb,
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

// out[r, n] = sum_k w1[n, wofs + k] h[r, k] (+ bias[n]): k_rank_tile<true>'s tile on either weight block.  The chain per
// output is the one k_rank_tile runs over an operand's first d columns: accumulator from 0, k ascending, two per MFMA.
__global__ void __launch_bounds__(256) k_half_tile(int64_t R, int d, int ldw, int wofs, const float* __restrict__ h,
                                                   const float* __restrict__ w1, const float* __restrict__ bias,
                                                   float* __restrict__ out) {
  __shared__ float As[SH_BM][LDK];
  __shared__ float Bs[SH_BN][LDK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fk = lane >> 5;
  const int64_t m0 = (int64_t)blockIdx.x * SH_BM;
  const int sr = tid >> 3, sk = (tid & 7) * 4;  // staging: 8 threads per 32-float row, 4 consecutive k each
  const float* arow = h + min(m0 + sr, R - 1) * d;  // rows past the end repeat the last one; they are never stored
  const int nkt = (d + BK - 1) / BK;
  for (int nc = 0; nc < d; nc += SH_BN) {
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
      for (int rr = 0; rr < SH_BN / 32; ++rr) {
        const int n = nc + sr + 32 * rr;
        const float* wrow = w1 + (int64_t)min(n, d - 1) * ldw + wofs;
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
      const float b = bias ? bias[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * fk;
        if (m0 + row < R) out[(m0 + row) * d + n] = bias ? acc[r] + b : acc[r];
      }
    }
  }
}

// 'none' / 'bin' / 'count'.  EMB: class tables are added.
template <bool EMB>
__global__ void __launch_bounds__(256) k_shared_pairs(SharedArgs a) {
  __shared__ float red[4][SH_TI * SH_TJ];
  __shared__ int2 off[SH_TI * SH_TJ];  // (class of the src hits, class of the dst hits) * d per pair of the chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fk = lane >> 5;
  const int d = a.d, K = a.K;
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
      __syncthreads();
    }
    float part[SH_TI / 2][SH_TJ];
#pragma unroll
    for (int ii = 0; ii < SH_TI / 2; ++ii)
#pragma unroll
      for (int jj = 0; jj < SH_TJ; ++jj) part[ii][jj] = 0.f;
    for (int nc = 0; nc < d; nc += SH_BN) {
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
    // the 32 lanes of one fk half hold the columns of the same pairs
#pragma unroll
    for (int ii = 0; ii < SH_TI / 2; ++ii) {
      if (ii < nii) {
#pragma unroll
        for (int jj = 0; jj < SH_TJ; ++jj) {
          if (jj < nj) {
            float v = part[ii][jj];
#pragma unroll
            for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o);
            if (fr == 0) red[wave][(2 * ii + fk) * SH_TJ + jj] = v;
          }
        }
      }
    }
    __syncthreads();
    if (tid < SH_TI * SH_TJ && i0 + pl < a.B && pj < nj)
      a.scores[(i0 + pl) * a.ld + j0 + pj] = ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) + a.b2[0];
    __syncthreads();  // red and off are free for the next chunk
  }
}

// 'vec': 32 pair rows (pair p = i C + j) per block; accumulators from P, operand columns = [dst hits | src hits]
__global__ void __launch_bounds__(256) k_shared_vec(SharedArgs a) {
  __shared__ float As[SH_BM][LDK];
  __shared__ float Bs[SH_BN][LDK];
  __shared__ float red[4][SH_BM];
  __shared__ int ev_i[SH_BM], ev_j[SH_BM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fk = lane >> 5;
  const int d = a.d, K = a.K, W = a.W, KX = 2 * a.K;
  const int64_t NP = a.B * a.C;
  const int64_t m0 = (int64_t)blockIdx.x * SH_BM;
  if (tid < SH_BM) {
    const int64_t p = min(m0 + tid, NP - 1);  // rows past the end repeat the last one; they are never stored
    ev_i[tid] = (int)(p / a.C);
    ev_j[tid] = (int)(p % a.C);
  }
  const int sr = tid >> 3, sk = (tid & 7) * 4;
  const int64_t ap = min(m0 + sr, NP - 1);
  const int64_t ai = ap / a.C, aj = ap % a.C;
  const int64_t a_src = a.src[ai], a_cat = a.cat[aj];
  float part[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) part[r] = 0.f;
  __syncthreads();  // ev_i / ev_j are written
  const int nkt = (KX + BK - 1) / BK;
  for (int nc = 0; nc < d; nc += SH_BN) {
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
      for (int rr = 0; rr < SH_BN / 32; ++rr) {
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
  if (tid < SH_BM && m0 + tid < NP)
    a.scores[(int64_t)ev_i[tid] * a.ld + ev_j[tid]] = ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) + a.b2[0];
}

static bool shared_params_ok(const tg_score_params* sp, int32_t K) {
  if (!sp || !sp->fc1.w || !sp->fc1.b || !sp->fc2.w || !sp->fc2.b) return false;
  if (sp->hit_type < TG_HIT_NONE || sp->hit_type > TG_HIT_COUNT) return false;
  const bool emb = sp->hit_type == TG_HIT_BIN || sp->hit_type == TG_HIT_COUNT;
  if (emb && (!sp->hit_emb || sp->n_hit_rows < (sp->hit_type == TG_HIT_BIN ? 2 : K + 1))) return false;
  return true;
}

static bool shared_vec_unsupported(const tg_score_params* sp, int32_t d, int32_t K) {
  return sp->hit_type == TG_HIT_VEC && ((d & 1) || (2 * (d + K)) % 4);
}

}  // namespace tg

using namespace tg;

extern "C" int tg_rank_cand_half(int64_t C, int32_t d, int32_t K, const tg_score_params* sp, const float* h_cat, float* P,
                                 void* stream) {
  if (C < 0 || C >= 0x7fffffffLL || d <= 0 || K < 0 || !shared_params_ok(sp, K)) return TG_EINVAL;
  if (shared_vec_unsupported(sp, d, K)) return TG_EUNSUPPORTED;
  if (C == 0) return TG_OK;
  if (!h_cat || !P) return TG_EINVAL;
  const int W = d + (sp->hit_type == TG_HIT_VEC ? K : 0);
  hipLaunchKernelGGL(k_half_tile, dim3((unsigned)cdiv(C, SH_BM)), dim3(256), 0, as_stream(stream), C, (int)d, 2 * W, W, h_cat,
                     sp->fc1.w, (const float*)nullptr, P);
  return check_launch("tg_rank_cand_half");
}

extern "C" size_t tg_rank_scores_shared_workspace_bytes(int64_t B, int32_t d, const tg_score_params* sp) {
  if (B < 0 || d <= 0 || !sp) return 0;
  const bool emb = sp->hit_type == TG_HIT_BIN || sp->hit_type == TG_HIT_COUNT;
  const int64_t rows = B + (emb ? 2 * (int64_t)sp->n_hit_rows : 0);
  return (size_t)(rows * d) * sizeof(float) + 16;
}

extern "C" int tg_rank_scores_shared(int64_t B, int64_t C, int32_t d, int32_t K, const tg_score_params* sp,
                                     const float* h_src, const float* P, const int64_t* nbr_src, const int64_t* nbr_cat,
                                     const int64_t* src, const int64_t* cat_ids, float* scores, int64_t ld, void* ws,
                                     size_t ws_bytes, void* stream) {
  if (B < 0 || C < 0 || d <= 0 || K < 0 || !shared_params_ok(sp, K)) return TG_EINVAL;
  if (B > 0 && C > 0 && C > 0x7fffffffLL / B) return TG_EINVAL;  // B C < 2^31
  if (ld < C) return TG_EINVAL;
  if (shared_vec_unsupported(sp, d, K)) return TG_EUNSUPPORTED;
  if (B == 0 || C == 0) return TG_OK;
  if (!h_src || !P || !scores || !ws) return TG_EINVAL;
  const bool hits = sp->hit_type != TG_HIT_NONE;
  if (hits && (K <= 0 || !nbr_src || !nbr_cat || !src || !cat_ids)) return TG_EINVAL;
  if (ws_bytes < tg_rank_scores_shared_workspace_bytes(B, d, sp)) return TG_EINVAL;
  const bool emb = sp->hit_type == TG_HIT_BIN || sp->hit_type == TG_HIT_COUNT;
  hipStream_t st = as_stream(stream);
  SharedArgs a{};
  a.B = B; a.C = C; a.ld = ld;
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
  a.scores = scores;
  if (emb) {
    hipLaunchKernelGGL(k_shared_tables, dim3(flat_grid((int64_t)a.n_hit_rows * d, 256)), dim3(256), 0, st, a.n_hit_rows, (int)d,
                       a.W, a.w1, sp->hit_emb, tab_s, tab_d);
    if (int rc = check_launch("tg_rank_scores_shared(tables)")) return rc;
  }
  hipLaunchKernelGGL(k_half_tile, dim3((unsigned)cdiv(B, SH_BM)), dim3(256), 0, st, B, (int)d, 2 * a.W, 0, h_src, a.w1, a.b1,
                     srow);
  if (int rc = check_launch("tg_rank_scores_shared(source half)")) return rc;
  if (sp->hit_type == TG_HIT_VEC) {
    hipLaunchKernelGGL(k_shared_vec, dim3((unsigned)cdiv(B * C, SH_BM)), dim3(256), 0, st, a);
  } else {
    const unsigned grid = (unsigned)(cdiv(B, SH_TI) * cdiv(C, SH_JS));
    if (emb)
      hipLaunchKernelGGL(k_shared_pairs<true>, dim3(grid), dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL(k_shared_pairs<false>, dim3(grid), dim3(256), 0, st, a);
  }
  return check_launch("tg_rank_scores_shared");
}
