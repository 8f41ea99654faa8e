// Ranking evaluation (one-vs-many): the score head over B * (1 + C) (source, candidate) pairs, and the rank statistics.
// Reference: the score head of tiger/model/tiger.py:257-288 (hit features: data_loader.py:61-75), applied to every
// candidate column in place of the one negative; MRR / Hits@k as the DGB / TGB protocol states them.
//
// tg_rank_scores.  score(i, j) = fc2(relu(fc1([xp | yp]))), fc1 = [d, 2W].  fc1's product is split by operand
// (tg_rank_head.h; this unit also holds the head's two shared kernels, k_head_tables and k_head_half):
//   source half   S[i, :] = W1[:, :d] x_i + b1                one 32-row MFMA tile pass over the B events (k_head_half)
//   hit classes   T_s[c, :] = W1[:, :W] e(c), T_d[c, :] = W1[:, W:] e(c)   ('bin' / 'count': n_hit_rows rows each, k_head_tables)
//   pair half     W1[:, W:W+d] y_p (+ 'vec': the K hit columns of either side as 2K more operand columns)
// The pair half is the B (1 + C)-row product: a 256-thread block owns 32 pair rows, its four wavefronts own 32 hidden
// columns each (a hidden width above 128 takes further column passes) and multiply with v_mfma_f32_32x32x2_f32 (lane l
// feeds A[l & 31][l >> 5], B[l >> 5][l & 31]; accumulator r is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31).
// Operand tiles are staged as [row][k] with a 33-float row stride (tg_gemm.hip: conflict-free ds_write / ds_read_b32).
// The epilogue runs on the accumulators: + S[event] (+ T_s[class] + T_d[class]), ReLU, * fc2.weight, summed over the 32
// lanes of a row's columns, then over column passes and wavefronts in a fixed order, + fc2.bias, one store per pair.
// Neither the hidden activations nor the concatenated pair rows reach memory.  A pair's score is a function of its
// own operands only - not of the row it takes in a tile - so equal pairs give equal bits wherever they stand.
//
// tg_rank_stats.  One wavefront per event counts the candidates that beat / tie the positive over the candidates left
// in (tiger_hip.h); a second one-wave launch folds the events' ranks into the caller's accumulator in a fixed order.
#include <cmath>

#include "tg_rank_head.h"

namespace tg {

struct RankArgs : HeadArgs {  // item = candidate: one row of h_cand, nbr_item and item per pair
  int64_t NP;  // pair rows, B * C1
  int C1, KX;  // 1 + C; operand columns of a pair row
  const float* h_cand;
};

// T_s / T_d: the hit embedding's rows through either half of fc1 (one thread per output)
__global__ void k_head_tables(int n_hit_rows, int d, int W, const float* __restrict__ w1, const float* __restrict__ emb,
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

int head_tables(const HeadArgs& a, const float* emb, hipStream_t st, const char* what) {
  hipLaunchKernelGGL(k_head_tables, dim3(flat_grid((int64_t)a.n_hit_rows * a.d, 256)), dim3(256), 0, st, a.n_hit_rows, a.d, a.W,
                     a.w1, emb, a.tab_s, a.tab_d);
  return check_launch(what);
}

// out[r, n] = sum_k w1[n, wofs + k] h[r, k] (+ bias[n]): a 32-row MFMA tile pass on either weight block of fc1.  The chain
// per output is the one k_rank_tile runs over an operand's first d columns: accumulator from 0, k ascending, two per MFMA,
// zero padding past d - so P stored as f32 and loaded again continues that chain exactly.
__global__ void __launch_bounds__(256) k_head_half(int64_t R, int d, int ldw, int wofs, const float* __restrict__ h,
                                                   const float* __restrict__ w1, const float* __restrict__ bias,
                                                   float* __restrict__ out) {
  __shared__ float As[RH_BM][LDK];
  __shared__ float Bs[RH_BN][LDK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fk = lane >> 5;
  const int64_t m0 = (int64_t)blockIdx.x * RH_BM;
  const int sr = tid >> 3, sk = (tid & 7) * 4;  // staging: 8 threads per 32-float row, 4 consecutive k each
  const float* arow = h + min(m0 + sr, R - 1) * d;  // rows past the end repeat the last one; they are never stored
  const int nkt = (d + BK - 1) / BK;
  for (int nc = 0; nc < d; nc += RH_BN) {
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
      for (int rr = 0; rr < RH_BN / 32; ++rr) {
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

int head_half(int64_t R, int d, int ldw, int wofs, const float* h, const float* w1, const float* bias, float* out,
              hipStream_t st, const char* what) {
  hipLaunchKernelGGL(k_head_half, dim3((unsigned)cdiv(R, RH_BM)), dim3(256), 0, st, R, d, ldw, wofs, h, w1, bias, out);
  return check_launch(what);
}

// rows are the pairs, operand [y_p | dst hits | src hits], weights W1[:, W:] (| W1[:, d:W]), output the scores
__global__ void __launch_bounds__(256) k_rank_tile(RankArgs a) {
  __shared__ float As[RH_BM][LDK];
  __shared__ float Bs[RH_BN][LDK];
  __shared__ float red[4][RH_BM];
  __shared__ int ev[RH_BM];
  __shared__ int2 off[RH_BM];  // (class of the src hits, class of the dst hits) * d per pair row
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fk = lane >> 5;
  const int64_t m0 = (int64_t)blockIdx.x * RH_BM;
  const int d = a.d, K = a.K, W = a.W, KX = a.KX;
  const bool vec = a.hit_type == TG_HIT_VEC;
  const bool emb = a.hit_type == TG_HIT_BIN || a.hit_type == TG_HIT_COUNT;
  if (tid < RH_BM) {
    const int64_t p = min(m0 + tid, a.NP - 1);  // rows past the end repeat the last one; they are never stored
    const int64_t i = p / a.C1;
    ev[tid] = (int)i;
    if (emb) off[tid] = hit_class_off(a, i, p);
  }
  // staging coordinates: 8 threads per 32-float row, 4 consecutive k each
  const int sr = tid >> 3, sk = (tid & 7) * 4;
  const int64_t ap = min(m0 + sr, a.NP - 1);
  const int64_t ai = ap / a.C1;
  const float* arow = a.h_cand + ap * d;
  const int64_t a_src = vec ? a.src[ai] : 0, a_cand = vec ? a.item[ap] : 0;
  float part[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) part[r] = 0.f;
  const int nkt = (KX + BK - 1) / BK;
  for (int nc = 0; nc < d; nc += RH_BN) {
    const bool live = nc + wave * 32 < d;  // wave-uniform: this wavefront has hidden columns in this pass
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int kt = 0; kt < nkt; ++kt) {
      __syncthreads();  // the previous tile has been read (and ev / cls are written)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = kt * BK + sk + e;
        float v = 0.f;
        if (k < d) {
          v = arow[k];
        } else if (vec) {
          v = hit_operand(k - d, K, a.nbr_src + ai * K, a.nbr_item + ap * K, a_src, a_cand);
        }
        As[sr][sk + e] = v;
      }
#pragma unroll
      for (int rr = 0; rr < RH_BN / 32; ++rr) {
        const int n = nc + sr + 32 * rr;
        const float* wrow = a.w1 + (int64_t)min(n, d - 1) * 2 * W;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = kt * BK + sk + e;
          float v = 0.f;
          if (n < d && k < KX) v = pair_weight(wrow, k, W, d);
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
    const int n = nc + wave * 32 + fr;
    if (live && n < d) {
      const float w2 = a.w2[n];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * fk;
        float v = acc[r] + a.srow[(int64_t)ev[row] * d + n];
        if (emb) v += a.tab_s[off[row].x + n] + a.tab_d[off[row].y + n];
        part[r] += fmaxf(v, 0.f) * w2;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) fold_slot(part[r], fr, &red[wave][(r & 3) + 8 * (r >> 2) + 4 * fk]);
  __syncthreads();
  if (tid < RH_BM && m0 + tid < a.NP) a.scores[m0 + tid] = head_score(red, tid, a.b2);
}

// ---- rank statistics --------------------------------------------------------------------------------------------------
struct RankKs {
  int n;
  int k[TG_RANK_MAX_K];
};

__host__ __device__ __forceinline__ bool rank_left_in(int64_t cand, int64_t dst, const uint8_t* mask, int64_t i, int C, int j) {
  return cand != dst && cand != 0 && (!mask || mask[i * C + (j - 1)]);
}

__global__ void __launch_bounds__(256) k_rank_event(int64_t B, int C, const float* __restrict__ scores,
                                                    const int64_t* __restrict__ cand, const int64_t* __restrict__ dst,
                                                    const uint8_t* __restrict__ mask, int32_t* __restrict__ n_greater,
                                                    int32_t* __restrict__ n_equal, int32_t* __restrict__ n_valid,
                                                    double* __restrict__ rank, int64_t* __restrict__ acc_i64) {
  const int lane = lane_id();
  const int64_t i = (int64_t)blockIdx.x * (blockDim.x / TG_WAVE) + threadIdx.x / TG_WAVE;
  if (i >= B) return;  // wave-uniform
  const int C1 = C + 1;
  const float s0 = scores[i * C1];
  const int64_t di = dst[i];
  int g = 0, e = 0, v = 0, bad = std::isfinite(s0) ? 0 : 1;
  for (int j0 = 1; j0 < C1; j0 += TG_WAVE) {
    const int j = j0 + lane;
    bool in = false;
    float s = 0.f;
    if (j < C1) {
      in = rank_left_in(cand[i * C1 + j], di, mask, i, C, j);
      s = scores[i * C1 + j];
    }
    g += __popcll(__ballot(in && s > s0));
    e += __popcll(__ballot(in && s == s0));
    v += __popcll(__ballot(in));
    bad += __popcll(__ballot(in && !std::isfinite(s)));
  }
  if (lane == 0) {
    n_greater[i] = g;
    n_equal[i] = e;
    n_valid[i] = v;
    rank[i] = 1.0 + (double)g + 0.5 * (double)e;
    if (bad) atomicAdd(reinterpret_cast<unsigned long long*>(acc_i64 + 1), (unsigned long long)bad);
  }
}

// one wavefront: lane l sums the events l, l + 64, ... in order, the lanes are folded by a fixed tree
__global__ void __launch_bounds__(TG_WAVE) k_rank_fold(int64_t B, const double* __restrict__ rank, RankKs ks,
                                                      double* __restrict__ acc_f64, int64_t* __restrict__ acc_i64) {
  const int lane = lane_id();
  double rr = 0.0;
  double hits[TG_RANK_MAX_K];
#pragma unroll
  for (int q = 0; q < TG_RANK_MAX_K; ++q) hits[q] = 0.0;
  for (int64_t i = lane; i < B; i += TG_WAVE) {
    const double r = rank[i];
    rr += 1.0 / r;
#pragma unroll
    for (int q = 0; q < TG_RANK_MAX_K; ++q) hits[q] += (q < ks.n && r <= (double)ks.k[q]) ? 1.0 : 0.0;
  }
  for (int off = TG_WAVE / 2; off >= 1; off >>= 1) {
    rr += __shfl_xor(rr, off);
#pragma unroll
    for (int q = 0; q < TG_RANK_MAX_K; ++q) hits[q] += __shfl_xor(hits[q], off);
  }
  if (lane == 0) {
    acc_f64[0] += rr;
#pragma unroll
    for (int q = 0; q < TG_RANK_MAX_K; ++q)
      if (q < ks.n) acc_f64[1 + q] += hits[q];
    acc_i64[0] += B;
  }
}

static bool rank_ks_ok(int32_t n_ks, const int32_t* ks_host, RankKs& out) {
  if (n_ks < 0 || n_ks > TG_RANK_MAX_K || (n_ks > 0 && !ks_host)) return false;
  out.n = n_ks;
  for (int q = 0; q < TG_RANK_MAX_K; ++q) out.k[q] = q < n_ks ? ks_host[q] : 0;
  for (int q = 0; q < n_ks; ++q)
    if (out.k[q] < 1) return false;
  return true;
}

static bool rank_shape_ok(int64_t B, int32_t C) {
  return B >= 0 && C >= 0 && C < 0x7fffffff && (B == 0 || (int64_t)(C + 1) <= 0x7fffffffLL / B);
}

}  // namespace tg

using namespace tg;

extern "C" size_t tg_rank_scores_workspace_bytes(int64_t B, int32_t d, const tg_score_params* sp) {
  return head_workspace_bytes(B, d, sp);
}

extern "C" int tg_rank_scores(int64_t B, int32_t C, int32_t d, int32_t K, const tg_score_params* sp, const float* h_src,
                              const float* h_cand, const int64_t* nbr_src, const int64_t* nbr_cand, const int64_t* src,
                              const int64_t* cand_ids, float* scores, void* ws, size_t ws_bytes, void* stream) {
  if (!rank_shape_ok(B, C) || d <= 0 || K < 0 || !head_params_ok(sp, K)) return TG_EINVAL;
  if (sp->hit_type == TG_HIT_VEC && (2 * (d + K)) % 4) return TG_EUNSUPPORTED;  // as the one-call evaluation step
  if (B == 0) return TG_OK;
  if (!h_src || !h_cand || !scores || !ws) return TG_EINVAL;
  const bool hits = sp->hit_type != TG_HIT_NONE;
  if (hits && (K <= 0 || !nbr_src || !nbr_cand || !src || !cand_ids)) return TG_EINVAL;
  if (ws_bytes < tg_rank_scores_workspace_bytes(B, d, sp)) return TG_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  RankArgs a{};
  head_fill(a, B, d, K, sp, nbr_src, nbr_cand, src, cand_ids, scores, ws);
  a.C1 = C + 1;
  a.NP = B * a.C1;
  a.KX = d + (sp->hit_type == TG_HIT_VEC ? 2 * K : 0);
  a.h_cand = h_cand;
  if (head_emb(sp))
    if (int rc = head_tables(a, sp->hit_emb, st, "tg_rank_scores(tables)")) return rc;
  if (int rc = head_half(B, d, 2 * a.W, 0, h_src, a.w1, a.b1, a.srow, st, "tg_rank_scores(source half)")) return rc;
  hipLaunchKernelGGL(k_rank_tile, dim3((unsigned)cdiv(a.NP, RH_BM)), dim3(256), 0, st, a);
  return check_launch("tg_rank_scores");
}

extern "C" int tg_rank_stats_host(int64_t B, int32_t C, const float* scores_host, const int64_t* cand_ids_host,
                                  const int64_t* dst_host, const uint8_t* mask_host, int32_t n_ks, const int32_t* ks_host,
                                  int32_t* n_greater_host, int32_t* n_equal_host, int32_t* n_valid_host, double* rank_host,
                                  double* acc_f64_host, int64_t* acc_i64_host) {
  RankKs ks;
  if (!rank_shape_ok(B, C) || !rank_ks_ok(n_ks, ks_host, ks)) return TG_EINVAL;
  if (B == 0) return TG_OK;
  if (!scores_host || !cand_ids_host || !dst_host || !n_greater_host || !n_equal_host || !n_valid_host || !rank_host ||
      !acc_f64_host || !acc_i64_host)
    return TG_EINVAL;
  const int64_t C1 = (int64_t)C + 1;
  for (int64_t i = 0; i < B; ++i) {
    const float s0 = scores_host[i * C1];
    int g = 0, e = 0, v = 0;
    int64_t bad = std::isfinite(s0) ? 0 : 1;
    for (int j = 1; j < C1; ++j) {
      if (!rank_left_in(cand_ids_host[i * C1 + j], dst_host[i], mask_host, i, C, j)) continue;
      const float s = scores_host[i * C1 + j];
      g += s > s0;
      e += s == s0;
      v += 1;
      bad += std::isfinite(s) ? 0 : 1;
    }
    const double r = 1.0 + (double)g + 0.5 * (double)e;
    n_greater_host[i] = g;
    n_equal_host[i] = e;
    n_valid_host[i] = v;
    rank_host[i] = r;
    acc_f64_host[0] += 1.0 / r;
    for (int q = 0; q < ks.n; ++q) acc_f64_host[1 + q] += r <= (double)ks.k[q] ? 1.0 : 0.0;
    acc_i64_host[1] += bad;
  }
  acc_i64_host[0] += B;
  return TG_OK;
}

extern "C" int tg_rank_stats(int64_t B, int32_t C, const float* scores, const int64_t* cand_ids, const int64_t* dst,
                             const uint8_t* mask, int32_t n_ks, const int32_t* ks_host, int32_t* n_greater,
                             int32_t* n_equal, int32_t* n_valid, double* rank, double* acc_f64, int64_t* acc_i64,
                             void* stream) {
  RankKs ks;
  if (!rank_shape_ok(B, C) || !rank_ks_ok(n_ks, ks_host, ks)) return TG_EINVAL;
  if (B == 0) return TG_OK;
  if (!scores || !cand_ids || !dst || !n_greater || !n_equal || !n_valid || !rank || !acc_f64 || !acc_i64) return TG_EINVAL;
  hipStream_t st = as_stream(stream);
  const int waves = 256 / TG_WAVE;
  hipLaunchKernelGGL(k_rank_event, dim3((unsigned)cdiv(B, waves)), dim3(256), 0, st, B, (int)C, scores, cand_ids, dst, mask,
                     n_greater, n_equal, n_valid, rank, acc_i64);
  if (int rc = check_launch("tg_rank_stats(events)")) return rc;
  hipLaunchKernelGGL(k_rank_fold, dim3(1), dim3(TG_WAVE), 0, st, B, (const double*)rank, ks, acc_f64, acc_i64);
  return check_launch("tg_rank_stats");
}
