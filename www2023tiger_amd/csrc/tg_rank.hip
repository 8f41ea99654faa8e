// Ranking evaluation (one-vs-many): the score head over B * (1 + C) (source, candidate) pairs, and the rank statistics.
// Reference: the score head of tiger/model/tiger.py:257-288 (hit features: data_loader.py:61-75), applied to every
// candidate column in place of the one negative; MRR / Hits@k as the DGB / TGB protocol states them.
//
// tg_rank_scores.  score(i, j) = fc2(relu(fc1([xp | yp]))), fc1 = [d, 2W].  fc1's product is split by operand:
//   source half   S[i, :] = W1[:, :d] x_i + b1                one 32-row MFMA tile pass over the B events (k_rank_tile<true>)
//   hit classes   T_s[c, :] = W1[:, :W] e(c), T_d[c, :] = W1[:, W:] e(c)   ('bin' / 'count': n_hit_rows rows each, k_rank_tables)
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

#include "tg_mfma.h"

namespace tg {

constexpr int RK_BM = 32;   // pair rows of a block
constexpr int RK_BN = 128;  // hidden columns of a column pass (4 wavefronts x 32)

struct RankArgs {
  int64_t B, P;  // events; rows of this pass (B: source half, B * C1: pairs)
  int C1, d, K, W, KX;  // 1 + C; hidden width; neighbours; operand width of one side; operand columns of this pass
  int hit_type, n_hit_rows;
  const float *h_src, *h_cand;
  const int64_t *nbr_src, *nbr_cand, *src, *cand;
  const float *w1, *b1, *w2, *b2;
  float *srow, *tab_s, *tab_d;
  float* scores;
};

// T_s / T_d: the hit embedding's rows through either half of fc1 (one thread per output)
__global__ void k_rank_tables(RankArgs a, const float* __restrict__ emb) {
  const int total = a.n_hit_rows * a.d;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    const int c = t / a.d, n = t - c * a.d;
    const float* w = a.w1 + (int64_t)n * 2 * a.W;
    const float* e = emb + (int64_t)c * a.d;
    float s = 0.f, q = 0.f;
    for (int k = 0; k < a.d; ++k) {
      s += w[k] * e[k];
      q += w[a.W + k] * e[k];
    }
    a.tab_s[t] = s;
    a.tab_d[t] = q;
  }
}

// PRE: rows are the events, operand x_i, weights W1[:, :d], output S = product + b1.
// else: rows are the pairs, operand [y_p | dst hits | src hits], weights W1[:, W:] (| W1[:, d:W]), output the scores.
template <bool PRE>
__global__ void __launch_bounds__(256) k_rank_tile(RankArgs a) {
  __shared__ float As[RK_BM][LDK];
  __shared__ float Bs[RK_BN][LDK];
  __shared__ float red[4][RK_BM];
  __shared__ int ev[RK_BM];
  __shared__ int cls[RK_BM][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 31, fk = lane >> 5;
  const int64_t m0 = (int64_t)blockIdx.x * RK_BM;
  const int d = a.d, K = a.K, W = a.W, KX = a.KX;
  const bool vec = !PRE && a.hit_type == TG_HIT_VEC;
  const bool emb = !PRE && (a.hit_type == TG_HIT_BIN || a.hit_type == TG_HIT_COUNT);
  if (tid < RK_BM) {
    const int64_t p = min(m0 + tid, a.P - 1);  // rows past the end repeat the last one; they are never stored
    const int64_t i = PRE ? p : p / a.C1;
    ev[tid] = (int)i;
    int cs = 0, cd = 0;
    if (emb) {
      const int64_t s = a.src[i], c = a.cand[p];
      for (int k = 0; k < K; ++k) {
        cs += a.nbr_cand[p * K + k] == s ? 1 : 0;  // the source among the candidate's neighbours (src hits)
        cd += a.nbr_src[i * K + k] == c ? 1 : 0;   // the candidate among the source's neighbours (dst hits)
      }
      if (a.hit_type == TG_HIT_BIN) {
        cs = cs > 0;
        cd = cd > 0;
      }
      cs = min(cs, a.n_hit_rows - 1);
      cd = min(cd, a.n_hit_rows - 1);
    }
    cls[tid][0] = cs;
    cls[tid][1] = cd;
  }
  // staging coordinates: 8 threads per 32-float row, 4 consecutive k each
  const int sr = tid >> 3, sk = (tid & 7) * 4;
  const int64_t ap = min(m0 + sr, a.P - 1);
  const int64_t ai = PRE ? ap : ap / a.C1;
  const float* arow = PRE ? a.h_src + ap * d : a.h_cand + ap * d;
  const int64_t a_src = vec ? a.src[ai] : 0, a_cand = vec ? a.cand[ap] : 0;
  float part[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) part[r] = 0.f;
  const int nkt = (KX + BK - 1) / BK;
  for (int nc = 0; nc < d; nc += RK_BN) {
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
        } else if (vec && k < d + K) {
          v = a.nbr_src[ai * K + (k - d)] == a_cand ? 1.f : 0.f;
        } else if (vec && k < KX) {
          v = a.nbr_cand[ap * K + (k - d - K)] == a_src ? 1.f : 0.f;
        }
        As[sr][sk + e] = v;
      }
#pragma unroll
      for (int rr = 0; rr < RK_BN / 32; ++rr) {
        const int n = nc + sr + 32 * rr;
        const float* wrow = a.w1 + (int64_t)min(n, d - 1) * 2 * W;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = kt * BK + sk + e;
          float v = 0.f;
          if (n < d && k < KX) v = PRE ? wrow[k] : (k < W ? wrow[W + k] : wrow[d + (k - W)]);
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
      const float b1 = PRE ? a.b1[n] : 0.f;
      const float w2 = PRE ? 0.f : a.w2[n];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * fk;
        if (PRE) {
          if (m0 + row < a.P) a.srow[(m0 + row) * d + n] = acc[r] + b1;
        } else {
          float v = acc[r] + a.srow[(int64_t)ev[row] * d + n];
          if (emb) v += a.tab_s[cls[row][0] * d + n] + a.tab_d[cls[row][1] * d + n];
          part[r] += fmaxf(v, 0.f) * w2;
        }
      }
    }
  }
  if (PRE) return;
  // the 32 lanes of one fk half hold the columns of the same 16 rows
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = part[r];
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if (fr == 0) red[wave][(r & 3) + 8 * (r >> 2) + 4 * fk] = v;
  }
  __syncthreads();
  if (tid < RK_BM && m0 + tid < a.P) a.scores[m0 + tid] = ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) + a.b2[0];
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

static bool rank_score_params_ok(const tg_score_params* sp, int32_t d, int32_t K) {
  if (!sp || !sp->fc1.w || !sp->fc1.b || !sp->fc2.w || !sp->fc2.b) return false;
  if (sp->hit_type < TG_HIT_NONE || sp->hit_type > TG_HIT_COUNT) return false;
  const bool emb = sp->hit_type == TG_HIT_BIN || sp->hit_type == TG_HIT_COUNT;
  if (emb && (!sp->hit_emb || sp->n_hit_rows < (sp->hit_type == TG_HIT_BIN ? 2 : K + 1))) return false;
  return true;
}

}  // namespace tg

using namespace tg;

extern "C" size_t tg_rank_scores_workspace_bytes(int64_t B, int32_t d, const tg_score_params* sp) {
  if (B < 0 || d <= 0 || !sp) return 0;
  const bool emb = sp->hit_type == TG_HIT_BIN || sp->hit_type == TG_HIT_COUNT;
  const int64_t rows = B + (emb ? 2 * (int64_t)sp->n_hit_rows : 0);
  return (size_t)(rows * d) * sizeof(float) + 16;
}

extern "C" int tg_rank_scores(int64_t B, int32_t C, int32_t d, int32_t K, const tg_score_params* sp, const float* h_src,
                              const float* h_cand, const int64_t* nbr_src, const int64_t* nbr_cand, const int64_t* src,
                              const int64_t* cand_ids, float* scores, void* ws, size_t ws_bytes, void* stream) {
  if (!rank_shape_ok(B, C) || d <= 0 || K < 0 || !rank_score_params_ok(sp, d, K)) return TG_EINVAL;
  if (sp->hit_type == TG_HIT_VEC && (2 * (d + K)) % 4) return TG_EUNSUPPORTED;  // as the one-call evaluation step
  if (B == 0) return TG_OK;
  if (!h_src || !h_cand || !scores || !ws) return TG_EINVAL;
  const bool hits = sp->hit_type != TG_HIT_NONE;
  if (hits && (K <= 0 || !nbr_src || !nbr_cand || !src || !cand_ids)) return TG_EINVAL;
  if (ws_bytes < tg_rank_scores_workspace_bytes(B, d, sp)) return TG_EWORKSPACE;
  const bool emb = sp->hit_type == TG_HIT_BIN || sp->hit_type == TG_HIT_COUNT;
  hipStream_t st = as_stream(stream);
  RankArgs a{};
  a.B = B;
  a.C1 = C + 1;
  a.d = d;
  a.K = K;
  a.W = d + (sp->hit_type == TG_HIT_VEC ? K : 0);
  a.hit_type = sp->hit_type;
  a.n_hit_rows = emb ? sp->n_hit_rows : 0;
  a.h_src = h_src; a.h_cand = h_cand;
  a.nbr_src = nbr_src; a.nbr_cand = nbr_cand; a.src = src; a.cand = cand_ids;
  a.w1 = sp->fc1.w; a.b1 = sp->fc1.b; a.w2 = sp->fc2.w; a.b2 = sp->fc2.b;
  a.srow = static_cast<float*>(ws);
  a.tab_s = a.srow + B * d;
  a.tab_d = a.tab_s + (int64_t)a.n_hit_rows * d;
  a.scores = scores;
  if (emb) {
    hipLaunchKernelGGL(k_rank_tables, dim3(flat_grid((int64_t)a.n_hit_rows * d, 256)), dim3(256), 0, st, a, sp->hit_emb);
    if (int rc = check_launch("tg_rank_scores(tables)")) return rc;
  }
  a.P = B;
  a.KX = d;
  hipLaunchKernelGGL(k_rank_tile<true>, dim3((unsigned)cdiv(a.P, RK_BM)), dim3(256), 0, st, a);
  if (int rc = check_launch("tg_rank_scores(source half)")) return rc;
  a.P = B * a.C1;
  a.KX = d + (sp->hit_type == TG_HIT_VEC ? 2 * K : 0);
  hipLaunchKernelGGL(k_rank_tile<false>, dim3((unsigned)cdiv(a.P, RK_BM)), dim3(256), 0, st, a);
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
