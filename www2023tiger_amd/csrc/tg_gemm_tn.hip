// Weight-gradient products and column sums on the float32 MFMA: out[n, k] = sum_m Y[m, n] X[m, k], single and grouped,
// with their fixed-order reductions (k_gemm_tn, k_gemm_tn_group, k_tn_reduce*, k_colsum*).
// Reference: the weight and bias gradients that autograd forms for torch.nn.Linear / nn.GRUCell
// (tiger/model/update_modules.py:30-47, message_modules.py:29-55, basic_modules.py:16-19).
#include "tg_mfma.h"

namespace tg {

// ---------------------------------------------------------------------------------
// Weight gradients: out[n, k] = sum_m Y[m, n] X[m, k].  Both MFMA operands are read along m,
// so tiles are staged [m][col] exactly as they lie in memory (no transposition): lane l feeds
// A[n = l&31][m = l>>5] = Ys[m][n], B[m = l>>5][k = l&31] = Xs[m][k].
// ---------------------------------------------------------------------------------
constexpr int TN_T = 64;        // output tile (n and k extent)
constexpr int TN_MC = 32;       // m rows per staged chunk
constexpr int TN_LD = TN_T + 32;  // row stride: the two half-waves (rows m, m+1) hit disjoint banks

__device__ __forceinline__ void tn_block(const TnArgs& a, int splits, int b) {
  __shared__ float Ys[2][TN_MC][TN_LD];
  __shared__ float Xs[2][TN_MC][TN_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NT = (a.n + TN_T - 1) / TN_T, KT = (a.k + TN_T - 1) / TN_T;
  const int kt = b % KT; b /= KT;
  const int nt = b % NT; b /= NT;
  const int bz = b % a.nbatch;
  const int sp = b / a.nbatch;
  int64_t M = a.m_cap;
  if (a.m_dev) M = min(M, (int64_t)*a.m_dev);
  const int64_t mc = ((M + splits - 1) / splits + TN_MC - 1) / TN_MC * TN_MC;  // rows per split
  const int64_t m_lo = (int64_t)sp * mc, m_hi = min(M, m_lo + mc);
  const int n0 = nt * TN_T, k0 = kt * TN_T;
  const int wn = wave >> 1, wk = wave & 1;
  const int fr = lane & 31, fk = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  // staging coordinates: 16 threads per 64-float row, 16 rows per pass, 2 passes per operand
  const int sr = tid >> 4, sc = (tid & 15) * 4;
  const float* yb = a.y + (int64_t)bz * a.y_bs;
  const float* x0b = a.x0.p + (int64_t)bz * a.x0_bs;
  const int ycol = min(n0 + sc, a.n - 4);           // clamped: columns past N are zeroed at the LDS store
  const bool yin = n0 + sc < a.n;
  const int kcol = k0 + sc;
  const bool xin = kcol < a.k;
  const int kc = xin ? kcol : 0;
  const bool seg1 = kc >= a.x0.w;
  // Two chunks travel in registers (sets A / B) while a third is multiplied from LDS, and the row indices of
  // gathered X rows (mailbox / memory rows of the outdated nodes) are fetched one chunk further ahead, so that
  // a chunk's row loads never wait for their index.  All loads are unconditional (rows clamped to M - 1, zeroed
  // at the LDS store when past the split): the loop body is straight-line code with exact wait counts.
  struct Regs {
    float4 y[2], x[2];
    int64_t row[2];
  };
  const int64_t* xidx = seg1 ? a.x1.idx : a.x0.idx;
  auto load_index = [&](int64_t mb, Regs& r) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t m = min(mb + sr + i * 16, M - 1);
      r.row[i] = xidx ? xidx[m] : m;
    }
  };
  auto load_chunk = [&](int64_t mb, Regs& r) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t m = min(mb + sr + i * 16, M - 1);
      r.y[i] = ldg4(yb + m * a.ldy + ycol);
      const float* xr = seg1 ? a.x1.p + r.row[i] * a.x1.ld + (kc - a.x0.w) : x0b + r.row[i] * a.x0.ld + kc;
      r.x[i] = ldg4(xr);
    }
  };
  auto store_chunk = [&](int buf, int64_t mb, const Regs& r) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bool live = mb + sr + i * 16 < m_hi;
      *reinterpret_cast<float4*>(&Ys[buf][sr + i * 16][sc]) = (live && yin) ? r.y[i] : zero4();
      *reinterpret_cast<float4*>(&Xs[buf][sr + i * 16][sc]) = (live && xin) ? r.x[i] : zero4();
    }
  };
  const bool do_bias = a.bias_out && kt == 0 && tid < TN_T;  // column sums of Y ride on the k-tile-0 blocks
  float bsum = 0.f;
  // chunk `mb` is in LDS[buf]: request chunk mb + 2 into `ld` (its indices are there already) and the indices of
  // chunk mb + 3 into `nx`'s slot... (see the call sites), multiply, then move chunk mb + 1 from `stv` to LDS
  auto step = [&](int buf, int64_t mb, Regs& ld, const Regs& stv) {
    load_chunk(mb + 2 * TN_MC, ld);
    const float* yp = &Ys[buf][fk][wn * 32 + fr];
    const float* xp = &Xs[buf][fk][wk * 32 + fr];
#pragma unroll
    for (int s2 = 0; s2 < TN_MC / 2; ++s2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(yp[s2 * 2 * TN_LD], xp[s2 * 2 * TN_LD], acc, 0, 0, 0);
    if (do_bias) {
      if (a.bias_rs) {
        for (int r = 0; r < TN_MC; ++r) {
          const int64_t m = min(mb + r, M - 1);  // rows past m_hi are zero in Ys
          bsum = fmaf(Ys[buf][r][tid], a.bias_rs[m * a.ld_brs + a.brs_col + bz], bsum);
        }
      } else {
#pragma unroll
        for (int r = 0; r < TN_MC; ++r) bsum += Ys[buf][r][tid];
      }
    }
    store_chunk(buf ^ 1, mb + TN_MC, stv);
    __syncthreads();
  };
  if (m_lo < m_hi) {
    Regs ra, rb;
    load_index(m_lo, ra);
    load_index(m_lo + TN_MC, rb);
    load_chunk(m_lo, ra);
    load_chunk(m_lo + TN_MC, rb);
    store_chunk(0, m_lo, ra);
    load_index(m_lo + 2 * TN_MC, ra);
    __syncthreads();
    int64_t mb = m_lo;
    const int64_t m_pairs = m_lo + (m_hi - m_lo + TN_MC - 1) / TN_MC / 2 * (2 * TN_MC);  // end of the whole chunk pairs
    for (; mb < m_pairs; mb += 2 * TN_MC) {
      // even chunk from LDS[0]: chunk mb+2 -> ra, chunk mb+1 (rb) -> LDS[1]; then rb's indices for chunk mb+3
      step(0, mb, ra, rb);
      load_index(mb + 3 * TN_MC, rb);
      step(1, mb + TN_MC, rb, ra);
      load_index(mb + 4 * TN_MC, ra);
    }
    if (mb < m_hi) step(0, mb, ra, rb);
  }
  // partial tile -> part[sp][bz][n][k] (zeros when this split is empty)
  float* pp = a.part + ((int64_t)sp * a.nbatch + bz) * a.n * a.k;
  const int kk = k0 + wk * 32 + fr;
  if (kk < a.k) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + wn * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
      if (n < a.n) pp[(int64_t)n * a.k + kk] = acc[r];
    }
  }
  if (do_bias && n0 + tid < a.n) {
    float* bp = a.part + (int64_t)splits * a.nbatch * a.n * a.k;  // bias partials follow the weight partials
    bp[((int64_t)sp * a.nbatch + bz) * a.n + n0 + tid] = bsum;
  }
}

__global__ void __launch_bounds__(256) k_gemm_tn(TnArgs a, int splits) { tn_block(a, splits, (int)blockIdx.x); }

// fixed-order reduction of the split partials of one problem; threads [start, start + stride, ...)
__device__ __forceinline__ void tn_reduce_part(const TnArgs& a, int splits, int64_t start, int64_t stride) {
  const int64_t per = (int64_t)a.n * a.k, total = per * a.nbatch;
  for (int64_t t = start; t < total; t += stride) {
    const int bz = (int)(t / per);
    const int64_t e = t - (int64_t)bz * per;
    float s = 0.f;
    for (int sp = 0; sp < splits; ++sp) s += a.part[((int64_t)sp * a.nbatch + bz) * per + e];
    float* o = a.out + (int64_t)bz * a.out_bs + (e / a.k) * a.ldo + (e % a.k);
    *o = a.alpha * s + (a.accumulate ? *o : 0.f);
  }
  if (a.bias_out) {
    const float* bp = a.part + (int64_t)splits * a.nbatch * per;
    const int64_t tb = (int64_t)a.n * a.nbatch;
    for (int64_t t = start; t < tb; t += stride) {
      const int bz = (int)(t / a.n);
      const int n = (int)(t - (int64_t)bz * a.n);
      float s = 0.f;
      for (int sp = 0; sp < splits; ++sp) s += bp[((int64_t)sp * a.nbatch + bz) * a.n + n];
      float* o = a.bias_out + (int64_t)bz * a.bias_bs + n;
      *o = a.alpha * s + (a.bias_accumulate ? *o : 0.f);
    }
  }
}
__global__ void k_tn_reduce(TnArgs a, int splits) {
  tn_reduce_part(a, splits, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// several weight-gradient products in ONE launch (and one reduction launch): the nine products of
// the contrastive backward pass are each too small to fill the chip and independent of one another
__global__ void __launch_bounds__(256) k_gemm_tn_group(TnGroup g) {
  int p = 0;
  while (p + 1 < g.n && (int)blockIdx.x >= g.first_block[p + 1]) ++p;
  tn_block(g.a[p], g.splits[p], (int)blockIdx.x - g.first_block[p]);
}
__global__ void k_tn_reduce_group(TnGroup g) {
  int p = 0;
  while (p + 1 < g.n && (int)blockIdx.x >= g.first_rblock[p + 1]) ++p;
  const int nb = g.first_rblock[p + 1] - g.first_rblock[p];
  tn_reduce_part(g.a[p], g.splits[p], (int64_t)((int)blockIdx.x - g.first_rblock[p]) * blockDim.x + threadIdx.x,
                 (int64_t)nb * blockDim.x);
}

int gemm_tn_launch(const TnArgs& a, hipStream_t st) {
  if (a.m_cap <= 0) return TG_OK;
  if (a.n <= 0 || a.k <= 0 || (a.n % 4) || (a.k % 4) || (a.x0.w % 4) || (a.ldy % 4) || a.nbatch <= 0) return TG_EINVAL;
  if (a.x0.w + (a.x1.p ? a.x1.w : 0) != a.k) return TG_EINVAL;
  const int NT = (int)cdiv(a.n, TN_T), KT = (int)cdiv(a.k, TN_T);
  const int64_t tiles = (int64_t)NT * KT * a.nbatch;
  // enough blocks to fill the chip, but a short fixed-order reduction (k_tn_reduce walks the splits serially)
  int64_t splits = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(cdiv(768, tiles), 16), cdiv(a.m_cap, 2 * TN_MC)));
  const int64_t fit = (int64_t)(a.part_floats / ((size_t)a.nbatch * a.n * (a.k + 1)));
  if (fit < 1) return TG_EWORKSPACE;
  splits = std::min(splits, fit);
  TG_KLAUNCH(k_gemm_tn, dim3((unsigned)(tiles * splits)), dim3(256), 0, st, a, (int)splits);
  TG_KLAUNCH(k_tn_reduce, dim3(flat_grid((int64_t)a.n * a.k * a.nbatch, 256)), dim3(256), 0, st, a, (int)splits);
  return check_launch("gemm_tn");
}

int gemm_tn_group_launch(const TnArgs* list, int n, float* part, size_t part_floats, hipStream_t st) {
  if (n <= 0) return TG_OK;
  if (n > TN_GROUP_MAX) return TG_EINVAL;
  TnGroup g{};
  g.n = n;
  int64_t tiles_total = 0;
  for (int p = 0; p < n; ++p) {
    const TnArgs& a = list[p];
    if (a.m_cap <= 0 || a.n <= 0 || a.k <= 0 || (a.n % 4) || (a.k % 4) || (a.x0.w % 4) || (a.ldy % 4) || a.nbatch <= 0)
      return TG_EINVAL;
    if (a.x0.w + (a.x1.p ? a.x1.w : 0) != a.k) return TG_EINVAL;
    tiles_total += cdiv(a.n, TN_T) * cdiv(a.k, TN_T) * a.nbatch;
  }
  // splits: aim at ~1500 blocks in total, at least two staged chunks per block
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>(16, cdiv(1536, tiles_total)));
  size_t off = 0;
  for (int p = 0; p < n; ++p) {
    g.a[p] = list[p];
    TnArgs& a = g.a[p];
    const int64_t tiles = cdiv(a.n, TN_T) * cdiv(a.k, TN_T) * a.nbatch;
    const int64_t sp = std::max<int64_t>(1, std::min<int64_t>(want, cdiv(a.m_cap, 2 * TN_MC)));
    const size_t need = (size_t)sp * a.nbatch * a.n * (a.k + 1);
    if (off + need > part_floats) return TG_EWORKSPACE;
    a.part = part + off;
    a.part_floats = need;
    off += (need + 3) & ~(size_t)3;
    g.splits[p] = (int)sp;
    g.first_block[p + 1] = g.first_block[p] + (int)(tiles * sp);
    g.first_rblock[p + 1] = g.first_rblock[p] + (int)std::min<int64_t>(cdiv((int64_t)a.n * a.k * a.nbatch, 256), 256);
  }
  TG_KLAUNCH(k_gemm_tn_group, dim3((unsigned)g.first_block[n]), dim3(256), 0, st, g);
  TG_KLAUNCH(k_tn_reduce_group, dim3((unsigned)g.first_rblock[n]), dim3(256), 0, st, g);
  return check_launch("gemm_tn_group");
}

// column sums: one block per (64 columns, split of m); partials then a fixed-order reduce
__global__ void __launch_bounds__(256) k_colsum(int64_t m_cap, const int32_t* __restrict__ m_dev, int n,
                                                const float* __restrict__ y, int64_t ldy, float* __restrict__ part,
                                                int splits) {
  __shared__ float red[4][64];
  const int c = blockIdx.x % ((n + 63) / 64) * 64 + (threadIdx.x & 63);
  const int sp = blockIdx.x / ((n + 63) / 64);
  int64_t M = m_cap;
  if (m_dev) M = min(M, (int64_t)*m_dev);
  const int64_t mc = (M + splits - 1) / splits;
  const int64_t lo = sp * mc, hi = min(M, lo + mc);
  float s = 0.f;
  if (c < n)
    for (int64_t m = lo + (threadIdx.x >> 6); m < hi; m += 4) s += y[m * ldy + c];
  red[threadIdx.x >> 6][threadIdx.x & 63] = s;
  __syncthreads();
  if (threadIdx.x < 64 && c < n) part[(int64_t)sp * n + c] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}
__global__ void k_colsum_reduce(int n, const float* __restrict__ part, int splits, float alpha, float* __restrict__ out,
                                int accumulate) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  float s = 0.f;
  for (int sp = 0; sp < splits; ++sp) s += part[(int64_t)sp * n + c];
  out[c] = alpha * s + (accumulate ? out[c] : 0.f);
}

int colsum_launch(int64_t m_cap, const int32_t* m_dev, int n, const float* y, int64_t ldy, float alpha, float* out,
                  int accumulate, float* part, size_t part_floats, hipStream_t st) {
  if (m_cap <= 0 || n <= 0) return TG_OK;
  const int ct = (n + 63) / 64;
  int64_t splits = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(cdiv(512, ct), 16), cdiv(m_cap, 64)));
  splits = std::min<int64_t>(splits, (int64_t)(part_floats / (size_t)n));
  if (splits < 1) return TG_EWORKSPACE;
  TG_KLAUNCH(k_colsum, dim3((unsigned)(ct * splits)), dim3(256), 0, st, m_cap, m_dev, n, y, ldy, part, (int)splits);
  TG_KLAUNCH(k_colsum_reduce, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, n, part, (int)splits, alpha, out,
                     accumulate);
  return check_launch("colsum");
}


}  // namespace tg
