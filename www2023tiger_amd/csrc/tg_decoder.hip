// Node-classification decoder and its metric (tiger/model/basic_modules.py:22-33, tiger/eval_utils.py:72-99).
//   MLP(d):  y = W3 drop(relu(z2)) + b3,  z2 = W2 drop(relu(z1)) + b2,  z1 = W1 x + b1     (80 and 10 hidden units)
// tg_decoder_fwd: the three layers in one launch.  A workgroup of four wavefronts takes 64 rows at a time, 16 per
// wavefront; layer 1 is a 16 x 80 tile per wavefront on v_mfma_f32_16x16x4_f32 (five 16-column tiles), its A operand
// read straight from x (one float4 per lane and 16-wide K block), its B operand from W1 staged in LDS (K in chunks of
// DEC_KC columns: once per workgroup when d <= DEC_KC, once per row tile beyond).  The K index an MFMA step stands for
// is permuted (lane group g, step s -> k = kb + 4 g + s) identically in A and B, so each lane reads whole float4s.
// Layers 2 and 3 run on VALU from the wavefront's activation tile in LDS.
// tg_decoder_bwd: two launches, no float atomics.  (1) per row tile: dz2, dz1 (kept in the workspace), dx; per
// workgroup partial sums of dW2, db2, dW3, db3, db1 in a fixed row order.  (2) dW1 = dz1^T x, every output summed over
// all rows in row order by the one thread that owns it, and one more workgroup that adds the partials in workgroup
// order: the gradients do not depend on scheduling.
// tg_roc_auc: sklearn's roc_auc_score over a whole array.  Keys: order-preserving uint32 of the finite negatives'
// scores (positives and non-finite scores map to 0xffffffff, above every finite key), an LSD radix sort of the keys
// (four 8-bit passes: histogram, scan, stable wavefront multisplit scatter), then every finite positive counts the
// negatives below and equal to its score by binary search in the sorted prefix:
//   AUC = sum over positives of (#neg < s + 0.5 #neg == s) / (P N),
// accumulated as the integer 2 #lt + #eq - exact, and independent of the order of the additions.
#include <algorithm>
#include <utility>

#include "tg_common.h"

namespace tg {

constexpr int DEC_H1 = 80, DEC_H2 = 10;
constexpr int DEC_KC = 192;          // W1 columns staged in LDS at a time (d = 172 in one chunk)
constexpr int DEC_LDW = DEC_KC + 4;  // LDS row pitch of the W1 chunk (floats)
constexpr int DEC_A1P = DEC_H1 + 4;  // LDS row pitch of an activation tile
constexpr int DEC_ROWS = 64;         // rows per workgroup tile (16 per wavefront in the forward)
constexpr int DEC_KB = DEC_KC / 16;  // 16-wide K blocks of a chunk
constexpr int DEC_STAGE = (DEC_H1 * DEC_KC / 4 + 255) / 256;  // float4s of a W1 chunk per thread
constexpr size_t DEC_FWD_LDS = (size_t)(DEC_H1 * DEC_LDW + DEC_H2 * DEC_H1 + 4 * 16 * DEC_A1P + 4 * 16 * 12) * 4;

typedef float v4f __attribute__((ext_vector_type(4)));

struct DecW {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
};

// inverted-dropout factor of element idx of mask stream `site` (1 when dropout is off)
__device__ __forceinline__ float dec_drop(const DropCfg& dc, uint64_t key, uint32_t site, uint64_t idx) {
  if (dc.p <= 0.f) return 1.f;
  return drop_keep(key, site, idx, dc.thresh) ? dc.scale : 0.f;
}

__global__ void __launch_bounds__(256) k_decoder_fwd(int64_t n, const float* __restrict__ x, int d, DecW w, DropCfg dc,
                                                     float* __restrict__ y, float* __restrict__ z1_out,
                                                     float* __restrict__ z2_out) {
  extern __shared__ float lds[];
  float* w1s = lds;                     // [80][DEC_LDW]
  float* w2s = w1s + DEC_H1 * DEC_LDW;  // [10][80]
  float* a1s = w2s + DEC_H2 * DEC_H1;   // [4 wavefronts][16][DEC_A1P]
  float* a2s = a1s + 4 * 16 * DEC_A1P;  // [4 wavefronts][16][12]
  const int lane = lane_id(), wv = threadIdx.x / TG_WAVE;
  const int g = lane >> 4, c16 = lane & 15;
  const int nchunk = (d + DEC_KC - 1) / DEC_KC;
  const uint64_t key = drop_key(dc);
  for (int i = threadIdx.x; i < DEC_H2 * DEC_H1; i += blockDim.x) w2s[i] = w.w2[i];
  float* A1 = a1s + wv * 16 * DEC_A1P;
  float* A2 = a2s + wv * 16 * 12;
  const int64_t ntile = (n + DEC_ROWS - 1) / DEC_ROWS;
  bool staged = false;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int64_t r0 = tile * DEC_ROWS + wv * 16;  // this wavefront's first row
    const int64_t ra = r0 + c16;                   // the row this lane feeds into the A operand
    const bool live = ra < n;
    v4f acc[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) acc[t] = v4f{0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < nchunk; ++ch) {
      const int k0 = ch * DEC_KC, kn = min(DEC_KC, d - k0);
      // every global load of the chunk is issued before the first one is waited for: this row's float4s of x, then
      // (first tile / several chunks) the chunk of W1 - at small n the kernel is bound by these round trips
      float4 xa[DEC_KB];
#pragma unroll
      for (int b = 0; b < DEC_KB; ++b) {
        const int kk = 16 * b + 4 * g;  // this lane's float4 of the 16-wide K block b (d % 4 == 0: wholly in or out)
        xa[b] = (live && kk < kn) ? *reinterpret_cast<const float4*>(x + ra * d + k0 + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      if (!staged) {
        __syncthreads();  // every wavefront is done with the previous chunk
        const int q4 = kn / 4;
        float4 wv4[DEC_STAGE];
#pragma unroll
        for (int u = 0; u < DEC_STAGE; ++u) {
          const int i = min((int)threadIdx.x + 256 * u, DEC_H1 * q4 - 1);  // (past the end: a repeated load, not stored)
          const int j = i / q4, q = i - j * q4;
          wv4[u] = *reinterpret_cast<const float4*>(w.w1 + (int64_t)j * d + k0 + 4 * q);
        }
#pragma unroll
        for (int u = 0; u < DEC_STAGE; ++u) {
          const int i = threadIdx.x + 256 * u;
          const int j = i / q4, q = i - j * q4;
          if (i < DEC_H1 * q4) *reinterpret_cast<float4*>(w1s + j * DEC_LDW + 4 * q) = wv4[u];
        }
        __syncthreads();
        staged = nchunk == 1;  // a single chunk stays for every later tile
      }
#pragma unroll
      for (int b = 0; b < DEC_KB; ++b) {
        const int kk = 16 * b + 4 * g;  // (blocks past kn multiply zeros: DEC_KB is a compile-time trip count)
        float4 wb[5];
#pragma unroll
        for (int t = 0; t < 5; ++t)
          wb[t] = kk < kn ? *reinterpret_cast<const float4*>(w1s + (t * 16 + c16) * DEC_LDW + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int t = 0; t < 5; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[b].x, wb[t].x, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 5; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[b].y, wb[t].y, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 5; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[b].z, wb[t].z, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 5; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[b].w, wb[t].w, acc[t], 0, 0, 0);
      }
    }
    // layer-1 epilogue: the lane holds rows 4 g + r, column 16 t + c16 of the wavefront's 16 x 80 tile
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const int col = t * 16 + c16;
      const float bias = w.b1[col];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = 4 * g + r;
        const int64_t row = r0 + rl;
        const float z = acc[t][r] + bias;
        float a = 0.f;
        if (row < n) {
          if (z1_out) z1_out[row * DEC_H1 + col] = z;
          a = z > 0.f ? z * dec_drop(dc, key, DROP_DEC1, (uint64_t)row * DEC_H1 + col) : 0.f;
        }
        A1[rl * DEC_A1P + col] = a;
      }
    }
    __syncthreads();
    {  // layer 2: lane (row c16, quarter g) forms outputs g, g + 4, g + 8
      const int rl = c16;
      const int64_t row = r0 + rl;
      for (int c = g; c < DEC_H2; c += 4) {
        float s = w.b2[c];
#pragma unroll 16
        for (int j = 0; j < DEC_H1; ++j) s = fmaf(A1[rl * DEC_A1P + j], w2s[c * DEC_H1 + j], s);
        float a = 0.f;
        if (row < n) {
          if (z2_out) z2_out[row * DEC_H2 + c] = s;
          a = s > 0.f ? s * dec_drop(dc, key, DROP_DEC2, (uint64_t)row * DEC_H2 + c) : 0.f;
        }
        A2[rl * 12 + c] = a;
      }
    }
    __syncthreads();
    if (lane < 16) {  // layer 3
      const int64_t row = r0 + lane;
      if (row < n) {
        float s = w.b3[0];
        for (int c = 0; c < DEC_H2; ++c) s = fmaf(A2[lane * 12 + c], w.w3[c], s);
        y[row] = s;
      }
    }
  }
}

// ---- backward, launch 1 -------------------------------------------------------------------------------------------
// per workgroup partials (floats): [dW2 800 | db2 10 | dW3 10 | db3 1 | db1 80], DEC_PART apart
constexpr int DEC_PART = 904;
constexpr int P_DW2 = 0, P_DB2 = 800, P_DW3 = 810, P_DB3 = 820, P_DB1 = 821, P_END = 901;

__global__ void __launch_bounds__(256) k_decoder_bwd_rows(int64_t n, int d, DecW w, DropCfg dc, const float* __restrict__ z1,
                                                          const float* __restrict__ z2, const float* __restrict__ dy,
                                                          float* __restrict__ dz1_ws, float* __restrict__ part,
                                                          float* __restrict__ dx) {
  __shared__ float w2s[DEC_H2 * DEC_H1];
  __shared__ float dz2s[DEC_ROWS][12];
  __shared__ float a2s[DEC_ROWS][12];
  __shared__ float dys[DEC_ROWS];
  __shared__ float a1s[DEC_ROWS][DEC_A1P];
  __shared__ float dz1s[DEC_ROWS][DEC_A1P];
  const int tid = threadIdx.x;
  const uint64_t key = drop_key(dc);
  for (int i = tid; i < DEC_H2 * DEC_H1; i += blockDim.x) w2s[i] = w.w2[i];
  float acc_w2[4] = {0.f, 0.f, 0.f, 0.f};  // dW2[o], o = tid + 256 q
  float acc_s = 0.f;  // tid < 10: db2[tid]; 16..25: dW3[tid - 16]; 32: db3; 64..143: db1[tid - 64]
  const int64_t ntile = (n + DEC_ROWS - 1) / DEC_ROWS;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int64_t r0 = tile * DEC_ROWS;
    const int rows = (int)min((int64_t)DEC_ROWS, n - r0);
    __syncthreads();  // the previous tile's LDS has been read
    for (int e = tid; e < DEC_ROWS * DEC_H2; e += blockDim.x) {
      const int rl = e / DEC_H2, c = e - rl * DEC_H2;
      float dz = 0.f, a = 0.f;
      if (rl < rows) {
        const int64_t row = r0 + rl;
        const float z = z2[row * DEC_H2 + c];
        const float m = z > 0.f ? dec_drop(dc, key, DROP_DEC2, (uint64_t)row * DEC_H2 + c) : 0.f;
        a = z * m;
        dz = dy[row] * w.w3[c] * m;
      }
      dz2s[rl][c] = dz;
      a2s[rl][c] = a;
    }
    if (tid < DEC_ROWS) dys[tid] = tid < rows ? dy[r0 + tid] : 0.f;
    __syncthreads();
    for (int e = tid; e < DEC_ROWS * DEC_H1; e += blockDim.x) {
      const int rl = e / DEC_H1, j = e - rl * DEC_H1;
      float dz = 0.f, a = 0.f;
      if (rl < rows) {
        const int64_t row = r0 + rl;
        const float z = z1[row * DEC_H1 + j];
        const float m = z > 0.f ? dec_drop(dc, key, DROP_DEC1, (uint64_t)row * DEC_H1 + j) : 0.f;
        a = z * m;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < DEC_H2; ++c) s = fmaf(dz2s[rl][c], w2s[c * DEC_H1 + j], s);
        dz = s * m;
        dz1_ws[row * DEC_H1 + j] = dz;
      }
      a1s[rl][j] = a;
      dz1s[rl][j] = dz;
    }
    __syncthreads();
    // partial sums over this tile's rows, in row order
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int o = tid + 256 * q;
      if (o < DEC_H2 * DEC_H1) {
        const int c = o / DEC_H1, j = o - c * DEC_H1;
        float s = acc_w2[q];
        for (int rl = 0; rl < rows; ++rl) s = fmaf(dz2s[rl][c], a1s[rl][j], s);
        acc_w2[q] = s;
      }
    }
    if (tid < DEC_H2) {
      for (int rl = 0; rl < rows; ++rl) acc_s += dz2s[rl][tid];
    } else if (tid >= 16 && tid < 16 + DEC_H2) {
      for (int rl = 0; rl < rows; ++rl) acc_s = fmaf(dys[rl], a2s[rl][tid - 16], acc_s);
    } else if (tid == 32) {
      for (int rl = 0; rl < rows; ++rl) acc_s += dys[rl];
    } else if (tid >= 64 && tid < 64 + DEC_H1) {
      for (int rl = 0; rl < rows; ++rl) acc_s += dz1s[rl][tid - 64];
    }
    if (dx) {  // dx[row, k] = sum_j dz1[row, j] W1[j, k]: a thread per column k, W1's column in registers
      for (int k = tid; k < d; k += blockDim.x) {
        float wc[DEC_H1];
#pragma unroll
        for (int j = 0; j < DEC_H1; ++j) wc[j] = w.w1[(int64_t)j * d + k];
        for (int rl = 0; rl < rows; ++rl) {
          float s = 0.f;
#pragma unroll
          for (int j = 0; j < DEC_H1; ++j) s = fmaf(dz1s[rl][j], wc[j], s);
          dx[(r0 + rl) * d + k] = s;
        }
      }
    }
  }
  float* p = part + (int64_t)blockIdx.x * DEC_PART;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int o = tid + 256 * q;
    if (o < DEC_H2 * DEC_H1) p[P_DW2 + o] = acc_w2[q];
  }
  if (tid < DEC_H2) p[P_DB2 + tid] = acc_s;
  else if (tid >= 16 && tid < 16 + DEC_H2) p[P_DW3 + tid - 16] = acc_s;
  else if (tid == 32) p[P_DB3] = acc_s;
  else if (tid >= 64 && tid < 64 + DEC_H1) p[P_DB1 + tid - 64] = acc_s;
}

// ---- backward, launch 2: dW1 = dz1^T x (workgroups 0 .. cdiv(d, 64) - 1) and the partials' sums (the last one) ------
__global__ void __launch_bounds__(256) k_decoder_bwd_w1(int64_t n, const float* __restrict__ x, int d,
                                                        const float* __restrict__ dz1, const float* __restrict__ part,
                                                        int nparts, tg_decoder gr) {
  const int tid = threadIdx.x;
  const int ncol = (d + 63) / 64;
  if ((int)blockIdx.x == ncol) {
    for (int o = tid; o < P_END; o += blockDim.x) {
      float s = 0.f;
      for (int b = 0; b < nparts; ++b) s += part[(int64_t)b * DEC_PART + o];
      if (o < P_DB2) gr.w2[o] = s;
      else if (o < P_DW3) gr.b2[o - P_DB2] = s;
      else if (o < P_DB3) gr.w3[o - P_DW3] = s;
      else if (o == P_DB3) gr.b3[0] = s;
      else gr.b1[o - P_DB1] = s;
    }
    return;
  }
  __shared__ float xs[64][65];
  __shared__ float zs[64][DEC_H1];
  const int kl = tid & 63, jg = tid >> 6;  // column of this workgroup's 64; group of 20 hidden units (one per wavefront)
  const int k = blockIdx.x * 64 + kl;
  float acc[20];
#pragma unroll
  for (int j = 0; j < 20; ++j) acc[j] = 0.f;
  for (int64_t r0 = 0; r0 < n; r0 += 64) {
    const int rows = (int)min((int64_t)64, n - r0);
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += blockDim.x) {
      const int rl = e >> 6, c = e & 63;
      const int kk = blockIdx.x * 64 + c;
      xs[rl][c] = (rl < rows && kk < d) ? x[(r0 + rl) * d + kk] : 0.f;
    }
    for (int e = tid; e < 64 * DEC_H1; e += blockDim.x) {
      const int rl = e / DEC_H1, j = e - rl * DEC_H1;
      zs[rl][j] = rl < rows ? dz1[(r0 + rl) * DEC_H1 + j] : 0.f;
    }
    __syncthreads();
    for (int rl = 0; rl < rows; ++rl) {
      const float xv = xs[rl][kl];
#pragma unroll
      for (int j = 0; j < 20; ++j) acc[j] = fmaf(zs[rl][jg * 20 + j], xv, acc[j]);
    }
  }
  if (k < d) {
#pragma unroll
    for (int j = 0; j < 20; ++j) gr.w1[(int64_t)(jg * 20 + j) * d + k] = acc[j];
  }
}

// row-tile workgroups of the backward's first launch: a function of n only (the partials' order is fixed by it)
inline int dec_bwd_parts(int64_t n) { return (int)std::min<int64_t>(cdiv(n, DEC_ROWS), 256); }

// ---- ROC AUC -------------------------------------------------------------------------------------------------------
constexpr int AUC_TILE = 4096;  // keys per workgroup and radix pass
constexpr uint32_t AUC_SENTINEL = 0xffffffffu;  // above orderable(x) of every finite x (at most 0xff7fffff)

// keys, and cnt[0] = finite positives, cnt[1] = finite negatives, cnt[2] = non-finite scores
__global__ void __launch_bounds__(256) k_auc_keys(int64_t n, const float* __restrict__ s, const float* __restrict__ lab,
                                                  uint32_t* __restrict__ keys, unsigned long long* __restrict__ cnt,
                                                  int32_t* __restrict__ n_bad) {
  __shared__ unsigned long long c[3];
  if (threadIdx.x < 3) c[threadIdx.x] = 0ull;
  __syncthreads();
  unsigned long long np = 0, nn = 0, nb = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = s[i] == 0.f ? 0.f : s[i];  // (-0 ties with +0, as in sklearn)
    const bool pos = lab[i] > 0.5f, fin = isfinite(v);
    keys[i] = (fin && !pos) ? (uint32_t)orderable(v) : AUC_SENTINEL;
    np += (fin && pos) ? 1 : 0;
    nn += (fin && !pos) ? 1 : 0;
    nb += fin ? 0 : 1;
  }
  atomicAdd(&c[0], np);
  atomicAdd(&c[1], nn);
  atomicAdd(&c[2], nb);
  __syncthreads();
  if (threadIdx.x < 3) atomicAdd(&cnt[threadIdx.x], c[threadIdx.x]);
  if (threadIdx.x == 0 && n_bad && c[2]) atomicAdd(n_bad, (int32_t)c[2]);
}

// digit histogram of each tile: hist[digit * nblk + tile]
__global__ void __launch_bounds__(256) k_auc_hist(int64_t n, const uint32_t* __restrict__ keys, int shift,
                                                  uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0u;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * AUC_TILE, hi = min(n, lo + AUC_TILE);
  for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
  __syncthreads();
  hist[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of `total` counters in place, one workgroup of 1024 threads
__global__ void __launch_bounds__(1024) k_auc_scan(uint32_t* __restrict__ v, int64_t total) {
  __shared__ uint32_t sums[1024];
  const int64_t per = (total + 1023) / 1024;
  const int64_t lo = min(total, (int64_t)threadIdx.x * per), hi = min(total, lo + per);
  uint32_t s = 0;
  for (int64_t i = lo; i < hi; ++i) s += v[i];
  sums[threadIdx.x] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan of the 1024 sums
    const uint32_t t = threadIdx.x >= (unsigned)o ? sums[threadIdx.x - o] : 0u;
    __syncthreads();
    sums[threadIdx.x] += t;
    __syncthreads();
  }
  uint32_t run = sums[threadIdx.x] - s;
  for (int64_t i = lo; i < hi; ++i) {
    const uint32_t c = v[i];
    v[i] = run;
    run += c;
  }
}

// stable scatter of each tile by digit: one wavefront per workgroup walks its tile 64 keys at a time; lanes with the
// same digit find each other with eight ballots and take consecutive slots in lane order
__global__ void __launch_bounds__(64) k_auc_scatter(int64_t n, const uint32_t* __restrict__ in, int shift,
                                                    const uint32_t* __restrict__ offs, uint32_t* __restrict__ out) {
  __shared__ uint32_t base[256];
  const int lane = threadIdx.x;
  for (int dg = lane; dg < 256; dg += 64) base[dg] = offs[(int64_t)dg * gridDim.x + blockIdx.x];
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * AUC_TILE, hi = min(n, lo + AUC_TILE);
  const uint64_t lt = (1ull << lane) - 1ull;
  for (int64_t i0 = lo; i0 < hi; i0 += 64) {
    const int64_t i = i0 + lane;
    const bool valid = i < hi;
    const uint32_t k = valid ? in[i] : 0u;
    const uint32_t dg = (k >> shift) & 255u;
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const uint32_t bit = (dg >> b) & 1u;
      const uint64_t bb = __ballot(bit);
      peers &= bit ? bb : ~bb;
    }
    const uint32_t rank = (uint32_t)__popcll(peers & lt);
    const uint32_t cnt = (uint32_t)__popcll(peers);
    const uint32_t b0 = valid ? base[dg] : 0u;
    __syncthreads();  // every lane has read its digit's base
    if (valid) {
      out[b0 + rank] = k;
      if (rank == 0) base[dg] = b0 + cnt;
    }
    __syncthreads();
  }
}

__device__ __forceinline__ int64_t lower_bound_u32(const uint32_t* a, int64_t len, uint32_t v) {
  int64_t lo = 0, hi = len;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// every finite positive: 2 #(neg < s) + #(neg == s), summed as integers into cnt[3]
__global__ void __launch_bounds__(256) k_auc_count(int64_t n, const float* __restrict__ s, const float* __restrict__ lab,
                                                   const uint32_t* __restrict__ sorted, unsigned long long* __restrict__ cnt) {
  __shared__ unsigned long long tot;
  if (threadIdx.x == 0) tot = 0ull;
  __syncthreads();
  const int64_t nneg = (int64_t)cnt[1];
  unsigned long long acc = 0ull;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = s[i] == 0.f ? 0.f : s[i];
    if (!(lab[i] > 0.5f) || !isfinite(v)) continue;
    const uint32_t k = (uint32_t)orderable(v);
    const int64_t l = lower_bound_u32(sorted, nneg, k);
    const int64_t u = lower_bound_u32(sorted, nneg, k + 1u);  // (k + 1 <= 0xff800000: no wrap for finite scores)
    acc += (unsigned long long)(2 * l + (u - l));
  }
  atomicAdd(&tot, acc);
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(&cnt[3], tot);
}

// NaN when a class is empty (sklearn raises there; the caller does)
__global__ void k_auc_final(const unsigned long long* __restrict__ cnt, double* __restrict__ auc) {
  const double P = (double)cnt[0], N = (double)cnt[1];
  *auc = (P > 0.0 && N > 0.0) ? (double)cnt[3] / (2.0 * P * N) : __longlong_as_double(0x7ff8000000000000ll);
}

struct AucWs {
  uint32_t *a, *b, *hist;
  unsigned long long* cnt;
};
inline size_t auc_layout(int64_t n, char* base, AucWs* w) {
  const int64_t nblk = cdiv(n, AUC_TILE);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return base ? base + o : nullptr;
  };
  char* cnt = take(4 * sizeof(unsigned long long));
  char* a = take((size_t)n * 4);
  char* b = take((size_t)n * 4);
  char* h = take((size_t)nblk * 256 * 4);
  if (w) *w = AucWs{(uint32_t*)a, (uint32_t*)b, (uint32_t*)h, (unsigned long long*)cnt};
  return off;
}

}  // namespace tg

using namespace tg;

static bool dec_args_ok(int64_t n, const float* x, int32_t d, const tg_decoder* w) {
  return n >= 0 && d > 0 && d % 4 == 0 && d <= TG_DECODER_MAX_D && w && w->w1 && w->b1 && w->w2 && w->b2 && w->w3 &&
         w->b3 && (n == 0 || x);
}

static bool dec_drop_ok(float p, const uint64_t* rng) { return p >= 0.f && p < 1.f && (p == 0.f || rng); }

// the forward's dynamic LDS exceeds the 64 KB default of a launch
static int dec_lds_attr() {
  static int done = 0;  // (per process; the attribute belongs to the function, whichever device runs it)
  if (done) return TG_OK;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_decoder_fwd),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)DEC_FWD_LDS);
  if (e != hipSuccess) {
    set_hip_error(e, "tg_decoder_fwd: hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
    return TG_EHIP;
  }
  done = 1;
  return TG_OK;
}

extern "C" int tg_decoder_fwd(int64_t n, const float* x, int32_t d, const tg_decoder* w, float dropout_p,
                              const uint64_t* rng, float* y, float* z1, float* z2, void* stream) {
  if (!dec_args_ok(n, x, d, w) || !dec_drop_ok(dropout_p, rng) || (n > 0 && !y)) return TG_EINVAL;
  if (n == 0) return TG_OK;
  const int rc = dec_lds_attr();
  if (rc) return rc;
  const DecW dw{w->w1, w->b1, w->w2, w->b2, w->w3, w->b3};
  const unsigned grid = (unsigned)std::min<int64_t>(cdiv(n, DEC_ROWS), 1024);
  hipLaunchKernelGGL(k_decoder_fwd, dim3(grid), dim3(256), DEC_FWD_LDS, as_stream(stream), n, x, (int)d, dw,
                     make_drop(dropout_p, rng), y, z1, z2);
  return check_launch("tg_decoder_fwd");
}

extern "C" size_t tg_decoder_bwd_workspace_bytes(int64_t n, int32_t d) {
  if (n < 0 || d <= 0) return 0;
  return (size_t)n * DEC_H1 * 4 + (size_t)std::max(1, dec_bwd_parts(n)) * DEC_PART * 4;
}

extern "C" int tg_decoder_bwd(int64_t n, const float* x, int32_t d, const tg_decoder* w, float dropout_p,
                              const uint64_t* rng, const float* z1, const float* z2, const float* dy,
                              const tg_decoder* grads, float* dx, void* ws, size_t ws_bytes, void* stream) {
  if (!dec_args_ok(n, x, d, w) || !dec_drop_ok(dropout_p, rng) || !grads || !grads->w1 || !grads->b1 || !grads->w2 ||
      !grads->b2 || !grads->w3 || !grads->b3 || (n > 0 && (!z1 || !z2 || !dy)))
    return TG_EINVAL;
  if (n > 0 && (!ws || ws_bytes < tg_decoder_bwd_workspace_bytes(n, d))) return TG_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  const DecW dw{w->w1, w->b1, w->w2, w->b2, w->w3, w->b3};
  float* dz1 = static_cast<float*>(ws);
  float* part = n > 0 ? dz1 + n * DEC_H1 : nullptr;
  const int parts = dec_bwd_parts(n);
  if (parts > 0) {
    hipLaunchKernelGGL(k_decoder_bwd_rows, dim3(parts), dim3(256), 0, st, n, (int)d, dw, make_drop(dropout_p, rng), z1, z2,
                       dy, dz1, part, dx);
    const int rc = check_launch("tg_decoder_bwd");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_decoder_bwd_w1, dim3((unsigned)cdiv(d, 64) + 1), dim3(256), 0, st, n, x, (int)d, dz1, part, parts,
                     *grads);
  return check_launch("tg_decoder_bwd");
}

extern "C" size_t tg_roc_auc_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  return auc_layout(n, nullptr, nullptr);
}

extern "C" int tg_roc_auc(int64_t n, const float* scores, const float* labels, double* auc, int32_t* n_nonfinite, void* ws,
                          size_t ws_bytes, void* stream) {
  if (n < 0 || n > ((int64_t)1 << 31) - 1 || !auc || (n > 0 && (!scores || !labels))) return TG_EINVAL;
  if (!ws || ws_bytes < tg_roc_auc_workspace_bytes(n)) return TG_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  AucWs w;
  auc_layout(n, static_cast<char*>(ws), &w);
  const hipError_t e = hipMemsetAsync(w.cnt, 0, 4 * sizeof(unsigned long long), st);
  if (e != hipSuccess) {
    set_hip_error(e, "tg_roc_auc");
    return TG_EHIP;
  }
  if (n > 0) {
    const int64_t nblk = cdiv(n, AUC_TILE);
    hipLaunchKernelGGL(k_auc_keys, dim3(flat_grid(n, 256)), dim3(256), 0, st, n, scores, labels, w.a, w.cnt, n_nonfinite);
    uint32_t *src = w.a, *dst = w.b;
    for (int shift = 0; shift < 32; shift += 8) {
      hipLaunchKernelGGL(k_auc_hist, dim3((unsigned)nblk), dim3(256), 0, st, n, src, shift, w.hist);
      hipLaunchKernelGGL(k_auc_scan, dim3(1), dim3(1024), 0, st, w.hist, nblk * 256);
      hipLaunchKernelGGL(k_auc_scatter, dim3((unsigned)nblk), dim3(64), 0, st, n, src, shift, w.hist, dst);
      std::swap(src, dst);
    }
    hipLaunchKernelGGL(k_auc_count, dim3(flat_grid(n, 256)), dim3(256), 0, st, n, scores, labels, src, w.cnt);
  }
  hipLaunchKernelGGL(k_auc_final, dim3(1), dim3(1), 0, st, w.cnt, auc);
  return check_launch("tg_roc_auc");
}
