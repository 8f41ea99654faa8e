// Embedding nearest neighbours: the k best catalogue rows of every query row by inner product, selected on the MFMA
// accumulators - the [Q, C] score matrix is never written.  No reference counterpart; the leave-out rules, the keys and
// the order are tg_topk_rows's (tg_topk_keys.h), the float32 chain is the one tg_rank_cand_half relies on.
//
// k_knn_tiles.  Grid: (query tiles) x (catalogue splits), one workgroup each, no workgroup waits for another.  A workgroup
// of NW wavefronts keeps NW x 32 query rows resident in LDS for its whole life (NW = 4: TG_KNN_Q_TILE rows, while
// 128 (d + 2) floats and the catalogue ring fit the 160 KiB; NW = 2 for wider rows) and streams the catalogue tiles of its
// split, TG_KNN_C_TILE = 64 columns at a time in chunks of 32 k: 16-byte loads into registers one chunk ahead, written to
// the other half of a two-chunk LDS ring behind the products, one barrier per chunk.  Wavefront w multiplies its 32 query
// rows with the tile's two 32-column blocks: two independent v_mfma_f32_32x32x2_f32 chains, each ONE chain per (row, column)
// from accumulator 0 with k ascending, two k per instruction - bit for bit s = fmaf(q[i, k], c[j, k], s).  Both LDS images
// hold every four k as (k0, k2, k1, k3), so that lane half h fetches its operands of two consecutive instructions (k = 4g + h,
// 4g + 2 + h) with one 8-byte read; rows are d + 2 (34) floats apart, which spreads the 32 rows of a half over all 64 banks.
// After a tile's last chunk the accumulators are scaled, turned into keys and compared with their row's threshold - the
// current k-th best key of the row.  The row lists live in registers: a wavefront owns its 32 rows, lane p holds the p-th
// best key of each (32 x 64-bit registers), and only keys that beat the threshold are inserted (tg_topk_keys.h: one
// cross-lane shift each).  Once the lists have warmed up insertions are rare; a row of ascending scores inserts every
// column: correct, and slow.  The order is total, so which lane met which column, the tile order and the split do not
// show in the result.  Every (row, split) leaves its best k keys and two counts in the workspace.
// k_knn_merge.  One wavefront per row merges the n_split x k keys by the same insertion and writes ids, scores and columns.
// A score comes back out of its key; the key has lost the sign of a zero, so a zero score is recomputed by the scalar chain.
#include <algorithm>
#include <cmath>
#include <vector>

#include "tg_topk_keys.h"

namespace tg {

typedef float knn_f32x16 __attribute__((ext_vector_type(16)));

constexpr int KN_CT = TG_KNN_C_TILE;  // catalogue columns of a tile: two 32-column MFMA blocks
constexpr int KN_KC = 32;             // k extent of a staged chunk
constexpr int KN_LDC = KN_KC + 2;     // floats between the rows of a staged chunk
constexpr int KN_MWPB = 4;            // wavefronts of a merge workgroup
constexpr size_t KN_LDS_MAX = 160 * 1024;
constexpr size_t KN_RING_BYTES = 2 * KN_CT * KN_LDC * sizeof(float);

static_assert(KN_CT == 64 && TG_KNN_Q_TILE == 128, "k_knn_tiles: 4 wavefronts x 32 rows against 2 x 32 columns");

struct KnnArgs {
  int64_t Q, C, ldq, ldc, tiles_per_split;
  int d, k, ns, aligned;
  const float* q;
  const float* c;
  const int64_t* ids;
  const float* qs;
  const float* cs;
  const int64_t* excl;
  const uint8_t* mask;
  int64_t* out_ids;
  float* out_scores;
  int32_t* out_cols;
  int32_t* n_valid;
  int64_t* n_nonfinite;
  uint64_t* ws_keys;  // [Q, ns, k]
  int32_t* ws_cnt;    // [Q, ns, 2]: columns left in, non-finite scores met
};

static size_t knn_lds_bytes(int nw, int d) { return (size_t)nw * 32 * (size_t)(d + 2) * sizeof(float) + KN_RING_BYTES; }
static int knn_waves(int d) { return knn_lds_bytes(4, d) <= KN_LDS_MAX ? 4 : 2; }

__device__ __forceinline__ float4 knn_ld4(const float* p, int aligned) {
  if (aligned) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}
// four consecutive k as (k0, k2, k1, k3)
__device__ __forceinline__ void knn_st4(float* p, float4 v) {
  *reinterpret_cast<float2*>(p) = make_float2(v.x, v.z);
  *reinterpret_cast<float2*>(p + 2) = make_float2(v.y, v.w);
}

// topk_insert for the lanes of `todo` only
__device__ __forceinline__ void knn_insert(uint64_t& best, uint64_t key, unsigned long long todo, int kth, int lane) {
  uint64_t thr = lane_bcast(best, kth);
  while (todo) {  // wave-uniform, at most 32 rounds
    const int src = __builtin_amdgcn_readfirstlane(__ffsll(todo) - 1);
    todo &= todo - 1;
    const uint64_t x = lane_bcast(key, src);
    if (x > thr) {
      const uint64_t up = __shfl_up(best, 1);
      if (best < x) best = (lane == 0 || up > x) ? x : up;
      thr = lane_bcast(best, kth);
    }
  }
}

template <int NW>
__global__ void __launch_bounds__(NW * TG_WAVE) k_knn_tiles(KnnArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
  constexpr int NT = NW * TG_WAVE, QT = NW * 32;
  constexpr int PER = KN_CT * (KN_KC / 4) / NT;  // float4 pieces of a chunk per thread
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 31, fk = lane >> 5;
  const int ldqs = a.d + 2;
  float* Qs = reinterpret_cast<float*>(knn_lds);  // [QT][d + 2]
  float* Cs = Qs + QT * ldqs;                     // [2][KN_CT][KN_LDC]
  const int64_t qt = blockIdx.x / a.ns;
  const int split = (int)(blockIdx.x - qt * a.ns);
  const int64_t row0 = qt * QT + wave * 32;  // this wavefront's first query row
  const int64_t n_tiles = (a.C + KN_CT - 1) / KN_CT;
  const int64_t t_lo = min(n_tiles, split * a.tiles_per_split), t_hi = min(n_tiles, t_lo + a.tiles_per_split);
  const int nchunk = (a.d + KN_KC - 1) / KN_KC;
  const int64_t T = (t_hi - t_lo) * nchunk;  // chunks of this workgroup, tile-major
  const int kth = a.k - 1;

  uint64_t best[32];
#pragma unroll
  for (int r = 0; r < 32; ++r) best[r] = 0;
  int nvv = 0, badv = 0;  // lane r < 32: the counts of row r

  if (T > 0) {  // block-uniform
    const int d4 = a.d >> 2;
    for (int i = tid; i < QT * d4; i += NT) {
      const int r = i / d4, g = i - r * d4;
      const int64_t gr = min(qt * QT + r, a.Q - 1);  // rows past Q repeat the last one; they select nothing
      knn_st4(Qs + r * ldqs + 4 * g, knn_ld4(a.q + gr * a.ldq + 4 * g, a.aligned));
    }
    float qsr[16];
    int64_t exr[16];
    uint32_t rowbits = 0;  // bit r: accumulator register r of this lane is a row below Q (rows past Q select nothing)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t lr = row0 + (r & 3) + 8 * (r >> 2) + 4 * fk;
      rowbits |= (lr < a.Q ? 1u : 0u) << r;
      const int64_t gr = min(lr, a.Q - 1);
      qsr[r] = a.qs ? a.qs[gr] : 1.0f;  // x * 1.0f is x
      exr[r] = a.excl ? a.excl[gr] : 0;  // id 0 is left out anyway
    }

    float4 st[PER];
    auto load_chunk = [&](int64_t tile, int kc) {
#pragma unroll
      for (int p = 0; p < PER; ++p) {
        const int j = tid + p * NT;
        const int64_t col = min(tile * KN_CT + (j >> 3), a.C - 1);  // columns past C repeat the last one: left out below
        const int kk = min(kc * KN_KC + 4 * (j & 7), a.d - 4);      // pieces past d repeat the last one: never multiplied
        st[p] = knn_ld4(a.c + col * a.ldc + kk, a.aligned);
      }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
      for (int p = 0; p < PER; ++p) {
        const int j = tid + p * NT;
        knn_st4(Cs + (buf * KN_CT + (j >> 3)) * KN_LDC + 4 * (j & 7), st[p]);
      }
    };

    load_chunk(t_lo, 0);
    store_chunk(0);
    __syncthreads();

    knn_f32x16 acc0 = {}, acc1 = {};
    int64_t idv[2] = {0, 0};
    float csv[2] = {1.0f, 1.0f};
    bool okv[2] = {false, false};
    uint32_t cjv[2] = {0, 0};
    int64_t tile = t_lo;
    int kc = 0;
    for (int64_t it = 0; it < T; ++it) {
      const int buf = (int)(it & 1);
      int64_t ntile = tile;
      int nkc = kc + 1;
      if (nkc == nchunk) { nkc = 0; ++ntile; }
      const bool more = it + 1 < T;
      if (more) load_chunk(ntile, nkc);
      if (kc == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int64_t cj = tile * KN_CT + b * 32 + fr;
          const int64_t cc = min(cj, a.C - 1);
          cjv[b] = (uint32_t)cc;
          idv[b] = a.ids ? a.ids[cc] : cc + 1;
          csv[b] = a.cs ? a.cs[cc] : 1.0f;
          okv[b] = cj < a.C && idv[b] != 0 && (!a.mask || a.mask[cc]);
        }
      }
      {
        const int n4 = min(KN_KC, a.d - kc * KN_KC) >> 2;  // groups of four k: two instructions per chain
        const float* ap = Qs + (wave * 32 + fr) * ldqs + kc * KN_KC + 2 * fk;
        const float* b0p = Cs + (buf * KN_CT + fr) * KN_LDC + 2 * fk;
        const float* b1p = b0p + 32 * KN_LDC;
        float2 av = *reinterpret_cast<const float2*>(ap);
        float2 b0 = *reinterpret_cast<const float2*>(b0p);
        float2 b1 = *reinterpret_cast<const float2*>(b1p);
        for (int g = 0; g < n4; ++g) {  // the operands of group g + 1 are fetched behind the products of group g
          const int gn = 4 * min(g + 1, n4 - 1);
          const float2 nav = *reinterpret_cast<const float2*>(ap + gn);
          const float2 nb0 = *reinterpret_cast<const float2*>(b0p + gn);
          const float2 nb1 = *reinterpret_cast<const float2*>(b1p + gn);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b0.x, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b1.x, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b0.y, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b1.y, acc1, 0, 0, 0);
          av = nav; b0 = nb0; b1 = nb1;
        }
      }
      if (more) store_chunk(buf ^ 1);  // last read before the barrier that ended chunk it - 1
      if (kc == nchunk - 1) {
        // accumulator register r of lane half fk is row (r & 3) + 8 (r >> 2) + 4 fk, column fr of its block
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rA = (r & 3) + 8 * (r >> 2), rB = rA + 4;
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            float s = b ? acc1[r] : acc0[r];
            s = s * qsr[r];
            s = s * csv[b];
            const uint32_t u = __float_as_uint(s);
            const bool in = okv[b] && idv[b] != exr[r] && ((rowbits >> r) & 1u);
            const bool fin = topk_finite(u);
            const uint64_t key = (in && fin) ? topk_key(u, cjv[b]) : 0ull;
            const unsigned long long bi = __ballot(in && fin), bb = __ballot(in && !fin);
            nvv += lane == rA ? __popc((uint32_t)bi) : (lane == rB ? __popc((uint32_t)(bi >> 32)) : 0);
            if (bb) badv += lane == rA ? __popc((uint32_t)bb) : (lane == rB ? __popc((uint32_t)(bb >> 32)) : 0);
            const uint64_t thrA = lane_bcast(best[rA], kth), thrB = lane_bcast(best[rB], kth);
            const unsigned long long hit = __ballot(key > (fk ? thrB : thrA));
            if (hit) {  // wave-uniform; rare once the lists have warmed up
              knn_insert(best[rA], key, hit & 0xffffffffull, kth, lane);
              knn_insert(best[rB], key, hit & ~0xffffffffull, kth, lane);
            }
          }
        }
      }
      __syncthreads();
      tile = ntile;
      kc = nkc;
    }
  }

#pragma unroll
  for (int r = 0; r < 32; ++r) {
    const int64_t gr = row0 + r;
    if (gr < a.Q && lane < a.k) a.ws_keys[(gr * a.ns + split) * a.k + lane] = best[r];
  }
  if (lane < 32 && row0 + lane < a.Q) {
    const int64_t w = (row0 + lane) * a.ns + split;
    a.ws_cnt[2 * w] = nvv;
    a.ws_cnt[2 * w + 1] = badv;
  }
}

__global__ void __launch_bounds__(KN_MWPB * TG_WAVE) k_knn_merge(KnnArgs a) {
  const int lane = lane_id();
  const int64_t row = (int64_t)blockIdx.x * KN_MWPB + threadIdx.x / TG_WAVE;
  if (row >= a.Q) return;  // wave-uniform
  const int64_t n = (int64_t)a.ns * a.k;
  const uint64_t* keys = a.ws_keys + row * n;
  uint64_t best = 0;
  for (int64_t i0 = 0; i0 < n; i0 += TG_WAVE) {
    const int64_t i = i0 + lane;
    topk_insert(best, i < n ? keys[i] : 0ull, a.k - 1, lane);
  }
  int nv = 0, bad = 0;
  for (int64_t s = lane; s < a.ns; s += TG_WAVE) {
    nv += a.ws_cnt[2 * (row * a.ns + s)];
    bad += a.ws_cnt[2 * (row * a.ns + s) + 1];
  }
  for (int off = TG_WAVE / 2; off >= 1; off >>= 1) {
    nv += __shfl_xor(nv, off);
    bad += __shfl_xor(bad, off);
  }
  if (lane < a.k) {
    int64_t id = 0;
    float s = -INFINITY;
    int32_t col = -1;
    if (best) {
      col = (int32_t)~(uint32_t)best;
      id = a.ids ? a.ids[col] : (int64_t)col + 1;
      const uint32_t o = (uint32_t)(best >> 32);
      const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
      if ((u << 1) != 0) {
        s = __uint_as_float(u);
      } else {  // the key has lost the sign of a zero
        const float* qr = a.q + row * a.ldq;
        const float* cr = a.c + (int64_t)col * a.ldc;
        s = 0.0f;
        for (int kk = 0; kk < a.d; ++kk) s = fmaf(qr[kk], cr[kk], s);
        if (a.qs) s = s * a.qs[row];
        if (a.cs) s = s * a.cs[col];
      }
    }
    a.out_ids[row * a.k + lane] = id;
    a.out_scores[row * a.k + lane] = s;
    a.out_cols[row * a.k + lane] = col;
  }
  if (lane == 0) {
    a.n_valid[row] = nv;
    // the one integer sum over rows, as tg_topk_rows keeps it: its value does not depend on the order of the additions
    if (bad) atomicAdd(reinterpret_cast<unsigned long long*>(a.n_nonfinite), (unsigned long long)bad);
  }
}

// splits chosen by the library: about two workgroups per CU over the nominal query tiles, at least four catalogue tiles
// each.  (Q and C only: tg_knn_rows_workspace_bytes has to make the same choice without d.)
static int64_t knn_choose_splits(int64_t Q, int64_t C) {
  if (Q <= 0 || C <= 0) return 1;
  const int64_t qt = cdiv(Q, TG_KNN_Q_TILE), tiles = cdiv(C, KN_CT);
  return std::max<int64_t>(1, std::min<int64_t>(512 / std::min<int64_t>(qt, 512), tiles / 4));
}

static int64_t knn_splits(int64_t Q, int64_t C, int32_t n_split) {
  return (Q == 0 || C == 0) ? 1 : (n_split > 0 ? (int64_t)n_split : knn_choose_splits(Q, C));
}

static int knn_args_check(int64_t Q, int64_t C, int32_t d, int32_t k, int64_t ldq, int64_t ldc, int32_t n_split) {
  if (Q < 0 || C < 0 || C > 0x7fffffffLL || d < 0 || k < 1 || k > TG_TOPK_MAX_K || ldq < d || ldc < d || n_split < 0)
    return TG_EINVAL;
  if (Q > 0 && std::max<int64_t>(n_split, 1) > 0x7fffffffLL / cdiv(Q, 64)) return TG_EINVAL;  // workgroups in one grid
  if (d == 0 || d % 4 != 0 || d > 512) return TG_EUNSUPPORTED;
  return TG_OK;
}

static int knn_lds_attr() {
  static int done = 0;  // (per process; the attribute belongs to the function, whichever device runs it)
  if (done) return TG_OK;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_knn_tiles<4>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)KN_LDS_MAX);
  if (e == hipSuccess)
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_knn_tiles<2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)KN_LDS_MAX);
  if (e != hipSuccess) {
    set_hip_error(e, "tg_knn_rows: hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
    return TG_EHIP;
  }
  done = 1;
  return TG_OK;
}

}  // namespace tg

using namespace tg;

extern "C" size_t tg_knn_rows_workspace_bytes(int64_t Q, int64_t C, int32_t k, int32_t n_split) {
  if (knn_args_check(Q, C, 4, k, 4, 4, n_split) != TG_OK) return 0;
  return (size_t)Q * (size_t)knn_splits(Q, C, n_split) * ((size_t)k * sizeof(uint64_t) + 2 * sizeof(int32_t));
}

extern "C" int tg_knn_rows(int64_t Q, int64_t C, int32_t d, int32_t k, const float* q, int64_t ldq, const float* c,
                           int64_t ldc, const int64_t* ids, const float* q_scale, const float* c_scale,
                           const int64_t* exclude, const uint8_t* col_mask, int32_t n_split, int64_t* out_ids,
                           float* out_scores, int32_t* out_cols, int32_t* n_valid, int64_t* n_nonfinite, void* ws,
                           size_t ws_bytes, void* stream) {
  if (int rc = knn_args_check(Q, C, d, k, ldq, ldc, n_split)) return rc;
  if (Q == 0) return TG_OK;
  if (!out_ids || !out_scores || !out_cols || !n_valid || !n_nonfinite || (C > 0 && (!q || !c))) return TG_EINVAL;
  const int64_t ns = knn_splits(Q, C, n_split);
  const size_t need = tg_knn_rows_workspace_bytes(Q, C, k, n_split);
  if (!ws || ws_bytes < need) return TG_EWORKSPACE;
  if (reinterpret_cast<uintptr_t>(ws) & 7) return TG_EINVAL;
  if (int rc = knn_lds_attr()) return rc;
  hipStream_t st = as_stream(stream);
  KnnArgs a{};
  a.Q = Q; a.C = C; a.ldq = ldq; a.ldc = ldc;
  a.tiles_per_split = cdiv(std::max<int64_t>(cdiv(C, KN_CT), 1), ns);
  a.d = d; a.k = k; a.ns = (int)ns;
  // rows on 16-byte boundaries take 16-byte loads; any other base or stride takes the scalar-load path
  a.aligned = ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(c)) & 15) == 0 && ldq % 4 == 0 && ldc % 4 == 0;
  a.q = q; a.c = c; a.ids = ids; a.qs = q_scale; a.cs = c_scale; a.excl = exclude; a.mask = col_mask;
  a.out_ids = out_ids; a.out_scores = out_scores; a.out_cols = out_cols; a.n_valid = n_valid; a.n_nonfinite = n_nonfinite;
  a.ws_keys = static_cast<uint64_t*>(ws);
  a.ws_cnt = reinterpret_cast<int32_t*>(a.ws_keys + Q * ns * k);
  const int nw = knn_waves(d);
  const unsigned grid = (unsigned)(cdiv(Q, nw * 32) * ns);
  if (nw == 4)
    hipLaunchKernelGGL(k_knn_tiles<4>, dim3(grid), dim3(4 * TG_WAVE), knn_lds_bytes(4, d), st, a);
  else
    hipLaunchKernelGGL(k_knn_tiles<2>, dim3(grid), dim3(2 * TG_WAVE), knn_lds_bytes(2, d), st, a);
  if (int rc = check_launch("tg_knn_rows(tiles)")) return rc;
  hipLaunchKernelGGL(k_knn_merge, dim3((unsigned)cdiv(Q, KN_MWPB)), dim3(KN_MWPB * TG_WAVE), 0, st, a);
  return check_launch("tg_knn_rows(merge)");
}

extern "C" int tg_knn_rows_host(int64_t Q, int64_t C, int32_t d, int32_t k, const float* q, int64_t ldq, const float* c,
                                int64_t ldc, const int64_t* ids, const float* q_scale, const float* c_scale,
                                const int64_t* exclude, const uint8_t* col_mask, int32_t n_split, int64_t* out_ids,
                                float* out_scores, int32_t* out_cols, int32_t* n_valid, int64_t* n_nonfinite,
                                float* scores_out_host) {
  if (int rc = knn_args_check(Q, C, d, k, ldq, ldc, n_split)) return rc;
  if (Q == 0) return TG_OK;
  if (!out_ids || !out_scores || !out_cols || !n_valid || !n_nonfinite || (C > 0 && (!q || !c))) return TG_EINVAL;
  std::vector<uint64_t> keys;
  std::vector<float> srow((size_t)C);
  for (int64_t i = 0; i < Q; ++i) {
    keys.clear();
    int64_t bad = 0;
    for (int64_t j = 0; j < C; ++j) {
      float s = 0.0f;
      for (int32_t kk = 0; kk < d; ++kk) s = fmaf(q[i * ldq + kk], c[j * ldc + kk], s);
      if (q_scale) s = s * q_scale[i];
      if (c_scale) s = s * c_scale[j];
      srow[(size_t)j] = s;
      if (scores_out_host) scores_out_host[i * C + j] = s;
      const int64_t id = ids ? ids[j] : j + 1;
      if (id == 0 || (col_mask && !col_mask[j]) || (exclude && id == exclude[i])) continue;
      const uint32_t u = __builtin_bit_cast(uint32_t, s);
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
      out_ids[i * k + p] = live ? (ids ? ids[col] : (int64_t)col + 1) : 0;
      out_scores[i * k + p] = live ? srow[(size_t)col] : -INFINITY;
      out_cols[i * k + p] = col;
    }
    n_valid[i] = (int32_t)keys.size();
    *n_nonfinite += bad;
  }
  return TG_OK;
}
