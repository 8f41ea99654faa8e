// The one-layer temporal graph attention (tiger/model/temporal_agg_modules.py:29-83,186-235): STEP 3 of
// TIGE.contrast_learning, as the streaming step, the training step and the operator exports run it.  SURVEY.md K8; a15-a18.
//
// Attention is restructured around the fact that there is ONE query per centre and K
// keys: instead of projecting every key/value row (24*K*d^2 flop per centre) the query
// is folded through Wk (g_h = Wk_h^T q_h), scores are plain dot products with the raw
// key rows, the softmax-weighted raw rows are summed first and projected through Wv
// once.  q.bk is constant over keys and cancels in the softmax; sum(a)=1 carries bv.
// Mathematically identical, ~5x fewer flops, and the K*3d key rows are touched once by
// a gather kernel instead of being materialised for a GEMM.
#include "tg_step.h"
#include "tg_sample.h"
#include "tg_profile.h"

namespace tg {

// centre rows: c_i = reprs[local(nid_i)] + nfeat[nid_i]   (temporal_agg_modules.py:48-50)
// The last `qblocks` blocks of the grid instead compute the constant half of the query
// projection, qconst[n] = bq[n] + sum_j Wq[n, d + j] * cos(phase[j])   (TE(0) = cos(phi)).
__global__ void __launch_bounds__(256) k_attn_centres(int64_t Q, int d4, const int64_t* __restrict__ nids,
                                                      const float4* __restrict__ reprs, const uint64_t* __restrict__ bm,
                                                      const uint32_t* __restrict__ rank, const float4* __restrict__ nf,
                                                      float4* __restrict__ out, int qblocks, const float* __restrict__ wq,
                                                      const float* __restrict__ bq, const float* __restrict__ freq,
                                                      const float* __restrict__ phase, float* __restrict__ qconst,
                                                      PosArgs pos) {
  const int cblocks = (int)gridDim.x - qblocks;
  if (pos.best && (int)blockIdx.x < cblocks)  // second dedup pass rides on the centre blocks
    pos_winners_pass(pos, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)cblocks * blockDim.x);
  if ((int)blockIdx.x >= cblocks) {
    const int d = d4 * 4, lane = lane_id();
    const int n = ((int)blockIdx.x - cblocks) * 4 + (threadIdx.x >> 6);
    if (n >= 2 * d) return;
    float acc = 0.f;
    for (int j = lane; j < d; j += TG_WAVE) acc += wq[(int64_t)n * 2 * d + d + j] * time_enc(0.f, freq[j], phase[j]);
    acc = wave_sum(acc);
    if (lane == 0) qconst[n] = acc + bq[n];
    return;
  }
  const int64_t total = Q * d4;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)cblocks * blockDim.x) {
    const int64_t i = t / d4;
    const int c = (int)(t - i * d4);
    const int64_t id = nids[i];
    float4 v = reprs[(int64_t)bm_rank(bm, rank, id) * d4 + c];
    if (nf) {
      const float4 f = nf[id * d4 + c];
      v.x += f.x; v.y += f.y; v.z += f.z; v.w += f.w;
    }
    out[t] = v;
  }
}

__global__ void __launch_bounds__(256) k_attn_centres_direct(tg_model m, int64_t Q, const int64_t* __restrict__ nids,
                                                             const float4* __restrict__ nf, float4* __restrict__ out,
                                                             DirectArgs da, PosArgs pos) {
  centres_direct_body(m, Q, ArrayIds{nids, pos.ts}, nf, out, da, pos,
                      (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// explicit fma: the library is built with -ffp-contract=off (only the time encoding needs the
// unfused product), so contractions are spelled out where they are wanted
__device__ __forceinline__ float dot4(float4 a, float4 b, float acc) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc))));
}
__device__ __forceinline__ void axpy4(float4& s, float b, float4 x) {
  s.x = fmaf(b, x.x, s.x);
  s.y = fmaf(b, x.y, s.y);
  s.z = fmaf(b, x.z, s.z);
  s.w = fmaf(b, x.w, s.w);
}
__device__ __forceinline__ void scale4(float4& s, float a) {
  s.x *= a; s.y *= a; s.z *= a; s.w *= a;
}

// One wavefront per centre.  Streams its K neighbour rows once: node part
// reprs[local]+nfeat, edge part efeat, time part cos(dt*w+phi); per head an online
// softmax over the keys accumulates the weighted raw row.  A lane owns W consecutive columns
// of every segment (NV such groups, i.e. widths up to 64*W*NV); W is picked per model so that
// the 64 lanes are as full as possible: the kernel is VALU-bound (time encoding + 2*NH fmas per
// column and key), and d = 172 fills 43 lanes as float4 but 58 lanes as three floats.
// Latency structure: lane k first resolves key k's metadata (neighbour id -> local row via
// the rank popcount, edge id, dt) for all K keys at once, the per-key loop then only
// broadcasts it, and the raw rows of the next keys are requested before key k is reduced.
template <int W>
struct RowVec {
  float a[W];
};
struct __attribute__((packed, aligned(4))) F3 {
  float x, y, z;
};
// columns [col, col+W) of a row of `width` floats (row 16-byte aligned, width % 4 == 0); zeros past the end
template <int W>
__device__ __forceinline__ RowVec<W> row_load(const float* __restrict__ row, int col, int width, const float* __restrict__ zl) {
  RowVec<W> r;
  // W = 4, 2: the load is UNCONDITIONAL and its result is used as it is - lanes past the end of the row read the zero line zl.
  // (A load inside a divergent branch makes the compiler's wait-count pass wait for every load in flight at the join,
  // and so does a select on the loaded value scheduled right behind the load: either way the gathers of the key ring
  // were serialised, one full memory latency per key.)
  if (W == 4) {
    const float4 v = *reinterpret_cast<const float4*>(col < width ? row + col : zl);
    r.a[0] = v.x; r.a[1] = v.y; r.a[2] = v.z; r.a[W - 1] = v.w;
  } else if (W == 2) {  // rows are 16-byte aligned and widths multiples of 4: an 8-byte access never straddles the row end
    const float2 v = *reinterpret_cast<const float2*>(col < width ? row + col : zl);
    r.a[0] = v.x; r.a[W - 1] = v.y;
  } else if (W == 3) {
    if (col + 3 <= width) {
      const F3 v = *reinterpret_cast<const F3*>(row + col);
      r.a[0] = v.x; r.a[1] = v.y; r.a[W - 1] = v.z;
    } else {  // the lane that straddles the row end (one per wave) and the idle lanes
#pragma unroll
      for (int j = 0; j < W; ++j) r.a[j] = col + j < width ? row[col + j] : 0.f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < W; ++j) r.a[j] = col + j < width ? row[col + j] : 0.f;
  }
  return r;
}
template <int W>
__device__ __forceinline__ void row_store(float* __restrict__ row, int col, int width, const RowVec<W>& r) {
  if (W == 4) {
    // streaming (non-temporal) stores: the S rows - 12.7 MB per C2 batch, the step's largest output - are read once, by the
    // next launch, from other XCDs: kept out of this XCD's L2 they do not wait for its write-back at the end of the kernel
    // (C2, same box: core 17.86 -> 16.82 us, fc1 behind it 22.45 -> 23.02 us, step 85.40 -> 84.64 us)
    typedef float v4f __attribute__((ext_vector_type(4)));
    const v4f x = {r.a[0], r.a[1], r.a[2], r.a[W - 1]};
    if (col < width) __builtin_nontemporal_store(x, reinterpret_cast<v4f*>(row + col));
  } else if (W == 2) {
    if (col < width) *reinterpret_cast<float2*>(row + col) = make_float2(r.a[0], r.a[W - 1]);
  } else if (W == 3 && col + 3 <= width) {
    F3 v;
    v.x = r.a[0]; v.y = r.a[1]; v.z = r.a[W - 1];
    *reinterpret_cast<F3*>(row + col) = v;
  } else {
#pragma unroll
    for (int j = 0; j < W; ++j)
      if (col + j < width) row[col + j] = r.a[j];
  }
}

// broadcast of lane k's pointer / float to the whole wavefront through SGPRs (k is wave-uniform): v_readlane instead of a
// ds_bpermute round trip, and the row address becomes scalar base + per-lane column offset (no 64-bit vector arithmetic)
__device__ __forceinline__ const float* bcast_ptr(const float* p, int k) {
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, k);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), k);
  return reinterpret_cast<const float*>(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ float bcast_f(float x, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), k)); }
// W consecutive floats at p, no bounds: the caller clamps the column offset of lanes past the end of the row
template <int W>
__device__ __forceinline__ RowVec<W> row_load_raw(const float* __restrict__ p) {
  RowVec<W> r;
  if (W == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    r.a[0] = v.x; r.a[1] = v.y; r.a[2] = v.z; r.a[W - 1] = v.w;
  } else {
    const float2 v = *reinterpret_cast<const float2*>(p);
    r.a[0] = v.x; r.a[W - 1] = v.y;
  }
  return r;
}

// The kernel is bound by instruction issue, not by its gathers (ablated in the one-launch form, profiles/
// r03_attn_tile_phase_trace.txt: without the gathers its time does not change), so the per-key path is kept short:
//  * lane k resolves key k's three row addresses ONCE; per key they are broadcast through SGPRs (bcast_ptr) and every lane
//    adds its constant column offset - lanes past the end of a row read its first columns, which meet g = 0;
//  * node features are added as fma(fmask, yn, ya) with fmask = 0 when there is no table (yn then re-reads the node row),
//    edge features are emask * yb likewise;
//  * the range test of the time encoding (|x| <= 3e6: hardware cosine) is made once per key on a wave-uniform bound
//    instead of per element;
//  * the softmax exponentials are v_exp_f32 (arguments <= 0; ~2 ulp).
//  * FT = false: the model has neither a node-feature nor an edge-feature table (C4, C5): one gather per key instead of
//    three, and twice as many keys in flight.
// FS: feature streams gathered per key beside the node row - 2: node features + edge features, 1: edge features only
// (no node table, or the node part of a key comes from tg_model.c_table, which has the features folded in), 0: none
// diagnostic only (a build with -DTG_CORE_TRACE and TG_CORE_DBG=1, tools/trace_core.py - the stamps cost 29 registers, i.e. the
// third wavefront per SIMD, so they are compiled out of the production kernel): per-wavefront s_memtime stamps {entry, lists arrived, first key reduced,
// keys done, exit}.  C2 (one centre per wavefront, three wavefronts per SIMD): 6 450 ticks from entry to the lists' arrival,
// 5 600 to the first reduced key, 11 150 for the ten keys, 1 080 to the exit.  Hoisting the list / centre-id loads above the
// winners pass and the time-encoder rows and the G rows above the lists was tried: 178 registers (two wavefronts per SIMD),
// and held to 168 it spills and is slower (31 600 ticks against 24 300).
#ifdef TG_CORE_TRACE
__device__ unsigned long long g_core_trace[4096 * 5];
#define TG_CT(...) __VA_ARGS__
#else
#define TG_CT(...)
#endif
template <int NH, int NV, int W, int FS>
__global__ void __launch_bounds__(256) k_attn_core(tg_model m, int64_t Q, const float* __restrict__ ts,
                                                   const int64_t* __restrict__ l1_nids,
                                                   const int64_t* __restrict__ l1_eids, const float* __restrict__ l1_ts,
                                                   const float* __restrict__ reprs, const uint64_t* __restrict__ bm,
                                                   const uint32_t* __restrict__ rank, const float* __restrict__ G,
                                                   float* __restrict__ S, uint8_t* __restrict__ valid, DropCfg dc,
                                                   float* __restrict__ rsum, int direct, PosArgs pos,
                                                   const float* __restrict__ key_rows, const float* __restrict__ zl,
                                                   const float* __restrict__ gtab, const int64_t* __restrict__ cnids,
                                                   const float* __restrict__ ctab) {
  constexpr bool FT = FS > 0;
  using V = RowVec<W>;
  const int lane = lane_id();
  TG_CT(const bool trace = (direct & 256) != 0;)
  direct &= 1;
  TG_CT(const unsigned gw = blockIdx.x * 4 + (threadIdx.x >> 6);)
  TG_CT(unsigned long long tr0 = 0, tr1 = 0, tr2 = 0, tr3 = 0;)
  TG_CT(if (trace) tr0 = __builtin_amdgcn_s_memtime();)
  // direct (eager updates): neighbour rows come from the state tables, row(v) = has_msg[v] ? pending[v] : right[v];
  // the second dedup pass of the step rides here (a few thousand threads of work)
  if (pos.best) pos_winners_pass(pos, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
  if (pos.advance_off && blockIdx.x == 0 && threadIdx.x == 0) *pos.advance_off += pos.B;  // (the sampler has read it)
  const uint64_t dkey = drop_key(dc);
  const int d = m.d, de = m.d_e, K = m.n_neighbors;
  const int kvw = 2 * d + de;
  V w4[NV], p4[NV];
  int coff[NV], eoff[NV];  // column offsets of this lane in a node-width / edge-width row (0 past the end)
  float wmax = 0.f, pmax = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int c = (lane + v * TG_WAVE) * W;
    coff[v] = c < d ? c : 0;
    eoff[v] = c < de ? c : 0;
    w4[v] = row_load<W>(m.te_freq, c, d, zl);
    p4[v] = row_load<W>(m.te_phase, c, d, zl);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      wmax = fmaxf(wmax, fabsf(w4[v].a[j]));
      pmax = fmaxf(pmax, fabsf(p4[v].a[j]));
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    wmax = fmaxf(wmax, __shfl_xor(wmax, o, TG_WAVE));
    pmax = fmaxf(pmax, __shfl_xor(pmax, o, TG_WAVE));
  }
  const bool feat = FS == 2 && m.nfeats && !key_rows && !ctab;
  const float fmask = feat ? 1.f : 0.f;
  const float emask = m.efeats ? 1.f : 0.f;  // no edge table: the edge segment of a key row is zeros (feature_getter.py:95-99)
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < Q; i += (int64_t)gridDim.x * 4) {
    // ---- per-key metadata and row addresses, one key per lane
    int64_t nb_l = 0, eid_l = 0;
    float dt_l = 0.f;
    int u_l = 0;
    if (lane < K) {
      nb_l = l1_nids[i * K + lane];
      eid_l = l1_eids[i * K + lane];
      dt_l = ts[i] - l1_ts[i * K + lane];
      if (nb_l != 0) {
        if (ctab) {  // the node row comes from the per-node table: the has-message bit only feeds the invariant check
          if (pos.chk_err && bm_test(m.has_msg, nb_l)) check_msg_times(m, nb_l, pos.chk_err);
        } else if (direct) {
          const int64_t r = state_row(m, nb_l);
          u_l = (int)(2 * r + (bm_test(m.has_msg, r) ? 1 : 0));
          if (pos.chk_err && (u_l & 1)) check_msg_times(m, r, pos.chk_err);
        } else {
          u_l = (int)bm_rank(bm, rank, nb_l);
        }
      }
    }
    // key_rows (second attention layer of --n_layers 2): the node part of key k of centre i is row i*K + k of a dense
    // tensor - the neighbour's own embedding (temporal_agg_modules.py:57-66) - instead of its memory row + features.
    // A padding key (id 0) addresses row 0 of every table, which exists; its rows are fetched and never used.
    const int kk = lane < K ? lane : 0;
    const float* pn_l = key_rows ? key_rows + (i * K + kk) * d
                        : ctab   ? ctab + nb_l * d
                                 : (direct ? ((u_l & 1) ? m.pending_vals : m.right_vals) + (int64_t)(u_l >> 1) * d
                                           : reprs + (int64_t)u_l * d);
    const float* pf_l = feat ? m.nfeats + nb_l * d : pn_l;
    const float* pe_l = m.efeats ? m.efeats + eid_l * de : pn_l;
    unsigned long long live = __ballot(nb_l != 0);  // padding keys are masked (temporal_agg_modules.py:80)
    const bool any = live != 0ull;
    TG_CT(if (trace && tr1 == 0) { __builtin_amdgcn_sched_barrier(0); tr1 = __builtin_amdgcn_s_memtime() + (live & 0ull); })
    V g[NH][3][NV], acc[NH][3][NV];
    float mx[NH], l[NH], lk[NH];  // lk: sum of the kept exponentials (dropout), same rescaling as l
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      mx[h] = -INFINITY;
      l[h] = 0.f;
      lk[h] = 0.f;
      // eager query rows (tg_model.g_table): the centre NODE's row of the table instead of row i of this batch's product
      const float* gh = gtab ? gtab + (state_row(m, cnids[i]) * NH + h) * (int64_t)kvw : G + ((int64_t)i * NH + h) * kvw;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int c = (lane + v * TG_WAVE) * W;
        g[h][0][v] = row_load<W>(gh, c, d, zl);  // zeros past the end of a segment: those lanes add nothing to a score
        g[h][1][v] = row_load<W>(gh + d, c, de, zl);
        g[h][2][v] = row_load<W>(gh + d + de, c, d, zl);
#pragma unroll
        for (int j = 0; j < W; ++j) acc[h][0][v].a[j] = acc[h][1][v].a[j] = acc[h][2][v].a[j] = 0.f;
      }
    }
    // Raw rows of the next keys travel in a ring of PD register slots while the current key is reduced.  Keys are
    // reduced in list order whatever PD is, so the result does not depend on it.
    // (measured: narrow rows, W = 2, gain from a fourth slot - C4 core 84 -> 78 us - and nothing from a fifth or sixth,
    // eight are slower; W = 4 is the same with three and four)
    constexpr int PD = FS == 2 ? (NV == 1 ? (W == 2 ? 4 : 3) : 2) : FS == 1 ? (NV == 1 ? 4 : 2) : (NV == 1 ? 6 : 3);
    constexpr int PF = FT ? PD : 1;       // slots of the edge-feature rows (none without tables)
    constexpr int PN = FS == 2 ? PD : 1;  // ... of the node-feature rows
    V ya[PD][NV], yn[PN][NV], yb[PF][NV];
    auto fetch = [&](int slot, int k) {
      const float* pn = bcast_ptr(pn_l, k);
#pragma unroll
      for (int v = 0; v < NV; ++v) ya[slot][v] = row_load_raw<W>(pn + coff[v]);
      if (FS == 2) {
        const float* pf = bcast_ptr(pf_l, k);
#pragma unroll
        for (int v = 0; v < NV; ++v) yn[slot][v] = row_load_raw<W>(pf + coff[v]);
      }
      if (FT) {
        const float* pe = bcast_ptr(pe_l, k);
#pragma unroll
        for (int v = 0; v < NV; ++v) yb[slot][v] = row_load_raw<W>(pe + eoff[v]);
      }
    };
    auto reduce = [&](int slot, int k) {
      const float dt = bcast_f(dt_l, k);
      // |dt w + phi| <= |dt| wmax + pmax: below the switch-over of time_enc_fast the hardware cosine serves every element
      const bool small = fmaf(fabsf(dt), wmax, pmax) < 2.9e6f;
      V x[3][NV];
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int c = (lane + v * TG_WAVE) * W;
#pragma unroll
        for (int j = 0; j < W; ++j) {
          x[0][v].a[j] = FS == 2 ? fmaf(fmask, yn[slot][v].a[j], ya[slot][v].a[j]) : ya[slot][v].a[j];
          x[1][v].a[j] = FT ? emask * yb[slot][v].a[j] : 0.f;
        }
        if (small) {
#pragma unroll
          for (int j = 0; j < W; ++j) x[2][v].a[j] = cos_hw(__fadd_rn(__fmul_rn(dt, w4[v].a[j]), p4[v].a[j]));
        } else {
#pragma unroll
          for (int j = 0; j < W; ++j) x[2][v].a[j] = c + j < d ? time_enc_fast(dt, w4[v].a[j], p4[v].a[j]) : 0.f;
        }
      }
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        float p = 0.f;
#pragma unroll
        for (int sgm = 0; sgm < 3; ++sgm)
#pragma unroll
          for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int j = 0; j < W; ++j) p = fmaf(g[h][sgm][v].a[j], x[sgm][v].a[j], p);
        p = wave_sum(p);  // wave-uniform
        float b = 1.f;
        if (p > mx[h]) {  // new running maximum: rescale what has been accumulated (uniform branch)
          const float a = __expf(mx[h] - p);
          l[h] *= a;
          lk[h] *= a;
#pragma unroll
          for (int sgm = 0; sgm < 3; ++sgm)
#pragma unroll
            for (int v = 0; v < NV; ++v)
#pragma unroll
              for (int j = 0; j < W; ++j) acc[h][sgm][v].a[j] *= a;
          mx[h] = p;
        } else {
          b = __expf(p - mx[h]);
        }
        l[h] += b;
        if (dc.p > 0.f) {  // attention dropout (nn.MultiheadAttention): the softmax normaliser keeps every key
          b = drop_keep(dkey, DROP_ATTN, ((uint64_t)i * NH + h) * (uint64_t)K + (uint64_t)k, dc.thresh) ? b * dc.scale : 0.f;
          lk[h] += b;
        }
#pragma unroll
        for (int sgm = 0; sgm < 3; ++sgm)
#pragma unroll
          for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int j = 0; j < W; ++j) acc[h][sgm][v].a[j] = fmaf(b, x[sgm][v].a[j], acc[h][sgm][v].a[j]);
      }
    };
    // Keys are walked in list order, padding included, PD at a time; key k travels in ring slot k % PD.  Every fetch is
    // unconditional and only the arithmetic is skipped for padding keys: a branch that holds vector-memory instructions
    // makes the compiler's wait-count pass wait for EVERYTHING in flight at the join.
#pragma unroll
    for (int sl = 0; sl < PD; ++sl) fetch(sl, min(sl, K - 1));
    for (int k0 = 0; k0 < K; k0 += PD) {
#pragma unroll
      for (int sl = 0; sl < PD; ++sl) {
        const int k = k0 + sl;
        if (k < K && ((live >> k) & 1ull)) reduce(sl, k);
        TG_CT(if (trace && k == 0 && tr2 == 0) { __builtin_amdgcn_sched_barrier(0); tr2 = __builtin_amdgcn_s_memtime() + (__float_as_uint(l[0]) & 0u); })
        fetch(sl, min(k + PD, K - 1));
      }
    }
    TG_CT(if (trace && tr3 == 0) { __builtin_amdgcn_sched_barrier(0); tr3 = __builtin_amdgcn_s_memtime() + (__float_as_uint(l[0]) & 0u); })
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const float inv = any ? 1.f / l[h] : 0.f;
      float* sh = S + ((int64_t)i * NH + h) * kvw;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int c = (lane + v * TG_WAVE) * W;
#pragma unroll
        for (int sgm = 0; sgm < 3; ++sgm)
#pragma unroll
          for (int j = 0; j < W; ++j) acc[h][sgm][v].a[j] *= inv;
        row_store<W>(sh, c, d, acc[h][0][v]);
        row_store<W>(sh + d, c, de, acc[h][1][v]);
        row_store<W>(sh + d + de, c, d, acc[h][2][v]);
      }
    }
    if (lane == 0) {
      valid[i] = any ? 1 : 0;
      if (rsum) {
#pragma unroll
        for (int h = 0; h < NH; ++h) rsum[i * NH + h] = dc.p > 0.f ? (any ? lk[h] / l[h] : 0.f) : 1.f;
      }
    }
  }
#ifdef TG_CORE_TRACE
  if (trace && lane == 0 && gw < 4096) {
    g_core_trace[gw * 5 + 0] = tr0; g_core_trace[gw * 5 + 1] = tr1; g_core_trace[gw * 5 + 2] = tr2;
    g_core_trace[gw * 5 + 3] = tr3; g_core_trace[gw * 5 + 4] = __builtin_amdgcn_s_memtime();
  }
#endif
}
#ifdef TG_CORE_TRACE
extern "C" int tg_debug_core_trace(unsigned long long* out_host, int n_waves) {
  return hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_core_trace), sizeof(unsigned long long) * 5 * n_waves) == hipSuccess ? 0 : -4;
}
#endif

int attn_dims_ok(const tg_model* m) {
  if (!m || m->d <= 0 || (m->d % 4) || m->d_e <= 0 || (m->d_e % 4) || m->n_neighbors <= 0) return 0;
  if (m->n_neighbors > TG_WAVE) return 0;  // one key per lane in k_attn_core
  if (m->n_head <= 0 || (2 * m->d) % m->n_head || ((2 * m->d / m->n_head) % 4)) return 0;
  // the k_attn_core instances (launch_attn_core): 1, 2 or 4 heads; rows of max(d, d_e) <= 256 floats in one float4 per
  // lane, up to 512 in two - the latter for 2 heads only.  Refused here, in every workspace query, before any launch.
  const int wmax = std::max(m->d, m->d_e);
  if (m->n_head != 1 && m->n_head != 2 && m->n_head != 4) return 0;
  if (wmax > 2 * 4 * TG_WAVE || (wmax > 4 * TG_WAVE && m->n_head != 2)) return 0;
  return 1;
}

bool carve_attn(const tg_model* m, int64_t Q, Carver& cv, AttnWs& w) {
  const int d = m->d, kvw = 2 * m->d + m->d_e, nh = m->n_head;
  w.cc = cv.take<float>((size_t)Q * d);
  w.qp = cv.take<float>((size_t)Q * 2 * d);
  w.g = cv.take<float>((size_t)Q * nh * kvw);
  w.s = cv.take<float>((size_t)Q * nh * kvw);
  w.o = cv.take<float>((size_t)Q * 2 * d);
  w.hh = cv.take<float>((size_t)Q * 2 * d);
  w.t = cv.take<float>((size_t)Q * d);
  w.qconst = cv.take<float>((size_t)2 * d);
  w.rsum = cv.take<float>((size_t)Q * nh);
  w.valid = cv.take<uint8_t>((size_t)Q);
  w.sk = cv.take<float>(TG_SK_WS_FLOATS);
  return cv.ok;
}

static size_t attn_ws_bytes(const tg_model* m, int64_t Q) {
  const size_t d = m->d, kvw = 2 * m->d + m->d_e, nh = m->n_head;
  return align16(Q * d * 4) * 2 + align16(Q * 2 * d * 4) * 3 + align16(Q * nh * kvw * 4) * 2 + align16(2 * d * 4) +
         align16(Q * nh * 4) + align16(Q) + align16(TG_SK_WS_FLOATS * 4);
}

// ---- inference with pre-multiplied weights (tg_attn_fuse) --------------------------------
struct FusedView {
  const float *wqk, *gconst, *w1f, *b1, *c1;
  int nk;  // n_head * kvw
};
static FusedView fused_view(const tg_model* m, const float* f) {
  FusedView v{};
  const int d = m->d;
  v.nk = m->n_head * (2 * d + (m->efeats ? m->d_e : 0));  // compact form without an edge table (tg_fuse.hip)
  v.wqk = f;
  v.gconst = v.wqk + (size_t)v.nk * d;
  v.w1f = v.gconst + v.nk;
  v.b1 = v.w1f + (size_t)d * (v.nk + d);
  v.c1 = v.b1 + d;
  return v;
}

void launch_attn_core(const tg_model* m, int64_t Q, const float* ts, const int64_t* l1_nids, const int64_t* l1_eids,
                      const float* l1_ts, const float* reprs, const uint64_t* bm, const uint32_t* rank, const AttnWs& w,
                      const DropCfg& dc, hipStream_t st, int* rc_out, int direct = 0, const PosArgs* pos = nullptr,
                      const float* key_rows = nullptr, const float* gtab = nullptr, const int64_t* cnids = nullptr,
                      const float* ctab = nullptr) {
  const int d = m->d, d_e = m->d_e, nh = m->n_head;
  *rc_out = TG_OK;
  // Columns per lane: float4 (three columns per lane fill 58 of 64 lanes at d = 172 instead of 43 but measured SLOWER,
  // 29.7 vs 24.3 us at C2: 12-byte accesses straddle 16-byte sectors; that variant is gone).
  const int wmax = std::max(d, d_e);
  int W = 4, nv = (int)cdiv(cdiv(wmax, 4), TG_WAVE);
  {
    static const int w_knob = env_int("TG_ATTN_W", 0);  // tuning knob: 4 forces float4 lanes
    // narrow rows (d <= 128, e.g. LastFM's --dim 100): two columns per lane instead of four fill 50 lanes instead of 25;
    // the kernel is bound by per-key VALU work and latency there, not by bytes (8-byte accesses stay sector aligned)
    if (wmax <= 128 && w_knob != 4) { W = 2; nv = 1; }
  }
  const unsigned cgrid = flat_grid(Q, 4);
  static const int core_dbg = env_int("TG_CORE_DBG", 0);  // diagnostic: s_memtime stamps (tools/trace_core.py)
  if (core_dbg) direct |= 256;
  const float* zl = zero_line();
  if (!zl) { *rc_out = TG_EHIP; return; }
  // feature streams per key: node + edge tables (2), the edge table alone - no node table, or the node rows come from the
  // per-node table of centre rows with the features folded in (1) - or none (0)
  const int fs = (m->nfeats && !key_rows && !ctab) ? 2 : (m->efeats ? 1 : 0);
#define TG_CORE_FS(NH_, NV_, W_, FS_)                                                                                      \
  TG_KLAUNCH((k_attn_core<NH_, NV_, W_, FS_>), dim3(cgrid), dim3(256), 0, st, *m, Q, ts, l1_nids, l1_eids, l1_ts,          \
                     reprs, bm, rank, (const float*)w.g, w.s, w.valid, dc, dc.p > 0.f ? w.rsum : (float*)nullptr, direct,  \
                     pos ? *pos : PosArgs{}, key_rows, zl, gtab, cnids, ctab)
#define TG_CORE(NH_, NV_, W_)                  \
  do {                                         \
    if (fs == 2) TG_CORE_FS(NH_, NV_, W_, 2);  \
    else if (fs == 1) TG_CORE_FS(NH_, NV_, W_, 1); \
    else TG_CORE_FS(NH_, NV_, W_, 0);          \
  } while (0)
  if (nh == 2 && nv == 1 && W == 2) TG_CORE(2, 1, 2);
  else if (nh == 1 && nv == 1 && W == 2) TG_CORE(1, 1, 2);
  else if (nh == 4 && nv == 1 && W == 2) TG_CORE(4, 1, 2);
  else if (nh == 2 && nv == 1) TG_CORE(2, 1, 4);
  else if (nh == 2 && nv == 2) TG_CORE(2, 2, 4);
  else if (nh == 1 && nv == 1) TG_CORE(1, 1, 4);
  else if (nh == 4 && nv == 1) TG_CORE(4, 1, 4);
  else *rc_out = TG_EUNSUPPORTED;
#undef TG_CORE_FS
#undef TG_CORE
}

static void launch_centres(const tg_model* m, int64_t Q, const int64_t* nids, const float* reprs, const uint64_t* bm,
                           const uint32_t* rank, const AttnWs& w, const PosArgs* pos, const DirectArgs* da, hipStream_t st,
                           bool no_copy = false) {
  const int d = m->d;
  if (da)  // rows from the state tables; checks + first dedup pass ride along (the second one rides on the core)
    // (no_copy: the centre rows are read from the per-node table, tg_model.c_table - only checks, dedup and snapshot)
    hipLaunchKernelGGL(k_attn_centres_direct, dim3(flat_grid((no_copy ? std::max<int64_t>(da->n_snap, 1) : Q) * (d / 4), 256)),
                       dim3(256), 0, st, *m, Q, nids, (const float4*)m->nfeats, no_copy ? (float4*)nullptr : (float4*)w.cc, *da,
                       pos ? *pos : PosArgs{});
  else
    hipLaunchKernelGGL(k_attn_centres, dim3(flat_grid(Q * (d / 4), 256)), dim3(256), 0, st, Q, d / 4, nids,
                       (const float4*)reprs, bm, rank, (const float4*)m->nfeats, (float4*)w.cc, 0, (const float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (float*)nullptr,
                       pos ? *pos : PosArgs{});
}

static int attn_forward_fused(const tg_model* m, int64_t Q, const int64_t* nids, const float* ts,
                              const int64_t* l1_nids, const int64_t* l1_eids, const float* l1_ts, const float* reprs,
                              const uint64_t* bm, const uint32_t* rank, float* out, const AttnWs& w, hipStream_t st,
                              tg_profiler* pf, const PosArgs* pos, const DirectArgs* da, bool centres_done,
                              const float* key_rows, bool use_gtab, const WbRider* wbr, bool* wb_rode, GemmArgs* fc2_defer) {
  // stage numbering of the profiler is kept: q -> "merged q+g", g -> skipped, v/out -> skipped, fc1 -> fused
  int stage = ST_ATTN_PREP + 1;
  const int d = m->d;
  const FusedView f = fused_view(m, m->attn_fused);
  if (!centres_done)  // else: rode on the sampler's launch (or on the previous step's last one)
    launch_centres(m, Q, nids, reprs, bm, rank, w, pos, da, st, use_gtab && m->c_table && da);
  int rc;
  GemmArgs g{};
  // G = c Wqk^T + gconst   (scaled query folded through the key projection, all heads at once) - or, with eager query
  // rows, nothing: the core reads G of a centre from the per-node table
  prof_mark(pf, stage++, st);
  if (!use_gtab) {
    g.m_cap = Q; g.n = f.nk; g.k = d; g.a0 = ASeg{w.cc, d, d, nullptr};
    g.w = f.wqk; g.ldw = d; g.bias = f.gconst; g.c = w.g; g.ldc = f.nk; g.alpha = 1.f; g.nbatch = 1;
    if ((rc = gemm_launch(g, st)) != TG_OK) return rc;
  }
  prof_mark(pf, stage++, st);
  prof_mark(pf, stage++, st);
  tg_model mc = *m;  // without an edge table the fused weights are compact: the key rows have no edge segment
  if (!m->efeats) mc.d_e = 0;
  {
    KSlot ks_(KT_CORE);
    launch_attn_core(&mc, Q, ts, l1_nids, l1_eids, l1_ts, reprs, bm, rank, w, DropCfg{}, st, &rc, da ? 1 : 0, da ? pos : nullptr,
                     key_rows, use_gtab ? m->g_table : nullptr, nids, (use_gtab && da) ? m->c_table : nullptr);
  }
  if (rc != TG_OK) return rc;
  prof_mark(pf, stage++, st);
  prof_mark(pf, stage++, st);
  // t = relu([S | c] W1f^T + b1 + valid * c1)   (value projection, out projection and fc1 merged)
  prof_mark(pf, stage++, st);
  g = GemmArgs{};
  g.m_cap = Q; g.n = d; g.k = f.nk + d;
  g.a0 = ASeg{w.s, f.nk, f.nk, nullptr};
  g.a1 = (use_gtab && m->c_table) ? ASeg{m->c_table, d, d, nids} : ASeg{w.cc, d, d, nullptr};  // centre rows: table or copy
  g.w = f.w1f; g.ldw = f.nk + d; g.bias = f.b1; g.bias2 = f.c1; g.bias2_valid = w.valid;
  g.c = w.t; g.ldc = d; g.relu = 1; g.alpha = 1.f; g.nbatch = 1;
  // C2-sized batches leave this product with fewer tiles than CUs: dealt as stream-K pieces, which fc2 sums
  // (+ b1 + valid * c1, ReLU) while it stages its A operand; otherwise the plain product writes t
  // ... or, with few enough 48 x 48 tiles, LDS-free K-split blocks that leave t itself (k_gemm_ks16): fc2 is then a plain
  // short-K product
  SkPlan sk{};
  KSlot ks_fc1(KT_FC1);
  bool wb_on_fc1 = false;  // the write-back rider on the fc1 launch: then fc2 only stores STEP 6's rows (c2)
  const bool ext = wbr && wbr->planned0;  // a caller's rider (tg_part_step): hosted like the write-back rider, no second row copy
  const bool ks16 = gemm_ks16_launch(g, st, (ext || (wbr && pos && pos->win_row)) ? wbr : nullptr, &wb_on_fc1);
  const bool pieces = !ks16 && gemm_sk_partials(g, w.sk, TG_SK_WS_FLOATS, st, &sk);
  if (!ks16 && !pieces && (rc = gemm_launch(g, st)) != TG_OK) return rc;
  prof_mark(pf, stage++, st);
  KSlot ks_fc2(KT_FC2);
  g = GemmArgs{};
  g.m_cap = Q; g.n = d; g.k = d;
  g.a0 = ASeg{w.t, d, d, nullptr};
  if (pieces) {
    g.ask_part = sk.part; g.ask_U = sk.U; g.ask_nkt = sk.nkt; g.ask_NT = sk.NT; g.ask_pieces = sk.pieces;
    g.ask_bias = f.b1; g.ask_bias2 = f.c1; g.ask_valid = w.valid; g.ask_relu = 1; g.ask_alpha = 1.f;
  }
  g.w = m->attn_fc2.w; g.ldw = d; g.bias = m->attn_fc2.b;
  g.c = out; g.ldc = d; g.alpha = 1.f; g.nbatch = 1;
  bool rode = false;
  if (ext) {
    // (no second destination; hosted by fc1 already, or by this launch, or not at all)
  } else if (wbr && pos && pos->win_row) {  // STEP 6's rows leave this product's epilogue; STEP 4-5 ride on its launch (WbRider)
    g.c2 = m->left_vals; g.c2_rows = pos->win_row; g.c2_m = 2 * wbr->a.B; g.ldc2 = d;
  } else {
    wbr = nullptr;
  }
  if (fc2_defer) {
    // four-launch form: this product is not launched here - the caller runs it as the second product of the step's last
    // launch.  The step took no snapshot for STEP 5, so the rider must have run on fc1's launch, as the caller foresaw
    // (attn_fc1_hosts_rider: the same decision code)
    if (!wb_on_fc1 || !g.c2) return TG_EINVAL;
    *fc2_defer = g;
    rode = true;
  } else if (wb_on_fc1) {  // ... or rode on fc1's already: this product only stores STEP 6's rows (c2)
    if ((rc = gemm_launch(g, st)) != TG_OK) return rc;
    rode = true;
  } else if ((rc = gemm_launch(g, st, wbr, &rode)) != TG_OK) {
    return rc;
  }
  if (wb_rode) *wb_rode = rode;
  return check_launch("tg_temporal_attn_fwd(fused)");
}

int attn_forward(const tg_model* m, int64_t Q, const int64_t* nids, const float* ts, const int64_t* l1_nids,
                 const int64_t* l1_eids, const float* l1_ts, const float* reprs, const uint64_t* bm,
                 const uint32_t* rank, float* out, const AttnWs& w, hipStream_t st, tg_profiler* pf,
                 const DropCfg* drop, const PosArgs* pos, const DirectArgs* da,
                 const float* key_rows, bool centres_done, bool use_gtab,
                 const WbRider* wbr, bool* wb_rode, GemmArgs* fc2_defer) {
  if (wb_rode) *wb_rode = false;
  const DropCfg dc = drop ? *drop : DropCfg{};
  int stage = ST_ATTN_PREP;
  prof_mark(pf, stage++, st);
  const int d = m->d, d_e = m->d_e, kvw = 2 * d + d_e, nh = m->n_head, dh = 2 * d / nh, E = 2 * d;
  if (m->attn_fused && dc.p == 0.f)  // (the pre-multiplied weights do not care where the node part of a key row comes from)
    return attn_forward_fused(m, Q, nids, ts, l1_nids, l1_eids, l1_ts, reprs, bm, rank, out, w, st, pf, pos, da, centres_done,
                              key_rows, use_gtab && m->g_table && !key_rows, wbr, wb_rode, fc2_defer);
  if (fc2_defer) return TG_EINVAL;  // (only the pre-multiplied block defers its last product)
  const int qblocks = (int)cdiv(2 * d, 4);
  if (da) {  // the constant half of the query projection from the rank-form kernel (no centre rows), then the direct centres
    hipLaunchKernelGGL(k_attn_centres, dim3(1 + qblocks), dim3(256), 0, st, (int64_t)0, d / 4, nids, (const float4*)reprs, bm,
                       rank, (const float4*)m->nfeats, (float4*)w.cc, qblocks, m->attn_wq, m->attn_b_in, m->te_freq,
                       m->te_phase, w.qconst, PosArgs{});
    if (!centres_done) launch_centres(m, Q, nids, reprs, bm, rank, w, pos, da, st);
  } else {
    hipLaunchKernelGGL(k_attn_centres, dim3(flat_grid(Q * (d / 4), 256) + qblocks), dim3(256), 0, st, Q, d / 4, nids,
                       (const float4*)reprs, bm, rank, (const float4*)m->nfeats, (float4*)w.cc, qblocks, m->attn_wq,
                       m->attn_b_in, m->te_freq, m->te_phase, w.qconst, pos ? *pos : PosArgs{});
  }
  int rc;
  GemmArgs g{};
  // q = (Wq [c | TE(0)] + bq) / sqrt(dh)          (F.multi_head_attention_forward scaling)
  prof_mark(pf, stage++, st);
  g = GemmArgs{};
  g.m_cap = Q; g.n = E; g.k = d;
  g.a0 = ASeg{w.cc, d, d, nullptr};
  g.w = m->attn_wq; g.ldw = E; g.bias = w.qconst;
  g.c = w.qp; g.ldc = E; g.alpha = 1.0f / sqrtf((float)dh); g.nbatch = 1;
  if ((rc = gemm_launch(g, st)) != TG_OK) return rc;
  // g_h = Wk_h^T q_h   (k-major weight view: B[k][n] = Wk[h*dh + k][n])
  prof_mark(pf, stage++, st);
  g = GemmArgs{};
  g.m_cap = Q; g.n = kvw; g.k = dh;
  g.a0 = ASeg{w.qp, E, dh, nullptr}; g.a0_bs = dh;
  g.w = m->attn_wk; g.ldw = kvw; g.w_kmajor = 1; g.w_bs = (int64_t)dh * kvw;
  g.c = w.g; g.ldc = (int64_t)nh * kvw; g.c_bs = kvw; g.alpha = 1.f; g.nbatch = nh;
  if ((rc = gemm_launch(g, st)) != TG_OK) return rc;
  // gather + scores + softmax + weighted raw sum
  prof_mark(pf, stage++, st);
  {
    KSlot ks_(KT_CORE);
    launch_attn_core(m, Q, ts, l1_nids, l1_eids, l1_ts, reprs, bm, rank, w, dc, st, &rc, da ? 1 : 0, da ? pos : nullptr, key_rows);
  }
  if (rc != TG_OK) return rc;
  // o_h = Wv_h s_h + bv_h
  prof_mark(pf, stage++, st);
  g = GemmArgs{};
  g.m_cap = Q; g.n = dh; g.k = kvw;
  g.a0 = ASeg{w.s, (int64_t)nh * kvw, kvw, nullptr}; g.a0_bs = kvw;
  g.w = m->attn_wv; g.ldw = kvw; g.w_bs = (int64_t)dh * kvw;
  g.bias = m->attn_b_in + 2 * E; g.bias_bs = dh;
  if (dc.p > 0.f) { g.bias_rs = w.rsum; g.ld_brs = nh; }
  g.c = w.o; g.ldc = E; g.c_bs = dh; g.alpha = 1.f; g.nbatch = nh;
  if ((rc = gemm_launch(g, st)) != TG_OK) return rc;
  // h = Wo o + bo, zeroed for centres without neighbours (temporal_agg_modules.py:224-231)
  prof_mark(pf, stage++, st);
  g = GemmArgs{};
  g.m_cap = Q; g.n = E; g.k = E;
  g.a0 = ASeg{w.o, E, E, nullptr};
  g.w = m->attn_out.w; g.ldw = E; g.bias = m->attn_out.b;
  g.c = w.hh; g.ldc = E; g.row_valid = w.valid; g.alpha = 1.f; g.nbatch = 1;
  if ((rc = gemm_launch(g, st)) != TG_OK) return rc;
  // z = fc2(relu(fc1([h | c])))   (MergeLayer, basic_modules.py:16-19)
  prof_mark(pf, stage++, st);
  g = GemmArgs{};
  g.m_cap = Q; g.n = d; g.k = E + d;
  g.a0 = ASeg{w.hh, E, E, nullptr}; g.a1 = ASeg{w.cc, d, d, nullptr};
  g.w = m->attn_fc1.w; g.ldw = E + d; g.bias = m->attn_fc1.b;
  g.c = w.t; g.ldc = d; g.relu = 1; g.alpha = 1.f; g.nbatch = 1;
  {
    KSlot ks_(KT_FC1);
    if ((rc = gemm_launch(g, st)) != TG_OK) return rc;
  }
  prof_mark(pf, stage++, st);
  KSlot ks_fc2(KT_FC2);
  g = GemmArgs{};
  g.m_cap = Q; g.n = d; g.k = d;
  g.a0 = ASeg{w.t, d, d, nullptr};
  g.w = m->attn_fc2.w; g.ldw = d; g.bias = m->attn_fc2.b;
  g.c = out; g.ldc = d; g.alpha = 1.f; g.nbatch = 1;
  bool rode = false;
  if (wbr && pos && pos->win_row && dc.p == 0.f) {  // the write-back rider (see attn_forward_fused)
    g.c2 = m->left_vals; g.c2_rows = pos->win_row; g.c2_m = 2 * wbr->a.B; g.ldc2 = d;
  } else {
    wbr = nullptr;
  }
  if ((rc = gemm_launch(g, st, wbr, &rode)) != TG_OK) return rc;
  if (wb_rode) *wb_rode = rode;
  return check_launch("tg_temporal_attn_fwd");
}

// rows of the nodes nids[0 .. n) as the attention centres read them, without node features (tg_step_io.h_new)
void centre_rows_launch(const tg_model* m, int64_t n, const int64_t* nids, const float* reprs, const uint64_t* bm,
                        const uint32_t* rank, float* out, bool direct, hipStream_t st) {
  if (direct)
    hipLaunchKernelGGL(k_attn_centres_direct, dim3(flat_grid(n * (m->d / 4), 256)), dim3(256), 0, st, *m, n, nids,
                       (const float4*)nullptr, (float4*)out, DirectArgs{}, PosArgs{});
  else
    hipLaunchKernelGGL(k_attn_centres, dim3(flat_grid(n * (m->d / 4), 256)), dim3(256), 0, st, n, m->d / 4, nids,
                       (const float4*)reprs, bm, rank, (const float4*)nullptr, (float4*)out, 0, (const float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, (float*)nullptr, PosArgs{});
}

// ---- eager query rows (tiger_hip.h: tg_model.g_table) -------------------------------------------------------------
__global__ void k_ids32(int64_t n, const int64_t* __restrict__ ids, int32_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (int32_t)ids[i];
}
// G rows of the nodes nids[0 .. min(cap, *n_dev)) into m->g_table: c = e(v) + nfeat(v) as the attention centres read it
// (into `crows`, cap x d floats), then the same product the forward pass runs, scattered to the nodes' table rows
// rows of a compact [n, d] buffer -> rows ids[i] of a table (the centre rows of a rebuild into tg_model.c_table)
__global__ void __launch_bounds__(256) k_scatter_rows(int64_t cap, const int32_t* __restrict__ n_dev, int d4,
                                                      const int64_t* __restrict__ ids, const float4* __restrict__ rows,
                                                      float4* __restrict__ table) {
  const int64_t n = n_dev ? min((int64_t)*n_dev, cap) : cap;
  const int64_t total = n * d4;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / d4;
    table[ids[i] * d4 + (t - i * d4)] = rows[t];
  }
}

// the shape of fc1 / of the query-row product as far as the launchers' form decisions read it (no data pointers needed
// beyond non-null markers)
static GemmArgs fc1_shape(const tg_model* m, int64_t Q) {
  const int d = m->d;
  const FusedView f = fused_view(m, m->attn_fused);
  GemmArgs g{};
  g.m_cap = Q; g.n = d; g.k = f.nk + d;
  g.a0 = ASeg{nullptr, f.nk, f.nk, nullptr};
  g.a1 = ASeg{m->attn_fused, d, d, nullptr};
  g.w = f.w1f; g.ldw = f.nk + d; g.bias = f.b1; g.bias2 = f.c1;
  g.ldc = d; g.relu = 1; g.alpha = 1.f; g.nbatch = 1;
  return g;
}
bool attn_fc1_hosts_rider(const tg_model* m, int64_t Q) {
  if (!m->attn_fused) return false;
  const GemmArgs g = fc1_shape(m, Q);
  WbRider probe{};
  bool rode = false;
  return gemm_ks16_launch(g, nullptr, &probe, &rode, true) && rode;
}
static GemmArgs gtab_shape(const tg_model* m, int64_t cap, int64_t rows_hint, const int32_t* n_dev, const int32_t* rows32) {
  const FusedView f = fused_view(m, m->attn_fused);
  GemmArgs g{};
  g.m_cap = cap; g.m_dev = n_dev; g.m_hint = rows_hint; g.n = f.nk; g.k = m->d;
  g.w = f.wqk; g.ldw = m->d; g.bias = f.gconst; g.c = m->g_table; g.ldc = f.nk; g.c_rows = rows32; g.alpha = 1.f; g.nbatch = 1;
  return g;
}
bool gtab_hosts_second(const tg_model* m, int64_t cap, int64_t rows_hint, const GemmArgs& second) {
  if (!m->g_table || !m->attn_fused) return false;
  GemmArgs g = gtab_shape(m, cap, rows_hint, nullptr, nullptr);
  g.a0 = ASeg{m->g_table, m->d, m->d, nullptr};
  return gemm_hosts_second(g, second);
}

int gtab_rows(const tg_model* m, int64_t cap, const int64_t* nids, const int32_t* rows32, const int32_t* n_dev, float* crows,
              hipStream_t st, bool crows_ready, const CollateRider* collate, bool* rode, int64_t rows_hint,
              const GemmArgs* second, bool* second_done) {
  if (rode) *rode = false;
  if (!m->g_table || !m->attn_fused || !m->pending_vals) return TG_EINVAL;
  if (m->row_of) return TG_EUNSUPPORTED;  // (rows32 are node ids)
  const int d = m->d;
  if (!crows_ready) {  // (the GRU updater writes these rows itself, GruArgs.out2 - into the per-node table when there is one)
    hipLaunchKernelGGL(k_attn_centres_direct, dim3(flat_grid(cap * (d / 4), 256)), dim3(256), 0, st, *m, cap, nids,
                       (const float4*)m->nfeats, (float4*)crows, DirectArgs{}, PosArgs{});
    if (m->c_table)
      hipLaunchKernelGGL(k_scatter_rows, dim3(flat_grid(cap * (d / 4), 256)), dim3(256), 0, st, cap, n_dev, d / 4, nids,
                         (const float4*)crows, (float4*)m->c_table);
  }
  GemmArgs g = gtab_shape(m, cap, rows_hint, n_dev, rows32);
  // the centre rows: this launch's compact copy, or - gathered by node id - the rows of the per-node table
  g.a0 = m->c_table ? ASeg{m->c_table, d, d, nids} : ASeg{crows, d, d, nullptr};
  return gemm_launch(g, st, nullptr, rode, collate, second, second_done);
}
}  // namespace tg
using namespace tg;

extern "C" size_t tg_temporal_attn_workspace_bytes(const tg_model* m, int64_t Q) {
  if (!attn_dims_ok(m) || Q < 0) return 0;
  return attn_ws_bytes(m, Q) + 64;
}

extern "C" int tg_temporal_attn_fwd(const tg_model* m, int64_t Q, const int64_t* nids, const float* ts,
                                    const int64_t* l1_nids, const int64_t* l1_eids, const float* l1_ts,
                                    const float* reprs, const uint64_t* bitmap, const uint32_t* rank, float* out,
                                    void* ws, size_t ws_bytes, void* stream) {
  if (!attn_dims_ok(m) || Q < 0) return TG_EINVAL;
  if (Q == 0) return TG_OK;
  if (!nids || !ts || !l1_nids || !l1_eids || !l1_ts || !reprs || !bitmap || !rank || !out) return TG_EINVAL;
  Carver cv(ws, ws_bytes);
  AttnWs w{};
  if (!carve_attn(m, Q, cv, w)) return TG_EWORKSPACE;
  return attn_forward(m, Q, nids, ts, l1_nids, l1_eids, l1_ts, reprs, bitmap, rank, out, w, as_stream(stream));
}

extern "C" int tg_temporal_attn_fwd_keys(const tg_model* m, int64_t Q, const int64_t* nids, const float* ts,
                                         const int64_t* l1_nids, const int64_t* l1_eids, const float* l1_ts,
                                         const float* reprs, const uint64_t* bitmap, const uint32_t* rank,
                                         const float* key_rows, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (!attn_dims_ok(m) || Q < 0) return TG_EINVAL;
  if (Q == 0) return TG_OK;
  if (!nids || !ts || !l1_nids || !l1_eids || !l1_ts || !reprs || !bitmap || !rank || !out || !key_rows) return TG_EINVAL;
  Carver cv(ws, ws_bytes);
  AttnWs w{};
  if (!carve_attn(m, Q, cv, w)) return TG_EWORKSPACE;
  return attn_forward(m, Q, nids, ts, l1_nids, l1_eids, l1_ts, reprs, bitmap, rank, out, w, as_stream(stream), nullptr,
                      nullptr, nullptr, nullptr, key_rows);
}

extern "C" int tg_attn_gtab_rows(const tg_model* m, int64_t n, const int64_t* nids, const int32_t* n_dev, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (!attn_dims_ok(m) || n < 0) return TG_EINVAL;
  if (n == 0) return TG_OK;
  if (!nids || !ws) return TG_EINVAL;
  Carver cv(ws, ws_bytes);
  float* crows = cv.take<float>((size_t)n * m->d);
  int32_t* rows32 = cv.take<int32_t>((size_t)n);
  if (!cv.ok) return TG_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_ids32, dim3(flat_grid(n, 256)), dim3(256), 0, st, n, nids, rows32);
  const int rc = gtab_rows(m, n, nids, rows32, n_dev, crows, st, false);
  return rc != TG_OK ? rc : check_launch("tg_attn_gtab_rows");
}
