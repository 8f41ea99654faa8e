// STEP 1-2 of TIGE.contrast_learning on device - message consumption + memory update
// (tiger/model/tiger.py:208-221,292-356) -, the dense operator exports, and the fused streaming step with its
// write-back (tiger.py:229-255).  SURVEY.md K6; a13-a14.  The temporal attention of STEP 3 is tg_attn.hip, the step
// profiler tg_profile.hip.
#include "tg_step.h"
#include "tg_sample.h"
#include "tg_profile.h"

namespace tg {

// ---- invariants of compute_messages (message_modules.py:158-159, tiger.py:325-327) ----
__global__ void k_check_messages(tg_model m, const int64_t* __restrict__ outdated, const int32_t* __restrict__ n_dev,
                                 int64_t cap, uint32_t* __restrict__ err) {
  const int64_t n = min((int64_t)*n_dev, cap);
  const float* mem_ts = (m.msg_src == TG_SRC_LEFT) ? m.left_ts : m.right_ts;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t id = outdated[i];
    const float mts = m.msg_ts[id], last = mem_ts[id];
    if (last > mts) atomicOr(err, TG_ERR_MSG_BEFORE_MEM);
    if (m.msg_src == TG_SRC_LEFT && !(mts == last)) atomicOr(err, TG_ERR_MSG_TS_MISMATCH);
  }
}

// ---- message transform + updater ------------------------------------------------------
struct ApplyWs {
  float *t0, *t1, *t2;
};

static size_t apply_ws_bytes(const tg_model* m, int64_t cap) {
  const size_t mw = 3 * (size_t)m->d + m->d_e;
  size_t b = 0;
  if (m->tsfm == TG_TSFM_MLP) b += align16(cap * (mw / 2) * 4);
  if (m->tsfm != TG_TSFM_ID) b += align16(cap * mw * 4);
  if (m->upd_fn == TG_UPD_MERGE) b += align16(cap * (size_t)m->d * 4);
  return b + 16;
}

// the updater's blend form (GruArgs.w_blend): row p's memory operand is row index[p] of t, h = attn_fc2(t) is never read
struct GruBlend {
  const float* t;
  const int64_t* index;
  const float *whh2, *bhh2;  // the fold a GRU model carries in tg_model.upd_fc2
};
int apply_messages(const tg_model* m, const int64_t* outdated, const int32_t* out_pos, const int32_t* n_dev,
                   int64_t cap, float* reprs, uint32_t* err, void* ws, size_t ws_bytes, hipStream_t st,
                   bool checked_already = false, float* gates = nullptr, int64_t rows_bound = 0, float* out2 = nullptr,
                   const float* add2 = nullptr, bool out2_by_row = false, const GruBlend* blend = nullptr) {
  const int d = m->d, mw = 3 * m->d + m->d_e;
  Carver cv(ws, ws_bytes);
  ApplyWs w{};
  if (m->tsfm == TG_TSFM_MLP) w.t0 = cv.take<float>((size_t)cap * (mw / 2));
  if (m->tsfm != TG_TSFM_ID) w.t1 = cv.take<float>((size_t)cap * mw);
  if (m->upd_fn == TG_UPD_MERGE) w.t2 = cv.take<float>((size_t)cap * d);
  if (!cv.ok) return TG_EWORKSPACE;
  if (!checked_already)
    hipLaunchKernelGGL(k_check_messages, dim3(flat_grid(cap, 256)), dim3(256), 0, st, *m, outdated, n_dev, cap, err);
  int rc;
  ASeg x{m->msg_vals, mw, mw, outdated};  // raw messages gathered from the mailbox
  if (m->tsfm == TG_TSFM_LINEAR || m->tsfm == TG_TSFM_MLP) {
    if (m->tsfm == TG_TSFM_MLP && ((mw / 2) % 4)) return TG_EUNSUPPORTED;
    GemmArgs g{};
    g.m_cap = cap; g.m_dev = n_dev; g.k = mw; g.a0 = x; g.alpha = 1.f; g.nbatch = 1;
    g.w = m->tsfm1.w; g.ldw = mw; g.bias = m->tsfm1.b;
    if (m->tsfm == TG_TSFM_MLP) {
      g.n = mw / 2; g.c = w.t0; g.ldc = mw / 2; g.relu = 1;
      if ((rc = gemm_launch(g, st)) != TG_OK) return rc;
      g = GemmArgs{};
      g.m_cap = cap; g.m_dev = n_dev; g.k = mw / 2; g.a0 = ASeg{w.t0, mw / 2, mw / 2, nullptr};
      g.w = m->tsfm2.w; g.ldw = mw / 2; g.bias = m->tsfm2.b; g.alpha = 1.f; g.nbatch = 1;
    }
    g.n = mw; g.c = w.t1; g.ldc = mw; g.relu = 0;
    if ((rc = gemm_launch(g, st)) != TG_OK) return rc;
    x = ASeg{w.t1, mw, mw, nullptr};
  }
  const float* upd_vals = (m->upd_src == TG_SRC_LEFT) ? m->left_vals : m->right_vals;
  ASeg h{upd_vals, d, d, outdated};
  if (m->upd_fn == TG_UPD_GRU) {
    GruArgs a{};
    a.cap = cap; a.n_dev = n_dev; a.d = d; a.xw = mw; a.x = x; a.h = h;
    a.w_ih = m->gru_w_ih; a.w_hh = m->gru_w_hh; a.b_ih = m->gru_b_ih; a.b_hh = m->gru_b_hh;
    a.out = reprs; a.ldo = d; a.out_rows = out_pos; a.gates = gates; a.out2 = out2; a.add2 = add2;
    a.out2_by_row = out2_by_row ? 1 : 0;
    if (!m->efeats && m->tsfm == TG_TSFM_ID) {
      // raw mailbox rows [own | other | edge | time] without an edge table: the edge segment [2d, 2d + d_e) is zeros
      // (memory.py:91 over feature_getter.py:95-99); the k-tiles that lie entirely inside it are skipped
      const int first = (2 * d + 31) / 32, last = (2 * d + m->d_e) / 32;  // tiles [first, last) are inside
      if (last > first) { a.x_skip_at = first; a.x_skip_n = last - first; }
    }
    a.rows_hint = std::min<int64_t>(cap, m->n_nodes);
    if (rows_bound > 0) a.rows_hint = std::min<int64_t>(a.rows_hint, rows_bound);  // the caller's bound on the live rows
    if (blend) {
      a.h = ASeg{blend->t, d, d, blend->index};
      a.w_hh = blend->whh2; a.b_hh = blend->bhh2;
      a.w_blend = m->attn_fc2.w; a.b_blend = m->attn_fc2.b;
    }
    return gru_launch(a, st);
  }
  if (blend) return TG_EINVAL;
  GemmArgs g{};  // MergeUpdater: fc2(relu(fc1([msg | mem])))
  g.m_cap = cap; g.m_dev = n_dev; g.n = d; g.k = mw + d; g.a0 = x; g.a1 = h;
  g.w = m->upd_fc1.w; g.ldw = mw + d; g.bias = m->upd_fc1.b; g.c = w.t2; g.ldc = d; g.relu = 1; g.alpha = 1.f; g.nbatch = 1;
  if ((rc = gemm_launch(g, st)) != TG_OK) return rc;
  g = GemmArgs{};
  g.m_cap = cap; g.m_dev = n_dev; g.n = d; g.k = d; g.a0 = ASeg{w.t2, d, d, nullptr};
  g.w = m->upd_fc2.w; g.ldw = d; g.bias = m->upd_fc2.b; g.c = reprs; g.ldc = d; g.c_rows = out_pos; g.alpha = 1.f; g.nbatch = 1;
  return gemm_launch(g, st);
}

int apply_messages_rows(const tg_model* m, const int64_t* rows, const int32_t* rows32, const int32_t* n_dev, int64_t cap,
                        uint32_t* err, void* ws, size_t ws_bytes, hipStream_t st) {
  // (checked_already: the rows have just been written by STEP 5 / 6 of this very batch - the message / memory time
  //  invariants hold by construction, as for the single-GPU step's eager updater)
  return apply_messages(m, rows, rows32, n_dev, cap, m->pending_vals, err, ws, ws_bytes, st, true);
}

// unified positive-node dedup of the fused step: float32 timestamps, winner = latest ts,
// first position among ties.  best[rank(node)] = max over positions of (ts_key << 32 | ~pos).
__global__ void k_pos_max(int64_t B, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                          const float* __restrict__ ts, const uint64_t* __restrict__ bm,
                          const uint32_t* __restrict__ rank, unsigned long long* __restrict__ best,
                          int32_t* __restrict__ winner_count) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *winner_count = 0;  // k_pos_winners (next launch) counts into it
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * B; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = i < B ? i : i - B;
    const int64_t node = i < B ? src[e] : dst[e];
    const unsigned long long key = (orderable(ts[e]) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)i);
    atomicMax(best + bm_rank(bm, rank, node), key);
  }
}

__global__ void k_pos_winners(int64_t B, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                              const float* __restrict__ ts, const uint64_t* __restrict__ bm,
                              const uint32_t* __restrict__ rank, const unsigned long long* __restrict__ best,
                              int64_t* __restrict__ upos, int64_t* __restrict__ index, int32_t* __restrict__ count) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * B; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = i < B ? i : i - B;
    const int64_t node = i < B ? src[e] : dst[e];
    const unsigned long long key = (orderable(ts[e]) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)i);
    if (best[bm_rank(bm, rank, node)] == key) {
      const int slot = atomicAdd(count, 1);
      upos[slot] = node;
      index[slot] = i;
    }
  }
}

// batch slice -> query arrays: nids3 = cat[src, dst, neg], ts3 = tile(ts, 3) (float64 for the
// sampler, float32 for the model, data_loader.py:79-81,92), eids copy.  `off` (nullable)
// is the device-resident element offset of the batch inside the stream arrays.
__global__ void k_build_queries(int64_t B, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                const int64_t* __restrict__ neg, const double* __restrict__ ts,
                                const int64_t* __restrict__ eids, const int64_t* __restrict__ off,
                                int64_t* __restrict__ nids3, double* __restrict__ ts3, float* __restrict__ ts3f,
                                int64_t* __restrict__ eids_b, uint32_t* __restrict__ tmin_key) {
  const int64_t o = off ? *off : 0;
  float tmin = INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 3 * B; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = i % B;
    const int r = (int)(i / B);
    nids3[i] = r == 0 ? src[o + e] : (r == 1 ? dst[o + e] : neg[o + e]);
    const double t = ts[o + e];
    ts3[i] = t;
    ts3f[i] = (float)t;
    if (r == 0) {
      eids_b[e] = eids[o + e];
      tmin = fminf(tmin, (float)t);
    }
  }
  if (tmin_key) {  // lazy restart only: the batch's earliest (float32) time, as sample_batch_body leaves it (tg_sample.h)
    __shared__ float s_tmin[4];
    for (int sh = 32; sh > 0; sh >>= 1) tmin = fminf(tmin, __shfl_xor(tmin, sh, TG_WAVE));
    if (lane_id() == 0) s_tmin[threadIdx.x >> 6] = tmin;
    __syncthreads();
    if (threadIdx.x == 0) {
      const float v = fminf(fminf(s_tmin[0], s_tmin[1]), fminf(s_tmin[2], s_tmin[3]));
      if (v < INFINITY) atomicMax(tmin_key, ~(uint32_t)orderable(v));
    }
  }
}

__global__ void k_advance(int64_t* off, int64_t B) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *off += B;
}

int unique_compact_launch(const uint8_t* flags, uint64_t* bm, int64_t n_nodes, uint32_t* rank, int64_t* ids,
                          int32_t* count, int64_t cap, const uint64_t* hm, uint32_t* rank2, int64_t* ids2,
                          int32_t* pos2, int32_t* count2, void* ws, size_t ws_bytes, hipStream_t st);

}  // namespace tg

using namespace tg;

extern "C" int tg_linear_fwd(int64_t n, const float* x, int32_t in_f, const tg_linear* lin, int32_t out_f, int32_t relu,
                             float* out, void* stream) {
  if (n < 0 || in_f <= 0 || (in_f % 4) || out_f <= 0 || !lin) return TG_EINVAL;
  if (n == 0) return TG_OK;
  if (!x || !lin->w || !out) return TG_EINVAL;
  GemmArgs g{};
  g.m_cap = n; g.n = out_f; g.k = in_f; g.a0 = ASeg{x, in_f, in_f, nullptr};
  g.w = lin->w; g.ldw = in_f; g.bias = lin->b; g.c = out; g.ldc = out_f; g.relu = relu; g.alpha = 1.f; g.nbatch = 1;
  return gemm_launch(g, as_stream(stream));
}

// torch.nn.Linear backward on dense rows (the operator path under autograd: MergeLayer, message functions)
extern "C" size_t tg_linear_bwd_workspace_bytes(int32_t in_f, int32_t out_f) {
  if (in_f <= 0 || out_f <= 0) return 0;
  return (size_t)16 * out_f * ((size_t)in_f + 1) * sizeof(float) + 256;  // at most 16 split partials of [out_f, in_f + 1]
}
extern "C" int tg_linear_bwd(int64_t n, const float* x, int32_t in_f, const float* w, int32_t out_f, const float* dy, float* dx,
                             float* dw, float* db, void* ws, size_t ws_bytes, void* stream) {
  if (n < 0 || in_f <= 0 || (in_f % 4) || out_f <= 0 || (out_f % 4)) return TG_EINVAL;
  if (n == 0) return TG_OK;
  if (!dy || (dx && !w) || (dw && !x) || ((dw || db) && !ws)) return TG_EINVAL;
  hipStream_t st = as_stream(stream);
  int rc;
  if (dx) {  // dx = dy W
    GemmArgs g{};
    g.m_cap = n; g.n = in_f; g.k = out_f; g.a0 = ASeg{dy, out_f, out_f, nullptr};
    g.w = w; g.ldw = in_f; g.w_kmajor = 1; g.c = dx; g.ldc = in_f; g.alpha = 1.f; g.nbatch = 1;
    if ((rc = gemm_launch(g, st)) != TG_OK) return rc;
  }
  if (dw) {  // dw = dy^T x, db = column sums of dy (same pass)
    if (ws_bytes < tg_linear_bwd_workspace_bytes(in_f, out_f)) return TG_EWORKSPACE;
    TnArgs tn{};
    tn.m_cap = n; tn.n = out_f; tn.k = in_f; tn.y = dy; tn.ldy = out_f; tn.x0 = ASeg{x, in_f, in_f, nullptr};
    tn.out = dw; tn.ldo = in_f; tn.alpha = 1.f; tn.accumulate = 0; tn.nbatch = 1;
    tn.part = reinterpret_cast<float*>(ws); tn.part_floats = ws_bytes / sizeof(float);
    tn.bias_out = db; tn.bias_accumulate = 0;
    if ((rc = gemm_tn_launch(tn, st)) != TG_OK) return rc;
  } else if (db) {
    if ((rc = colsum_launch(n, nullptr, out_f, dy, out_f, 1.f, db, 0, reinterpret_cast<float*>(ws), ws_bytes / sizeof(float), st)) != TG_OK)
      return rc;
  }
  return check_launch("tg_linear_bwd");
}

extern "C" int tg_gru_fwd(int64_t n, const float* x, int32_t xw, const float* h, int32_t d, const float* w_ih,
                          const float* w_hh, const float* b_ih, const float* b_hh, float* out, void* stream) {
  if (n < 0 || d <= 0 || (d % 4) || xw <= 0 || (xw % 4)) return TG_EINVAL;
  if (n == 0) return TG_OK;
  if (!x || !h || !w_ih || !w_hh || !b_ih || !b_hh || !out) return TG_EINVAL;
  GruArgs a{};
  a.cap = n; a.d = d; a.xw = xw; a.x = ASeg{x, xw, xw, nullptr}; a.h = ASeg{h, d, d, nullptr};
  a.w_ih = w_ih; a.w_hh = w_hh; a.b_ih = b_ih; a.b_hh = b_hh; a.out = out; a.ldo = d;
  return gru_launch(a, as_stream(stream));
}

extern "C" int tg_gru_blend_fwd(int64_t n, const float* x, int32_t xw, const float* t, const int64_t* index, int32_t d,
                                const float* w_ih, const float* whh2, const float* b_ih, const float* bhh2, const float* w2,
                                const float* b2, float* out, void* stream) {
  if (n < 0 || d <= 0 || (d % 4) || xw <= 0 || (xw % 4)) return TG_EINVAL;
  if (n == 0) return TG_OK;
  if (!x || !t || !index || !w_ih || !whh2 || !b_ih || !bhh2 || !w2 || !b2 || !out) return TG_EINVAL;
  GruArgs a{};
  a.cap = n; a.d = d; a.xw = xw; a.x = ASeg{x, xw, xw, nullptr}; a.h = ASeg{t, d, d, index};
  a.w_ih = w_ih; a.w_hh = whh2; a.b_ih = b_ih; a.b_hh = bhh2; a.w_blend = w2; a.b_blend = b2; a.out = out; a.ldo = d;
  return gru_launch(a, as_stream(stream));
}

extern "C" size_t tg_apply_messages_workspace_bytes(const tg_model* m, int64_t cap) {
  if (!attn_dims_ok(m) || cap < 0) return 0;
  return apply_ws_bytes(m, cap);
}

extern "C" int tg_apply_messages(const tg_model* m, const int64_t* outdated, const int32_t* out_pos,
                                 const int32_t* n_outdated, int64_t cap, float* reprs, uint32_t* err, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (!attn_dims_ok(m) || cap < 0) return TG_EINVAL;
  if (cap == 0) return TG_OK;
  if (!outdated || !out_pos || !n_outdated || !reprs || !err) return TG_EINVAL;
  return apply_messages(m, outdated, out_pos, n_outdated, cap, reprs, err, ws, ws_bytes, as_stream(stream));
}

// ---------------------------------------------------------------------------------
// Fused streaming step
// ---------------------------------------------------------------------------------
namespace tg {
constexpr int64_t SIDE_MIN_B = 16384;  // batches above this: launches that host no riders (gemm_launch, step_forward)
// capacity of the involved-node lists: every slot of the computation graph, or - two layers, where that is Q (1 + K + K^2)
// slots - every node id if that is fewer
static int64_t involved_cap(const tg_model* m, int64_t B, int n_layers) {
  const int64_t Q = 3 * B, K = m->n_neighbors;
  return n_layers == 2 ? std::min<int64_t>(Q * (1 + K + K * K), std::max<int64_t>(m->n_nodes, 1)) : Q * (K + 1);
}

bool carve_step(const tg_model* m, int64_t B, Carver& cv, StepWs& w, int n_layers) {
  const int64_t Q = 3 * B, K = m->n_neighbors, cap = involved_cap(m, B, n_layers);
  const int64_t W = (m->n_nodes + 63) / 64;
  char* z0 = cv.p;
  w.flags = cv.take<uint8_t>((size_t)W * 64);
  w.best = cv.take<unsigned long long>((size_t)cap);
  w.counts = cv.take<int32_t>(8);
  w.zero_bytes = cv.ok ? (size_t)(cv.p - z0) : 0;
  w.bm = cv.take<uint64_t>((size_t)W);
  w.rank = cv.take<uint32_t>((size_t)W + 1);
  w.rank_out = cv.take<uint32_t>((size_t)W + 1);
  w.upos32 = cv.take<int32_t>((size_t)2 * B);
  w.win_row = cv.take<int32_t>((size_t)2 * B);
  w.snap = cv.take<float>((size_t)2 * B * m->d);
  w.snap_ts = cv.take<float>((size_t)2 * B);
  w.nids3 = cv.take<int64_t>((size_t)Q);
  w.eids = cv.take<int64_t>((size_t)B);
  w.ts3 = cv.take<double>((size_t)Q);
  w.ts3f = cv.take<float>((size_t)Q);
  w.l1_nids = cv.take<int64_t>((size_t)Q * K);
  w.l1_eids = cv.take<int64_t>((size_t)Q * K);
  w.l1_ts = cv.take<float>((size_t)Q * K);
  w.involved = cv.take<int64_t>((size_t)cap);
  w.outdated = cv.take<int64_t>((size_t)cap);
  w.out_pos = cv.take<int32_t>((size_t)cap);
  w.upos = cv.take<int64_t>((size_t)2 * B);
  w.index = cv.take<int64_t>((size_t)2 * B);
  w.reprs = cv.take<float>((size_t)cap * m->d);
  w.scan_bytes = tg_unique_compact_workspace_bytes(m->n_nodes);
  w.scan_ws = cv.take<char>(w.scan_bytes);
  if (!carve_attn(m, Q, cv, w.attn)) return false;
  w.apply_bytes = apply_ws_bytes(m, cap);
  w.apply_ws = cv.take<char>(w.apply_bytes);
  w.best_id = cv.take<unsigned long long>((size_t)m->n_nodes);  // lean steps: dedup slots indexed by node id (kept zero)
  w.other = cv.take<int64_t>((size_t)2 * B);
  if (n_layers == 2) {
    const size_t Q2 = (size_t)Q * K;
    w.h2n = cv.take<int64_t>(Q2 * K);
    w.h2e = cv.take<int64_t>(Q2 * K);
    w.h2t = cv.take<float>(Q2 * K);
    w.ts2 = cv.take<float>(Q2);
    w.emb2 = cv.take<float>(Q2 * m->d);
    if (!carve_attn(m, (int64_t)Q2, cv, w.attn2)) return false;
  }
  return cv.ok;
}
// the carve above on a dry run: workspace size and the must-be-zero prefix without a second copy of the layout
static bool carve_dry(const tg_model* m, int64_t B, int n_layers, size_t* bytes, size_t* zero_bytes) {
  char* const base = reinterpret_cast<char*>((uintptr_t)1 << 20);  // never dereferenced
  Carver cv(base, (size_t)1 << 60);
  StepWs w{};
  if (!carve_step(m, B, cv, w, n_layers)) return false;
  if (bytes) *bytes = (size_t)(cv.p - base);
  if (zero_bytes) *zero_bytes = w.zero_bytes;
  return true;
}
}  // namespace tg

extern "C" size_t tg_stream_step_workspace_bytes2(const tg_model* m, int64_t B, int32_t n_layers);
extern "C" size_t tg_stream_step_workspace_bytes(const tg_model* m, int64_t B) {
  return tg_stream_step_workspace_bytes2(m, B, 1);
}
extern "C" size_t tg_stream_step_workspace_bytes2(const tg_model* m, int64_t B, int32_t n_layers) {
  if (!attn_dims_ok(m) || B <= 0 || m->n_nodes <= 0 || (n_layers != 1 && n_layers != 2)) return 0;
  size_t b = 0;
  return tg::carve_dry(m, B, n_layers, &b, nullptr) ? b + 256 : 0;
}

extern "C" size_t tg_stream_step_zero_bytes2(const tg_model* m, int64_t B, int32_t n_layers) {
  if (!attn_dims_ok(m) || B <= 0 || m->n_nodes <= 0 || (n_layers != 1 && n_layers != 2)) return 0;
  size_t z = 0;
  return tg::carve_dry(m, B, n_layers, nullptr, &z) ? z : 0;
}
extern "C" size_t tg_stream_step_zero_bytes(const tg_model* m, int64_t B) { return tg_stream_step_zero_bytes2(m, B, 1); }

namespace tg {
__global__ void k_slot_times(int64_t n, int K, const float* __restrict__ ts, float* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = ts[i / K];
}

static WritebackArgs writeback_args(const tg_model* m, const tg_step_io* io, StepWs& w);

// Which form a step takes: one place, shared by step_forward and tg_stream_step_form (the host asks before / after a step
// whether the per-node tables are read and kept by it).
struct StepForm {
  bool direct, fused_wb, lean, gtab, lz_static, fc2_defer;
};
// rows bound the eager updater launch of a step runs with (step_writeback_b, apply_messages)
static int64_t eager_rows_bound(const tg_model* m, const tg_step_io* io) {
  const int64_t P = 2 * io->B;
  return std::min<int64_t>(std::min<int64_t>(P, m->n_nodes), io->rows_hint > 0 ? io->rows_hint : P);
}
// the merger's fc2 over the Q centres as the pre-multiplied attention block forms it (shape fields only)
static GemmArgs fc2_shape(const tg_model* m, int64_t Q) {
  GemmArgs g{};
  g.m_cap = Q; g.n = m->d; g.k = m->d;
  g.a0 = ASeg{m->attn_fc2.w, m->d, m->d, nullptr};
  g.w = m->attn_fc2.w; g.ldw = m->d; g.bias = m->attn_fc2.b; g.ldc = m->d; g.alpha = 1.f; g.nbatch = 1;
  return g;
}
// TG_FORM_FC2_DEFERRED (tiger_hip.h): every term is known before the step's first launch, and the launchers are asked
// with the very code that decides at launch time (attn_fc1_hosts_rider, gtab_hosts_second, gru_blend_ok)
static bool fc2_defer_form(const tg_model* m, const tg_step_io* io, const StepForm& f, bool drop, bool inner) {
  static const int knob = env_int("TG_FC2_DEFER", 1), wbr_knob = env_int("TG_WB_RIDER", 1);
  if (!knob || !wbr_knob) return false;
  if (!(f.direct && f.fused_wb && f.lean && f.gtab && m->c_table) || drop || inner || io->lazy) return false;
  if (m->upd_fn != TG_UPD_GRU || m->msg_src != TG_SRC_LEFT || m->row_of) return false;
  if (io->h_new || io->h_prev_left || io->h_prev_right || io->B > SIDE_MIN_B) return false;
  if (m->upd_src == TG_SRC_LEFT && (!m->upd_fc2.w || !m->upd_fc2.b || !gru_blend_ok(2 * io->B, eager_rows_bound(m, io), m->d))) return false;
  return attn_fc1_hosts_rider(m, 3 * io->B) && gtab_hosts_second(m, 2 * io->B, io->rows_hint, fc2_shape(m, 3 * io->B));
}
static StepForm step_form(const tg_model* m, const tg_step_io* io, bool eager, bool drop, bool inner) {
  StepForm f{};
  const tg_lazy_restart* lz = (io->lazy && !io->embed_only) ? io->lazy : nullptr;
  // eager updates, direct form (default; TG_EAGER_DIRECT=0 keeps the compact copy): centres and neighbour rows are read
  // from pending / right themselves, so there is no gather launch and no reprs buffer
  static const int direct_knob = env_int("TG_EAGER_DIRECT", 1);
  f.direct = eager && direct_knob != 0 && !io->eager_copy && !io->collate_only;
  // the one-launch write-back needs the snapshot; the restarter targets (h_prev_*) are read between STEP 4 and STEP 6,
  // so a step that outputs them keeps the two-phase write-back
  f.fused_wb = f.direct && !io->embed_only && !io->h_prev_left && !io->h_prev_right;
  // lean: nothing in such a step needs the involved / outdated sets, so they are not formed (tiger_hip.h, tg_step_io.lean)
  // (an embed-only step has no write-back to clean up after: lean, it touches none of the self-cleaning state at all)
  // With the in-step restart loop of the STATIC restarter a lean step still marks the involved flags (the loop's only
  // input) but forms no sorted set; the list form (any other restarter) keeps the full step
  f.lz_static = lz && !lz->list;
  f.lean = io->lean && f.direct && (!lz || f.lz_static) && (f.fused_wb || io->embed_only);
  // eager query rows: a full eager step of a model that carries the table (it refreshes the table at its end)
  // (with the in-step restart loop: only with the centre-row table, whose rows of the re-initialised nodes the loop's
  // kernel rewrites itself - their query rows are refreshed right behind it)
  f.gtab = eager && m->g_table && m->attn_fused && (!lz || (f.lz_static && m->c_table && f.lean)) && !inner && !io->embed_only &&
           !io->collate_only && !drop;
  f.fc2_defer = fc2_defer_form(m, io, f, drop, inner);
  return f;
}

int step_forward(const tg_model* m, const tg_tcsr* g, const tg_step_io* io, StepWs& w, float* gates, hipStream_t st,
                 tg_profiler* pf, const DropCfg* drop, bool eager) {
  w.eager = eager;
  w.wb_rode = false;
  const tg_model* inner = w.h2n ? io->inner : nullptr;  // two attention layers (the workspace was carved for them)
  const int64_t B = io->B, Q = 3 * B, K = m->n_neighbors, cap = involved_cap(m, B, inner ? 2 : 1);
  prof_mark(pf, ST_QUERIES, st);
  hipError_t e = hipSuccess;
  int rc;
  // ---- collate (data_loader.py:77-131): queries + temporal neighbours + involved flags, one launch
  prof_mark(pf, ST_SAMPLE, st);
  w.l1n = io->l1_nids ? io->l1_nids : w.l1_nids;
  w.l1e = io->l1_eids ? io->l1_eids : w.l1_eids;
  w.l1t = io->l1_ts ? io->l1_ts : w.l1_ts;
  const tg_lazy_restart* lz = (io->lazy && !io->embed_only) ? io->lazy : nullptr;
  const StepForm form = step_form(m, io, eager, drop != nullptr, inner != nullptr);
  w.direct = form.direct;
  w.fused_wb = form.fused_wb;
  w.lean = form.lean;
  const bool need_flags = !w.lean || lz != nullptr;
  const bool untouched = w.lean && io->embed_only;  // no flags, no dedup slots, no counts
  if ((!io->ws_is_clean || io->embed_only || io->collate_only) && !untouched) e = hipMemsetAsync(w.flags, 0, w.zero_bytes, st);
  if (e == hipSuccess && w.lean && !io->embed_only && !io->ws_is_clean)
    e = hipMemsetAsync(w.best_id, 0, (size_t)m->n_nodes * 8, st);
  if (e != hipSuccess) {
    set_hip_error(e, "tg_stream_step memset");
    return TG_EHIP;
  }
  // the positive-node dedup (needed by the write-back) rides on two launches of the forward pass
  PosArgs pos{B, w.nids3, w.ts3f, w.bm, w.rank, w.best, w.counts + 2, w.upos, w.index, w.upos32, nullptr, nullptr};
  if (w.lean) { pos.bm = nullptr; pos.rank = nullptr; pos.best = w.best_id; pos.chk_err = io->err; }
  if (untouched) {  // no dedup (there is no write-back), but the core still checks its neighbours and moves the offset on
    pos.best = nullptr;
    pos.advance_off = (io->offset_dev && io->advance) ? io->offset_dev : nullptr;
  }
  // write-back rider (tg_common.h: WbRider): STEP 4-5 share the launch of the attention block's last product, whose
  // epilogue stores STEP 6's rows; TG_WB_RIDER=0 keeps the write-back launch
  static const int wbr_knob = env_int("TG_WB_RIDER", 1);
  // (not with io->h_new: those rows are read from the tables after the attention block, i.e. before STEP 4 must run)
  const bool want_rider = w.fused_wb && wbr_knob != 0 && !drop && !io->h_new;
  // four launches (TG_FORM_FC2_DEFERRED; not with a caller's rider): no snapshot for STEP 5, fc2 leaves the chain
  w.fc2_defer = form.fc2_defer && !w.ext_rider;
  w.fc2 = GemmArgs{};
  if (want_rider) pos.win_row = w.win_row;
  if (want_rider && w.fc2_defer) pos.other = w.other;
  const PosArgs* pp = (io->embed_only && !untouched) ? nullptr : &pos;
  w.gtab = form.gtab;
  // collate prefetch (tg_step_io.prefetch_state): this step runs the NEXT batch's sampler + centres on its last launch;
  // `prefetched`: the previous call did that for this batch (a repeated collate would be harmless, just wasted)
  static const int pf_knob = env_int("TG_PREFETCH", 1);
  w.prefetch = pf_knob != 0 && io->prefetch_state && io->stream_len > 0 && io->offset_dev && io->advance && io->ws_is_clean &&
               w.lean && w.gtab && w.fused_wb && !lz && io->strategy == 0 && K <= 16 && !io->l1_nids && !io->l1_eids && !io->l1_ts &&
               B <= SIDE_MIN_B;  // (large batches: the last product's launch takes no riders, see gemm_launch)
  // (a batch prefetched by a step of the five-launch form serves this form too - its snapshot is simply not read; the
  // reverse does not hold, see tg_step_io.prefetch_state)
  const int pf_in = io->prefetch_state ? *io->prefetch_state : 0;
  const bool prefetched = w.prefetch && pf_in == 1;
  if (io->prefetch_state) *io->prefetch_state = 0;  // set again by the end of the step, once the rider is enqueued
  if (pf_in != 0 && !prefetched) {
    // a prefetch that is not used (stale, or this step takes another form): its first dedup pass left maxima in the
    // node-indexed slot table, which only the write-back of THAT batch's lean step would have cleared
    if ((e = hipMemsetAsync(w.best_id, 0, (size_t)m->n_nodes * 8, st)) != hipSuccess) {
      set_hip_error(e, "tg_stream_step memset (discarded prefetch)");
      return TG_EHIP;
    }
  }
  DirectArgs da{w.lean ? nullptr : w.outdated, w.counts + 1, cap, io->err,
                (w.fused_wb && !w.fc2_defer) ? (float4*)w.snap : nullptr, w.snap_ts, 2 * B, w.lean ? 1 : 0,
                w.fc2_defer ? 2 * B : 0};
  // lean: the centres need nothing the sampler produces and share its launch
  // (with the per-node table of centre rows - tg_model.c_table, a step that uses the query-row table - no per-batch copy
  // of the centre rows is made: the centres pass keeps its checks, the first dedup pass and the snapshot)
  const bool ctab = w.gtab && m->c_table;
  const CentresRider rider{*m, (const float4*)m->nfeats, ctab ? (float4*)nullptr : (float4*)w.attn.cc, da, pp ? pos : PosArgs{},
                           flat_grid((ctab ? 2 * B : Q) * (m->d / 4), 256)};
  w.pos_args = pp ? pos : PosArgs{};
  w.da_args = da;
  const bool recent_nodes = io->strategy == 1, uniform = io->strategy == 2;
  if (io->strategy < 0 || io->strategy > 2 || (uniform && !io->mt_state)) return TG_EUNSUPPORTED;
  if (prefetched) {
    // sampler, centres, first dedup pass and snapshot of this batch rode on the previous step's last launch
  } else if (recent_nodes || uniform) {  // query arrays first, then the sampler of graph.py:129-143 / :101-115 and the involved flags
    // (the lazy-restart loop with `uniform`: a collate-only pass would consume draws of the graph's stream the step repeats)
    if (lz && uniform) return TG_EUNSUPPORTED;
    hipLaunchKernelGGL(k_build_queries, dim3(flat_grid(Q, 256)), dim3(256), 0, st, B, io->src, io->dst, io->neg, io->ts,
                       io->eids, (const int64_t*)io->offset_dev, w.nids3, w.ts3, w.ts3f, w.eids,
                       lz ? reinterpret_cast<uint32_t*>(w.counts + 4) : nullptr);
    // uniform: the graph's MT19937 stream is consumed per non-empty query, in query order (src, dst, neg of the batch, as
    // data_loader.py:79-81 concatenates them): one wavefront walks the queries, 64 words of the stream at a time
    if ((rc = uniform ? sample_uniform_launch(g, Q, w.nids3, w.ts3, (int32_t)K, io->mt_state, w.l1n, w.l1e, w.l1t,
                                              need_flags ? w.flags : nullptr, st)
                      : sample_nodes_launch(g, Q, w.nids3, w.ts3, (int32_t)K, w.l1n, w.l1e, w.l1t, need_flags ? w.flags : nullptr,
                                            st)) != TG_OK)
      return rc;
  } else if (KSlot ks_(KT_COLLATE); (rc = sample_batch_launch(g, B, io->src, io->dst, io->neg, io->ts, io->eids, io->offset_dev, (int32_t)K,
                                       w.nids3, w.ts3f, w.eids, w.l1n, w.l1e, w.l1t, need_flags ? w.flags : nullptr, st,
                                       lz ? reinterpret_cast<uint32_t*>(w.counts + 4) : nullptr,
                                       (w.lean && !lz) ? &rider : nullptr)) != TG_OK)  // (centres: behind the restart loop)
    return rc;
  // a caller that runs work beside the rest of the forward pass (the training step's restarter: it needs the id list only)
  if (w.collate_done && hipEventRecord(w.collate_done, st) == hipSuccess) w.collate_recorded = true;
  if (io->dbg_l1_nids || io->dbg_l1_eids || io->dbg_l1_ts) {  // the lists this step consumes, before its last launch prefetches the next
    const size_t n = (size_t)Q * K;
    if (io->dbg_l1_nids && (e = hipMemcpyAsync(io->dbg_l1_nids, w.l1n, n * 8, hipMemcpyDeviceToDevice, st)) != hipSuccess) return TG_EHIP;
    if (io->dbg_l1_eids && (e = hipMemcpyAsync(io->dbg_l1_eids, w.l1e, n * 8, hipMemcpyDeviceToDevice, st)) != hipSuccess) return TG_EHIP;
    if (io->dbg_l1_ts && (e = hipMemcpyAsync(io->dbg_l1_ts, w.l1t, n * 4, hipMemcpyDeviceToDevice, st)) != hipSuccess) return TG_EHIP;
  }
  // second hop (data_loader.py:128-131): every neighbour slot (padding included) queried at its own float32 timestamp
  // - with the graph's own strategy (uniform: the graph's stream goes on behind the first hop's draws)
  if (inner && (rc = uniform ? sample_uniform_f32_launch(g, Q * K, w.l1n, w.l1t, (int32_t)K, io->mt_state, w.h2n, w.h2e, w.h2t,
                                                         need_flags ? w.flags : nullptr, st)
                             : (recent_nodes ? sample_nodes_f32_launch : sample_edges_f32_launch)(
                                   g, Q * K, w.l1n, w.l1t, (int32_t)K, w.h2n, w.h2e, w.h2t, need_flags ? w.flags : nullptr, st)) !=
                   TG_OK)
    return rc;
  // lazy restart (train_self_supervised.py:152-163): before STEP 1, because a restarted node loses its pending message
  const bool lz_tables = lz && w.gtab;  // the loop also keeps the per-node tables current (lists what it re-initialised)
  if (lz && (rc = lazy_restart_launch(g, m, lz, w.flags, reinterpret_cast<const uint32_t*>(w.counts + 4), w.counts + 3, st,
                                      lz_tables ? w.outdated : nullptr, lz_tables ? w.out_pos : nullptr)) != TG_OK)
    return rc;
  // ... their query rows: one product over the listed nodes (usually none or a handful; everybody involved right after
  // a trigger).  Nodes that lost their message at a trigger and are not involved keep stale rows - they are not up to
  // date either, so they are re-initialised (and refreshed here) before any batch reads them
  if (lz_tables && (rc = gtab_rows(m, cap, w.outdated, w.out_pos, w.counts + 3, nullptr, st, true, nullptr, nullptr, 1024)) != TG_OK)
    return rc;
  prof_mark(pf, ST_COMPACT, st);
  w.inv = io->involved ? io->involved : w.involved;
  // involved = sorted(set(...)); outdated = involved & has-message (memory.py:108-126)
  if (!w.lean &&
      (rc = unique_compact_launch(w.flags, w.bm, m->n_nodes, w.rank, w.inv, w.counts + 0, cap,
                                  m->row_of ? nullptr : m->has_msg,  // (row-indexed bitmap: a collate-only pass has no use for it)
                                  w.rank_out, w.outdated, w.out_pos, w.counts + 1, w.scan_ws, w.scan_bytes, st)) != TG_OK)
    return rc;
  if (io->collate_only) return check_launch("tg_stream_step(collate_only)");
  prof_mark(pf, ST_GATHER, st);
  w.dedup_done = pp != nullptr && pp->best != nullptr;
  // ---- STEP 1-2: reprs = right_memory[involved] (+ invariants); outdated rows <- updater(...)
  if (KSlot ks_(KT_GATHER); !w.direct &&
      (rc = consume_gather_check_launch(m, w.inv, w.counts + 0, cap, w.reprs, w.outdated, w.counts + 1, io->err, st, pp,
                                        eager)) != TG_OK)
    return rc;
  prof_mark(pf, ST_UPDATE, st);
  if (KSlot ks_(KT_UPDATER); !eager &&  // eager: the rows were gathered from the table of precomputed updater rows just now
      (rc = apply_messages(m, w.outdated, w.out_pos, w.counts + 1, cap, w.reprs, io->err, w.apply_ws, w.apply_bytes,
                           st, true, gates, io->rows_hint)) != TG_OK)
    return rc;
  // ---- STEP 3: temporal embeddings of cat[src, dst, neg]
  const float* key_rows = nullptr;
  if (inner) {
    // the Q*K neighbour slots embedded with the second layer over their own neighbours, at the ROOT's query time
    // (temporal_agg_modules.py:57-66); padding slots (node 0) are embedded too and masked by the first layer
    const int64_t Q2 = Q * K;
    hipLaunchKernelGGL(k_slot_times, dim3(flat_grid(Q2, 256)), dim3(256), 0, st, Q2, (int)K, (const float*)w.ts3f, w.ts2);
    const DirectArgs da2{nullptr, w.counts + 1, cap, io->err, nullptr, nullptr, 0, w.lean ? 1 : 0};
    PosArgs pos2{};  // no dedup rides on the inner launches; lean: the neighbours' time invariants still do
    pos2.chk_err = w.lean ? io->err : nullptr;
    if ((rc = attn_forward(inner, Q2, w.l1n, w.ts2, w.h2n, w.h2e, w.h2t, w.reprs, w.bm, w.rank, w.emb2, w.attn2, st, nullptr,
                           drop, w.direct ? &pos2 : nullptr, w.direct ? &da2 : nullptr, nullptr, false)) != TG_OK)
      return rc;
    key_rows = w.emb2;
  }
  WbRider wbr{};
  if (want_rider) {
    wbr.m = *m;
    wbr.a = writeback_args(m, io, w);
    wbr.a.snap = w.fc2_defer ? nullptr : w.snap;  // (nullptr: STEP 5 reads the left memory itself)
    wbr.a.snap_ts = w.snap_ts;
    wbr.a.other = w.other;
  }
  if ((rc = attn_forward(m, Q, w.nids3, w.ts3f, w.l1n, w.l1e, w.l1t, w.reprs, w.bm, w.rank, io->h, w.attn, st, pf,
                         drop, pp, w.direct ? &da : nullptr, key_rows, w.lean && io->strategy == 0 && !lz, w.gtab,
                         want_rider ? &wbr : w.ext_rider, &w.wb_rode, w.fc2_defer ? &w.fc2 : nullptr)) != TG_OK)
    return rc;
  prof_mark(pf, ST_DEDUP, st);
  // h(t'+) rows of cat[src, dst]: reprs[local(node)], or the table rows themselves
  if (io->h_new) centre_rows_launch(m, 2 * B, w.nids3, w.reprs, w.bm, w.rank, io->h_new, w.direct, st);
  return check_launch("tg_stream_step(forward)");
}

// ---- dedup of positive nodes (select_latest_nids on float32 ts, tiger.py:232,419; memory.py:98),
// STEP 4-5 and the restarter targets.  STEP 4-6 (tiger.py:229-255) take two launches; STEP 5
// shares a launch with whichever of STEP 4 / STEP 6 does not write the message memory
// (see tg_memory.hip)
static WritebackArgs writeback_args(const tg_model* m, const tg_step_io* io, StepWs& w) {
  const int64_t B = io->B;
  WritebackArgs wa{};
  wa.B = B; wa.src = w.nids3; wa.dst = w.nids3 + B; wa.eids = w.eids; wa.upos = w.upos; wa.index = w.index;
  wa.ts = w.ts3f;
  wa.n_upos = w.counts + 2; wa.reprs = w.reprs; wa.bm = w.bm; wa.rank = w.rank; wa.h = io->h; wa.err = io->err;
  wa.counts_src = io->counts ? w.counts : nullptr; wa.counts_dst = io->counts;
  wa.offset_dev = (io->offset_dev && io->advance) ? io->offset_dev : nullptr;
  wa.clean_flags = (w.lean && !io->lazy) ? nullptr : w.flags; wa.flag_bytes = (int64_t)((m->n_nodes + 63) / 64) * 64;
  wa.clean_best = w.lean ? w.best_id : w.best; wa.clean_best_by_pos = w.lean ? 1 : 0;
  wa.clean_counts = w.counts;
  wa.lazy_batch = (io->lazy && io->lazy->batch_dev) ? io->lazy->batch_dev : nullptr;
  wa.new_from_pending = w.direct ? 1 : 0;  // no reprs copy was made: STEP 4 reads the owner table of updater rows
  return wa;
}

int step_writeback_a(const tg_model* m, const tg_step_io* io, StepWs& w, hipStream_t st, tg_profiler* pf) {
  const int64_t B = io->B;
  if (w.fused_wb) {  // STEP 4-6 run as ONE launch from step_writeback_b
    prof_mark(pf, ST_WRITE_RIGHT, st);
    prof_mark(pf, ST_STORE_EVENTS, st);
    return TG_OK;
  }
  const int64_t* src = w.nids3;
  const int64_t* dst = w.nids3 + B;
  if (!w.dedup_done) {
    hipLaunchKernelGGL(k_pos_max, dim3(flat_grid(2 * B, 256)), dim3(256), 0, st, B, src, dst, w.ts3f, w.bm, w.rank,
                       w.best, w.counts + 2);
    hipLaunchKernelGGL(k_pos_winners, dim3(flat_grid(2 * B, 256)), dim3(256), 0, st, B, src, dst, w.ts3f, w.bm, w.rank,
                       w.best, w.upos, w.index, w.counts + 2);
  }
  const WritebackArgs wa = writeback_args(m, io, w);
  int rc;
  prof_mark(pf, ST_WRITE_RIGHT, st);
  if ((rc = writeback_launch(m, wa, 0, st)) != TG_OK) return rc;
  prof_mark(pf, ST_STORE_EVENTS, st);
  // ---- side outputs for the restarter (tiger.py:248-251): after STEP 4, before STEP 6
  if (io->h_prev_left) {
    if ((rc = tg_gather_rows(2 * B, w.nids3, m->d, m->left_vals, io->h_prev_left, nullptr, nullptr, (void*)st)) != TG_OK)
      return rc;
  }
  if (io->h_prev_right) {
    if ((rc = tg_gather_rows(2 * B, w.nids3, m->d, m->right_vals, io->h_prev_right, nullptr, nullptr, (void*)st)) != TG_OK)
      return rc;
  }
  return TG_OK;
}

// the collate part of a batch as a launch of its own (collate prefetch when the last product's kernel hosts no rider)
__global__ void __launch_bounds__(256) k_collate(CollateRider co) { co.run(blockIdx.x); }
static void collate_blocks_standalone(CollateRider& c) {
  const int64_t Q = 3 * c.s.B;
  c.sblocks = flat_grid(Q, 16);
  c.cr.blocks = flat_grid(Q * (c.cr.m.d / 4), 256);
  c.blocks = c.sblocks + c.cr.blocks;
}

int step_writeback_b(const tg_model* m, const tg_tcsr* g, const tg_step_io* io, StepWs& w, hipStream_t st, tg_profiler* pf) {
  // unique positive nodes of the batch: slot 2 of the counts, or - one-pass write-back - its copy (see writeback_fused_body)
  const int32_t* n_upos = w.fused_wb ? w.counts + 5 : w.counts + 2;
  WritebackArgs wa = writeback_args(m, io, w);
  prof_mark(pf, ST_WRITE_LEFT, st);
  int rc;
  CollateRider co{};
  if (w.fused_wb) {
    wa.snap = w.snap;
    wa.snap_ts = w.snap_ts;
  }
  // (rider: STEP 4-6 already ran inside the launch of the attention block's last product)
  if (KSlot ks_(KT_WRITEBACK); !(w.fused_wb && w.wb_rode) && (rc = writeback_launch(m, wa, w.fused_wb ? 2 : 1, st)) != TG_OK) return rc;
  prof_mark(pf, ST_EAGER, st);
  if (w.eager && !io->embed_only) {
    // every unique positive node has just received a message (STEP 5) and its memories are final for this batch
    // (STEP 4 / STEP 6): the row a later batch would compute on the fly when the node turns up as a neighbour,
    // pending[v] = updater(upd_memory[v], tsfm(mailbox[v])), is computed here, once
    const int64_t P = 2 * io->B;
    // rows_hint (eager steps): the caller's bound on the unique positive nodes of a batch; performance only
    const int64_t bound = io->rows_hint > 0 ? std::min<int64_t>(P, io->rows_hint) : P;
    // With eager query rows the GRU epilogue also leaves the attention-centre form of its rows (h + node features) in the
    // centre-row buffer of the forward pass, which is free again
    // (centre-row buffer of these launches: the block's fc1 output buffer, free since fc2 - NOT the centre rows of the
    // forward pass, which the prefetched centres of the next batch overwrite during the query-row launch)
    const bool cr = w.gtab && m->upd_fn == TG_UPD_GRU;
    if (w.prefetch) {  // the next batch's collate part rides on the step's last launch (tg_sample.h: CollateRider)
      co.s = SampleBatchArgs{*g, io->B, io->src, io->dst, io->neg, io->ts, io->eids, (const int64_t*)io->offset_dev,
                             (int)m->n_neighbors, w.nids3, w.ts3f, w.eids, w.l1n, w.l1e, w.l1t, nullptr, nullptr};
      co.cr = CentresRider{*m, (const float4*)m->nfeats, m->c_table ? (float4*)nullptr : (float4*)w.attn.cc, w.da_args,
                           w.pos_args, 0u};
      co.stream_len = io->stream_len;
    }
    const bool ctab = cr && m->c_table;  // ... or straight into the per-node table of centre rows
    KSlot ks_upd(KT_UPDATER);
    // four-launch form, upd_src = left: the left rows of the positive nodes (STEP 6) are not stored yet - they are fc2 of
    // the rows index[p] of fc1's output, and the updater reads those through the folded weights
    const GruBlend blend{w.attn.t, w.index, m->upd_fc2.w, m->upd_fc2.b};
    const bool use_blend = w.fc2_defer && m->upd_src == TG_SRC_LEFT;
    if ((rc = apply_messages(m, w.upos, w.upos32, n_upos, P, m->pending_vals, io->err, w.apply_ws, w.apply_bytes, st,
                            true, nullptr, bound, cr ? (ctab ? m->c_table : w.attn.t) : nullptr, cr ? m->nfeats : nullptr,
                            ctab, use_blend ? &blend : nullptr)) != TG_OK)
      return rc;
  }
  prof_mark(pf, ST_GTAB, st);
  if (w.gtab) {
    // ... and the query rows of the same nodes: their effective rows have just changed (tg_model.g_table)
    bool rode = false;
    KSlot ks_q(KT_QROWS);
    bool fc2_done = false;
    if ((rc = gtab_rows(m, 2 * io->B, w.upos, w.upos32, n_upos, w.attn.t, st, m->upd_fn == TG_UPD_GRU,
                        w.prefetch ? &co : nullptr, &rode, io->rows_hint, w.fc2_defer ? &w.fc2 : nullptr, &fc2_done)) != TG_OK)
      return rc;
    if (w.fc2_defer && !fc2_done) return TG_EINVAL;  // (fc2_defer_form asked the same launcher)
    if (w.prefetch && !rode) {  // this product's kernel does not host riders: the same work as a launch of its own
      collate_blocks_standalone(co);
      hipLaunchKernelGGL(k_collate, dim3(co.blocks), dim3(256), 0, st, co);
    }
    if (w.prefetch) *io->prefetch_state = 1;
  }
  prof_mark(pf, ST_COUNT, st);
  if (pf) pf->armed = true;
  return check_launch("tg_stream_step");
}
}  // namespace tg

extern "C" int32_t tg_stream_step_form(const tg_model* m, const tg_step_io* io) { return tg_stream_step_form2(m, io, 0); }
extern "C" int32_t tg_stream_step_form2(const tg_model* m, const tg_step_io* io, int32_t dropout) {
  if (!m || !io) return 0;
  const tg::StepForm f = tg::step_form(m, io, m->pending_vals != nullptr, dropout != 0, io->inner != nullptr);
  return (f.direct ? TG_FORM_DIRECT : 0) | (f.fused_wb ? TG_FORM_FUSED_WB : 0) | (f.lean ? TG_FORM_LEAN : 0) |
         (f.gtab ? TG_FORM_TABLES : 0) | (f.fc2_defer ? TG_FORM_FC2_DEFERRED : 0);
}

namespace tg {
int stream_step_ext(const tg_model* m, const tg_tcsr* g, const tg_step_io* io, void* ws, size_t ws_bytes, hipStream_t st,
                    const WbRider* ext_rider, bool* ext_rode) {
  if (ext_rode) *ext_rode = false;
  if (!attn_dims_ok(m) || !g || !io || io->B <= 0) return TG_EINVAL;
  if (!io->src || !io->dst || !io->neg || !io->ts || !io->eids || (!io->h && !io->collate_only) || !io->err)
    return TG_EINVAL;
  if (g->num_node != m->n_nodes) return TG_EINVAL;
  // physically partitioned state (tg_model.row_of): only the forms that address state by row
  if (m->row_of && !io->collate_only && !(io->embed_only && io->lean && m->pending_vals && !io->inner)) return TG_EUNSUPPORTED;
  tg_profiler* pf = (tg_profiler*)io->profiler;
  struct KtScope {  // kernel-bound timing of the step's main launches while a profiler is attached (tg_common.h)
    explicit KtScope(tg_profiler* p) {
      if (p)
        for (int i = 0; i < KT_COUNT; ++i) p->kt.hit[i] = false;
      g_kt = p ? &p->kt : nullptr;
    }
    ~KtScope() { g_kt = nullptr; }
  } kt_scope(pf);
  Carver cv(ws, ws_bytes);
  StepWs w{};
  if (!carve_step(m, io->B, cv, w, io->inner ? 2 : 1)) return TG_EWORKSPACE;
  w.ext_rider = ext_rider;
  int rc;
  // eager updates need the full step (the updater launch at its end keeps the table current)
  // embed_only still GATHERS the precomputed rows when the table is there (the partitioned multi-GPU path keeps it
  // current through tg_apply_messages after its own write-back); only a full step runs the updater at its end
  const bool eager = m->pending_vals != nullptr;
  if ((rc = step_forward(m, g, io, w, nullptr, st, pf, nullptr, eager)) != TG_OK) return rc;
  if (ext_rode) *ext_rode = ext_rider && w.wb_rode;
  if (pf && (io->embed_only || io->collate_only)) {  // no write-back stages: close the timer's remaining intervals
    for (int i = ST_WRITE_RIGHT; i <= ST_COUNT; ++i) prof_mark(pf, i, st);
    pf->armed = true;
  }
  if (io->embed_only && w.lean) return check_launch("tg_stream_step(embed_only, lean)");  // counts are not written
  if (io->embed_only || io->collate_only) {
    if (io->counts) {
      hipError_t e = hipMemcpyAsync(io->counts, w.counts, 4 * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
      if (e != hipSuccess) {
        set_hip_error(e, "tg_stream_step counts copy");
        return TG_EHIP;
      }
    }
    if (io->offset_dev && io->advance) hipLaunchKernelGGL(k_advance, dim3(1), dim3(64), 0, st, io->offset_dev, io->B);
    return check_launch("tg_stream_step(embed_only)");
  }
  if ((rc = step_writeback_a(m, io, w, st, pf)) != TG_OK) return rc;
  return step_writeback_b(m, g, io, w, st, pf);
}
}  // namespace tg

extern "C" int tg_stream_step(const tg_model* m, const tg_tcsr* g, const tg_step_io* io, void* ws, size_t ws_bytes,
                              void* stream) {
  return tg::stream_step_ext(m, g, io, ws, ws_bytes, tg::as_stream(stream), nullptr, nullptr);
}

// ---------------------------------------------------------------------------------
// Multi-GPU write-back of a global batch (see include/tiger_hip.h)
// ---------------------------------------------------------------------------------
namespace tg {
// batch slice -> positive-node arrays + float32 times, and flag the positive nodes
__global__ void k_wb_prepare(int64_t Bg, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                             const double* __restrict__ ts, const int64_t* __restrict__ eids,
                             const int64_t* __restrict__ off, int64_t* __restrict__ pos, float* __restrict__ ts2f,
                             int64_t* __restrict__ eids_b, uint8_t* __restrict__ flags) {
  const int64_t o = off ? *off : 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * Bg; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = i < Bg ? i : i - Bg;
    const int64_t node = i < Bg ? src[o + e] : dst[o + e];
    pos[i] = node;
    ts2f[i] = (float)ts[o + e];
    flags[node] = 1;
    if (i < Bg) eids_b[e] = eids[o + e];
  }
}
}  // namespace tg

struct WbWs {
  uint8_t* flags;
  unsigned long long* best;
  int32_t* counts;
  size_t zero_bytes;
  uint64_t* bm;
  uint32_t* rank;
  int64_t *pos, *eids, *uniq, *upos, *index;
  float* ts2f;
  void* scan_ws;
  size_t scan_bytes;
};

static bool carve_wb(const tg_model* m, int64_t Bg, Carver& cv, WbWs& w) {
  const int64_t W = (m->n_nodes + 63) / 64;
  char* z0 = cv.p;
  w.flags = cv.take<uint8_t>((size_t)W * 64);
  w.best = cv.take<unsigned long long>((size_t)2 * Bg);
  w.counts = cv.take<int32_t>(4);
  w.zero_bytes = cv.ok ? (size_t)(cv.p - z0) : 0;
  w.bm = cv.take<uint64_t>((size_t)W);
  w.rank = cv.take<uint32_t>((size_t)W + 1);
  w.pos = cv.take<int64_t>((size_t)2 * Bg);
  w.eids = cv.take<int64_t>((size_t)Bg);
  w.uniq = cv.take<int64_t>((size_t)2 * Bg);
  w.upos = cv.take<int64_t>((size_t)2 * Bg);
  w.index = cv.take<int64_t>((size_t)2 * Bg);
  w.ts2f = cv.take<float>((size_t)2 * Bg);
  w.scan_bytes = tg_unique_compact_workspace_bytes(m->n_nodes);
  w.scan_ws = cv.take<char>(w.scan_bytes);
  return cv.ok;
}

extern "C" size_t tg_stream_writeback_workspace_bytes(const tg_model* m, int64_t Bg) {
  if (!attn_dims_ok(m) || Bg <= 0) return 0;
  const size_t W = (m->n_nodes + 63) / 64, n2 = 2 * (size_t)Bg;
  return align16(W * 64) + align16(n2 * 8) + 16 + align16(W * 8) + align16((W + 1) * 4) + 4 * align16(n2 * 8) +
         align16(Bg * 8) + align16(n2 * 4) + align16(tg_unique_compact_workspace_bytes(m->n_nodes)) + 256;
}

extern "C" int tg_stream_writeback(const tg_model* m, const tg_writeback_io* io, void* ws, size_t ws_bytes,
                                   void* stream) {
  if (!attn_dims_ok(m) || !io || io->Bg <= 0) return TG_EINVAL;
  if (!io->src || !io->dst || !io->ts || !io->eids || !io->rows || !io->left_row || !io->err) return TG_EINVAL;
  if (io->new_from_pending ? !m->pending_vals : !io->new_row) return TG_EINVAL;
  hipStream_t st = as_stream(stream);
  const int64_t Bg = io->Bg;
  if (m->row_of && (!io->n_upos_dev || !io->owner)) return TG_EUNSUPPORTED;  // rows: the planned, owner-filtered form only
  // planned winners (no dedup work, two launches): the caller hands over the count on the device.  A rank that owns no
  // winner of the batch passes empty lists, whose pointers may be NULL: nothing to write
  if (io->n_upos_dev && !io->upos) return TG_OK;
  if (io->upos) {
    if (!io->index || !io->n_upos_dev || !io->ts32) return TG_EINVAL;
    WritebackArgs wa{};
    wa.B = Bg; wa.src = io->src; wa.dst = io->dst; wa.eids = io->eids; wa.upos = io->upos; wa.index = io->index;
    wa.ts = io->ts32; wa.n_upos = io->n_upos_dev; wa.err = io->err;
    wa.rows = io->rows; wa.new_row = io->new_row; wa.left_row = io->left_row;
    wa.owner = io->owner; wa.my_rank = io->my_rank; wa.new_from_pending = io->new_from_pending;
    int rc;
    if ((rc = writeback_launch(m, wa, 0, st)) != TG_OK) return rc;
    if ((rc = writeback_launch(m, wa, 1, st)) != TG_OK) return rc;
    return check_launch("tg_stream_writeback(planned)");
  }
  Carver cv(ws, ws_bytes);
  WbWs w{};
  if (!carve_wb(m, Bg, cv, w)) return TG_EWORKSPACE;
  hipError_t e = hipMemsetAsync(w.flags, 0, w.zero_bytes, st);
  if (e != hipSuccess) {
    set_hip_error(e, "tg_stream_writeback memset");
    return TG_EHIP;
  }
  hipLaunchKernelGGL(k_wb_prepare, dim3(flat_grid(2 * Bg, 256)), dim3(256), 0, st, Bg, io->src, io->dst, io->ts, io->eids,
                     io->offset_dev, w.pos, w.ts2f, w.eids, w.flags);
  int rc;
  if ((rc = unique_compact_launch(w.flags, w.bm, m->n_nodes, w.rank, w.uniq, w.counts + 0, 2 * Bg, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, w.scan_ws, w.scan_bytes, st)) != TG_OK)
    return rc;
  const int64_t* src = w.pos;
  const int64_t* dst = w.pos + Bg;
  hipLaunchKernelGGL(k_pos_max, dim3(flat_grid(2 * Bg, 256)), dim3(256), 0, st, Bg, src, dst, w.ts2f, w.bm, w.rank, w.best,
                     w.counts + 2);
  hipLaunchKernelGGL(k_pos_winners, dim3(flat_grid(2 * Bg, 256)), dim3(256), 0, st, Bg, src, dst, w.ts2f, w.bm, w.rank,
                     w.best, w.upos, w.index, w.counts + 2);
  WritebackArgs wa{};
  wa.B = Bg; wa.src = src; wa.dst = dst; wa.eids = w.eids; wa.upos = w.upos; wa.index = w.index; wa.ts = w.ts2f;
  wa.n_upos = w.counts + 2; wa.err = io->err;
  wa.rows = io->rows; wa.new_row = io->new_row; wa.left_row = io->left_row; wa.plan_off = io->offset_dev;
  wa.owner = io->owner; wa.my_rank = io->my_rank; wa.new_from_pending = io->new_from_pending;
  if ((rc = writeback_launch(m, wa, 0, st)) != TG_OK) return rc;
  if ((rc = writeback_launch(m, wa, 1, st)) != TG_OK) return rc;
  // phase 1 itself reads the offset (plan_off), so it is advanced by a separate launch
  if (io->offset_dev && io->advance) hipLaunchKernelGGL(k_advance, dim3(1), dim3(64), 0, st, io->offset_dev, Bg);
  return check_launch("tg_stream_writeback");
}
