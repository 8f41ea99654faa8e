// float32 MFMA GEMM with gathered A rows: the forward products and what rides on their launches (a14).
// Reference: torch.nn.Linear as used at tiger/model/message_modules.py:29-55, basic_modules.py:16-19 and
// update_modules.py:40-47 (MergeUpdater).  The fused GRU cell lives in tg_gru.hip, the weight-gradient products and
// column sums in tg_gemm_tn.hip; tg_mfma.h holds what the three share.
//
// Tiling (CDNA4): 256-thread blocks = 4 wavefronts, each wavefront owns 32x32 output
// tiles computed with v_mfma_f32_32x32x2_f32 (lane l feeds A[l&31][l>>5], B[l>>5][l&31]).
// Operand tiles are staged global -> registers -> LDS as [row][k] with a 33-float row
// stride, which makes both the scalar ds_write of a float4 and the per-lane ds_read_b32
// of the MFMA operands bank-conflict free.  Two LDS buffers, one barrier per K step;
// the next tile's global loads are issued before the MFMAs of the current one.
// blockIdx -> tile mapping keeps all N-tiles (and batches) of one M-tile on the same
// XCD (blocks b and b+8 share an L2), so gathered A rows are fetched from HBM once.
#include <cstdlib>
#include <type_traits>

#include "tg_mfma.h"
#include "tg_sample.h"

namespace tg {

// diagnostic only (TG_GEMM_DBG=16): per-block s_memtime stamps {entry, loop start, loop end, exit}
__device__ unsigned long long g_gemm_trace[4096 * 4];
// TG_GEMM_DBG=16 stamps every product of a step into the same slots; TG_PHASE_NK=n,k keeps the stamps of the products with
// that output width and inner length only (C2: fc1 172,1204; fc2 172,172; query rows 1032,172) - tools/phase_budget.py
static bool phase_selected(const GemmArgs& g) {
  static const char* sel = getenv("TG_PHASE_NK");
  if (!sel) return true;
  int n = 0, k = 0;
  return sscanf(sel, "%d,%d", &n, &k) == 2 ? (g.n == n && g.k == k) : true;
}

// diagnostic (tg_debug_gemm): family and instance of the last product this thread launched - a string literal picked in
// the branch that picks the kernel, nothing is formatted on the launch path
static thread_local const char* t_gemm_form = nullptr;
#define TG_FORM(lit_) (t_gemm_form = (lit_))

__device__ __forceinline__ void gemm_epilogue(const GemmArgs& g, const f32x16& acc, float bias, float bias2,
                                              int64_t m0, int64_t M, int n0, int wm, int wn, int fr, int fk, int bz);

// One output tile over the k-tiles [kt_begin, kt_end).  raw == nullptr: the normal epilogue; otherwise the
// accumulators are stored unmodified as a row-major [BM][BN] piece for a later fixed-order sum (stream-K
// partials, below).  ASK: the A operand is not read from a0 / a1 but assembled from such pieces while it
// is staged: A[m, k] = act(alpha * (sum of the pieces of element (m, k) + bias[k] + valid[m] * bias2[k])).
template <int WM, int WN, int KS, int D, bool ASK = false, int AP = 3>  // AP: most pieces one element is summed from
__device__ __forceinline__ void gemm_tile(const GemmArgs& g, int64_t mt, int nt, int bz, int kt_begin, int kt_end,
                                          float* __restrict__ raw, int trace_slot) {
  const unsigned long long t_entry = (g.dbg & 16) ? __builtin_amdgcn_s_memtime() : 0ull;
  // KS = 2: a second group of four wavefronts takes the other half of every tile's k-steps into its
  // own accumulators (summed through LDS at the end).  For the under-filled launches of the C2 shapes
  // (a few hundred 64x64 tiles on 1024 SIMDs) this doubles the wavefronts in flight and halves each
  // one's serial MFMA / load chain; large launches keep KS = 1.
  constexpr int THREADS = 256 * KS;
  constexpr int BM = 32 * WM, BN = 32 * WN;
  constexpr int RP = THREADS / 8;       // tile rows staged per pass (8 threads per 32-float row)
  constexpr int NA = BM / RP;           // A float4 per thread per tile
  constexpr int NB = BN / RP;           // W float4 per thread per tile (row-major and k-major alike)
  constexpr int NOPS = NA + NB;
  constexpr int PP = 8 / KS;            // k-step pairs per wave per tile
  static_assert(BM % RP == 0 && BN % RP == 0 && NOPS <= PP / 2, "one memory op per k-step pair in each half");
  __shared__ float As[2][BM][LDK];
  __shared__ float Bs[2][BN][LDK];
  __shared__ float red[KS == 2 ? 4 : 1][KS == 2 ? 16 : 1][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = (tid >> 6) & 3, ks = tid >> 8;
  int64_t M = g.m_cap;
  if (g.m_dev) M = min(M, (int64_t)*g.m_dev);
  const int64_t m0 = mt * BM;
  if (m0 >= M) return;
  const int n0 = nt * BN;
  const float* a0p = g.a0.p + (int64_t)bz * g.a0_bs;
  const float* wp = g.w + (int64_t)bz * g.w_bs;
  const int K = g.k, N = g.n, kw0 = g.a0.w;

  const int ar = tid >> 3, ac4 = (tid & 7) * 4;  // A (and row-major W) tile coordinates
  // Branch-free staging: every load is issued unconditionally from a clamped (valid) address,
  // so the compiler can keep two tiles in flight behind counted vmcnt waits.  Rows past M and
  // weight rows past N only feed outputs that are never stored; only k >= K needs zeros.
  const float* arow0[NA];
  const float* arow1[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int64_t m = min(m0 + ar + i * RP, M - 1);
    arow0[i] = a0p + (g.a0.idx ? g.a0.idx[m] : m) * g.a0.ld;
    arow1[i] = g.a1.p ? g.a1.p + (g.a1.idx ? g.a1.idx[m] : m) * g.a1.ld - kw0 : arow0[i];
  }
  int amloc[NA];       // ASK: row inside the producer's 64-row tile, validity byte of the row
  uint8_t avalid[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int64_t m = min(m0 + ar + i * RP, M - 1);
    amloc[i] = (int)(m & 63);
    avalid[i] = (ASK && g.ask_valid) ? g.ask_valid[m] : 0;
  }
  const float* wrow[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    if (!g.w_kmajor) {
      wrow[i] = wp + (int64_t)min(n0 + ar + i * RP, N - 1) * g.ldw;
    } else {
      const int f = tid + i * THREADS;
      wrow[i] = wp + min(n0 + (f % (BN / 4)) * 4, N - 4);  // column offset; the k row is added per tile
    }
  }
  // D tiles in flight (global -> registers): with the short K of the attention shapes (6-17 tiles) the
  // kernel is a chain of dependent tile loads, so the prefetch distance sets its duration
  static_assert(D >= 2 && D % 2 == 0, "even prefetch depth");
  float4 ra[D][NA], rb[D][NB];
  float4 rx[D][ASK ? NA : 1][AP + 1];  // ASK: pieces 1 .. AP-1, bias, second bias of every staged A float4
  const int nkt = kt_end;  // tiles past the end are clamped to the last one of the range
  // ASK: the pieces of element column k of this block's row tile (producer tile T = mt * NT_p + k / 64)
  auto ask_pieces = [&](int kc, int* wsel, int* psel, bool* have) {
    // (units are dealt per XCD: row tile mt belongs to XCD mt % 8, whose workers are blockIdx = 8 j + mt % 8)
    const int U = g.ask_U;
    const int ua = (((int)mt >> 3) * g.ask_NT + (kc >> 6)) * g.ask_nkt, ub = ua + g.ask_nkt;
    int j0 = (int)((float)ua * g.ask_rcpU);  // ua / U without the integer-division sequence (ua < 2^20: exact after the fix-up)
    j0 += ((j0 + 1) * U <= ua) ? 1 : 0;
    j0 -= (j0 * U > ua) ? 1 : 0;
#pragma unroll
    for (int jj = 0; jj < AP; ++jj) {
      const int j = j0 + jj;
      have[jj] = j * U < ub;
      const int jc = have[jj] ? j : j0;
      wsel[jj] = jc * 8 + ((int)mt & 7);
      psel[jj] = jc * U < ua ? 1 : 0;  // a worker that started in the previous tile holds this one second
    }
  };
  // i-th staged float4 of tile kt (i < NA: A, else W): raw load from a clamped address; columns
  // past K are zeroed when the tile is written to LDS, so nothing waits on the load here
  auto load_one = [&](int kt, int i, float4* ra, float4* rb, float4 (*rx)[AP + 1]) {
    const int k = kt * BK + ac4;
    const int kc = k < K ? k : 0;
    if (ASK && i < NA) {
      int wsel[AP], psel[AP];
      bool have[AP];
      ask_pieces(kc, wsel, psel, have);
      const size_t off = (size_t)amloc[i] * 64 + (kc & 63);
      ra[i] = ldg4(g.ask_part + ((size_t)wsel[0] * 2 + psel[0]) * 4096 + off);
#pragma unroll
      for (int pc = 1; pc < AP; ++pc) rx[i][pc - 1] = ldg4(g.ask_part + ((size_t)wsel[pc] * 2 + psel[pc]) * 4096 + off);
      rx[i][AP - 1] = ldg4(g.ask_bias + kc);
      rx[i][AP] = ldg4((g.ask_bias2 ? g.ask_bias2 : g.ask_bias) + kc);
    } else if (i < NA) {
      ra[i] = ldg4((kc < kw0 ? arow0[i] : arow1[i]) + kc);
    } else if (!g.w_kmajor) {
      rb[i - NA] = ldg4(wrow[i - NA] + kc);
    } else {
      const int kk = kt * BK + (tid + (i - NA) * THREADS) / (BN / 4);
      rb[i - NA] = ldg4(wrow[i - NA] + (int64_t)min(kk, K - 1) * g.ldw);
    }
  };
  auto store_one = [&](int buf, int kt, int i, const float4* ra, const float4* rb, const float4 (*rx)[AP + 1]) {
    const bool kin = kt * BK + ac4 < K;
    if (ASK && i < NA) {
      int wsel[AP], psel[AP];
      bool have[AP];
      ask_pieces(kin ? kt * BK + ac4 : 0, wsel, psel, have);
      const bool b2 = g.ask_bias2 && avalid[i];
      float4 v = ra[i];
#pragma unroll
      for (int pc = 1; pc < AP; ++pc) {  // in worker (= k) order: a fixed order
        if (have[pc]) {
          v.x += rx[i][pc - 1].x; v.y += rx[i][pc - 1].y; v.z += rx[i][pc - 1].z; v.w += rx[i][pc - 1].w;
        }
      }
      auto fin = [&](float p, float b, float c) {
        float o = g.ask_alpha * (p + (b2 ? b + c : b));
        if (g.ask_relu) o = fmaxf(o, 0.f);
        return kin ? o : 0.f;
      };
      sts4(As[buf][ar + i * RP], ac4,
           make_float4(fin(v.x, rx[i][AP - 1].x, rx[i][AP].x), fin(v.y, rx[i][AP - 1].y, rx[i][AP].y),
                       fin(v.z, rx[i][AP - 1].z, rx[i][AP].z), fin(v.w, rx[i][AP - 1].w, rx[i][AP].w)));
    } else if (i < NA) {
      sts4(As[buf][ar + i * RP], ac4, kin ? ra[i] : zero4());
    } else if (!g.w_kmajor) {
      sts4(Bs[buf][ar + (i - NA) * RP], ac4, kin ? rb[i - NA] : zero4());
    } else {
      const int f = tid + (i - NA) * THREADS;
      const int kk = f / (BN / 4), nn = (f % (BN / 4)) * 4;
      const float4 v = (kt * BK + kk < K) ? rb[i - NA] : zero4();
      Bs[buf][nn][kk] = v.x;
      Bs[buf][nn + 1][kk] = v.y;
      Bs[buf][nn + 2][kk] = v.z;
      Bs[buf][nn + 3][kk] = v.w;
    }
  };
  const int wm = wave / WN, wn = wave % WN;
  const int fr = lane & 31, fk = lane >> 5;
  // the bias is requested before the main loop: in the epilogue its load latency (~1 us) would be
  // fully exposed, a third of the block's lifetime at K = 172
  const int n_out = min(n0 + wn * 32 + fr, N - 1);
  const float bias = g.bias ? g.bias[(int64_t)bz * g.bias_bs + n_out] : 0.f;
  const float bias2 = g.bias2 ? g.bias2[n_out] : 0.f;
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  // Hand-scheduled tile step (same idea as k_gru): the CU's vector-memory path and the
  // in-order wave make bursts of loads / ds_writes stall the matrix pipe, so tile t+2's
  // global loads and tile t+1's LDS writes are threaded between the MFMAs of tile t, with
  // the operand fragments read one k-step pair ahead.  One barrier per tile.
  auto tile = [&](int buf, int kt, float4* la, float4* lb, float4 (*lx)[AP + 1], const float4* sa, const float4* sb,
                  const float4 (*sx)[AP + 1]) {
    const int tl = min(kt + D, nkt - 1);
    const float* ap = &As[buf][wm * 32 + fr][fk + 4 * PP * ks];  // this wave group's share of the k-steps
    const float* bp = &Bs[buf][wn * 32 + fr][fk + 4 * PP * ks];
    float a0 = ap[0], a1 = ap[2], b0 = bp[0], b1 = bp[2];
#pragma unroll
    for (int pr = 0; pr < PP; ++pr) {
      float na0 = 0.f, na1 = 0.f, nb0 = 0.f, nb1 = 0.f;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc, 0, 0, 0);
      if (pr < PP - 1) {
        na0 = ap[4 * pr + 4]; na1 = ap[4 * pr + 6];
        nb0 = bp[4 * pr + 4]; nb1 = bp[4 * pr + 6];
      }
      __builtin_amdgcn_sched_barrier(0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc, 0, 0, 0);
      if ((pr % (PP / 2)) < NOPS) {
        if (pr < PP / 2) load_one(tl, pr % (PP / 2), la, lb, lx);
        else store_one(buf ^ 1, kt + 1, pr % (PP / 2), sa, sb, sx);
      }
      __builtin_amdgcn_sched_barrier(0);
      a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;
    }
    __syncthreads();
  };
#pragma unroll
  for (int j = 0; j < D; ++j)
#pragma unroll
    for (int i = 0; i < NOPS; ++i) load_one(min(kt_begin + j, nkt - 1), i, ra[j], rb[j], rx[j]);
#pragma unroll
  for (int i = 0; i < NOPS; ++i) store_one(0, kt_begin, i, ra[0], rb[0], rx[0]);
  __syncthreads();
  const unsigned long long t_loop0 = (g.dbg & 16) ? __builtin_amdgcn_s_memtime() : 0ull;
  // tile t multiplies LDS[t & 1]; meanwhile tile t + D is loaded into the register slot tile t just
  // left (t % D) and tile t + 1 moves from its slot to the other LDS buffer
  // The loop body is straight-line (whole groups of D tiles; the remainder follows it): with a conditional
  // tile inside the loop the compiler's wait-count bookkeeping loses track of which loads are pending at the
  // joins and waits for ALL of them (vmcnt(0)) at the top of every tile, which throws the prefetch away.
  int kt = kt_begin;
  for (; kt + D <= nkt; kt += D) {
#pragma unroll
    for (int j = 0; j < D; ++j)
      tile(j & 1, kt + j, ra[j], rb[j], rx[j], ra[(j + 1) % D], rb[(j + 1) % D], rx[(j + 1) % D]);
  }
#pragma unroll
  for (int j = 0; j < D - 1; ++j)
    if (kt + j < nkt) tile(j & 1, kt + j, ra[j], rb[j], rx[j], ra[(j + 1) % D], rb[(j + 1) % D], rx[(j + 1) % D]);
  const unsigned long long t_loop1 = (g.dbg & 16) ? __builtin_amdgcn_s_memtime() : 0ull;
  if (KS == 2) {  // fold the second k-group's partial sums into the first
    if (ks == 1) {
#pragma unroll
      for (int r = 0; r < 16; ++r) red[wave][r][lane] = acc[r];
    }
    __syncthreads();
    if (ks == 1) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] += red[wave][r][lane];
  }
  if (raw) {  // partial sums of a split tile, row-major [BM][BN]: a wave store covers two full 128-byte rows
#pragma unroll
    for (int r = 0; r < 16; ++r)
      raw[(wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk) * BN + wn * 32 + fr] = acc[r];
    return;
  }
  gemm_epilogue(g, acc, bias, bias2, m0, M, n0, wm, wn, fr, fk, bz);
  if ((g.dbg & 16) && tid == 0 && trace_slot >= 0 && trace_slot < 4096) {
    g_gemm_trace[trace_slot * 4 + 0] = t_entry;
    g_gemm_trace[trace_slot * 4 + 1] = t_loop0;
    g_gemm_trace[trace_slot * 4 + 2] = t_loop1;
    g_gemm_trace[trace_slot * 4 + 3] = __builtin_amdgcn_s_memtime();
  }
}

// the epilogue of one wave's 32x32 tile: bias / scale / activation / optional per-row operands / store
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& g, const f32x16& acc, float bias, float bias2,
                                                   int64_t m0, int64_t M, int n0, int wm, int wn, int fr, int fk, int bz) {
  const int N = g.n;
  const int n = n0 + wn * 32 + fr;
  if (n >= N) return;
  float* cp = g.c + (int64_t)bz * g.c_bs;
  const bool plain = !g.bias_rs && !g.bias2 && !g.row_valid && !g.relu_mask && !g.c_rows && !g.accumulate;
  if (plain) {
    // second destination (write-back rider: h(t-) of the winning positions -> left memory): the 16 row numbers are
    // requested together; wave tiles past the last listed row skip all of it
    const bool two = g.c2 && m0 + wm * 32 < g.c2_m;  // wave-uniform
    int c2r[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
      c2r[r] = two ? g.c2_rows[min(m, g.c2_m - 1)] : -1;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
      if (m >= M) continue;
      float v = g.alpha * (acc[r] + bias);
      if (g.relu) v = fmaxf(v, 0.f);
      cp[m * g.ldc + n] = v;
      if (two && m < g.c2_m && c2r[r] >= 0) g.c2[(int64_t)c2r[r] * g.ldc2 + n] = v;
    }
  } else {
    // Optional per-row / per-element operands (row scale of the bias, validity bytes, ReLU mask, output
    // row, old value for C +=).  Phase 1 issues EVERY load of the 16 outputs unconditionally - an absent
    // operand reads a harmless valid address (the output tile) and is ignored in phase 2 - so the wave
    // waits for memory once.  With a branch per operand and output the compiler waits after each load:
    // up to 16 x 5 serialised memory latencies per wave (this was a third of the merged fc1 product).
    const float* rsp = g.bias_rs ? g.bias_rs : cp;
    const uint8_t* v2p = g.bias2 ? g.bias2_valid : reinterpret_cast<const uint8_t*>(cp);
    const uint8_t* rvp = g.row_valid ? g.row_valid : reinterpret_cast<const uint8_t*>(cp);
    const float* rmp = g.relu_mask ? g.relu_mask : cp;
    const int* crp = g.c_rows ? g.c_rows : reinterpret_cast<const int*>(cp);
    const int64_t rs_ld = g.bias_rs ? g.ld_brs : 0, rs_o = g.bias_rs ? bz : 0;
    const int64_t rm_ld = g.relu_mask ? g.ld_mask : 0, rm_o = g.relu_mask ? n : 0;
    // four outputs at a time: one exposed latency per group, 24 live registers instead of 96
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float rs[4], rm[4], old[4];
      int crow[4];
      uint8_t v2[4], rv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = q * 4 + j;
        const int64_t m = min(m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk, M - 1);
        rs[j] = rsp[m * rs_ld + rs_o];
        v2[j] = v2p[m];
        rv[j] = rvp[m];
        rm[j] = rmp[m * rm_ld + rm_o];
        crow[j] = crp[m];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = q * 4 + j;
        const int64_t m = min(m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk, M - 1);
        if (!g.c_rows) crow[j] = (int)m;
        old[j] = cp[(int64_t)crow[j] * g.ldc + n];  // read even without C +=: a valid address either way
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = q * 4 + j;
        const int64_t m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
        if (m >= M) continue;
        float be = g.bias_rs ? bias * rs[j] : bias;
        if (g.bias2 && v2[j]) be += bias2;
        float v = g.alpha * (acc[r] + be);
        if (g.relu) v = fmaxf(v, 0.f);
        if (g.row_valid && !rv[j]) v = 0.f;
        if (g.relu_mask && !(rm[j] > 0.f)) v = 0.f;
        if (g.accumulate) v += old[j];
        cp[(int64_t)crow[j] * g.ldc + n] = v;
      }
    }
  }
}

extern "C" int tg_debug_gemm_trace(unsigned long long* out_host, int n_blocks) {
  return hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_gemm_trace), sizeof(unsigned long long) * 4 * n_blocks) == hipSuccess ? 0 : -4;
}

template <int WM, int WN, int KS, int D, bool ASK = false, int AP = 3>
__device__ __forceinline__ void gemm_block(const GemmArgs& g, unsigned bid) {
  constexpr int BN = 32 * WN;
  const int NT = (g.n + BN - 1) / BN;
  const int per = NT * g.nbatch;
  const int xcd = bid & 7, s = bid >> 3;
  const int64_t mt = (int64_t)(s / per) * 8 + xcd;
  const int rem = s % per;
  gemm_tile<WM, WN, KS, D, ASK, AP>(g, mt, rem % NT, rem / NT, 0, (g.k + BK - 1) / BK, nullptr, (int)bid);
}
template <int WM, int WN, int KS, int D, bool ASK = false, int AP = 3>
__global__ void __launch_bounds__(256 * KS) k_gemm(GemmArgs g) {
  gemm_block<WM, WN, KS, D, ASK, AP>(g, blockIdx.x);
}
// ... with a rider as the first r.blocks workgroups (WbRider: tg_common.h; CollateRider: tg_sample.h)
template <class R, int WM, int WN, int KS, int D, bool ASK = false, int AP = 3>
__global__ void __launch_bounds__(256 * KS) k_gemm_r(GemmArgs g, R r) {
  const unsigned own = gridDim.x - r.blocks;  // the product's blocks: before the riders (r.last) or after them
  if (r.last ? blockIdx.x >= own : blockIdx.x < r.blocks) {
    r.run(r.last ? blockIdx.x - own : blockIdx.x);
    return;
  }
  gemm_block<WM, WN, KS, D, ASK, AP>(g, r.last ? blockIdx.x : blockIdx.x - r.blocks);
}

// ---- register-blocked tiles for plain products ----------------------------------------------------------------------
// At C2 sizes the 64 x 64 blocks above are bound by what a CU can pull through its vector-memory path, not by the
// matrix pipe: the G product moves 306 KB per CU for 19.6 k cycles of MFMA work and takes 46 k cycles, and an LDS-free
// form with the SAME bytes per MFMA takes as long (tools/experiments/gemm_direct_no_lds.patch).  Here a wavefront owns
// RM x RN accumulator tiles of 32 x 32, the block (64 RM) x (64 RN): every staged float feeds 2 RN (A) or 2 RM (B) MFMA
// rows instead of two, i.e. 128 x 128 blocks stage half the bytes per MFMA, and a fragment read from LDS feeds RN (RM)
// MFMAs instead of one.  Same pipeline as gemm_tile (two register sets, two LDS buffers, one barrier per k-tile, the
// loads of tile t + 2 and the LDS writes of tile t + 1 threaded between the MFMAs of tile t); plain epilogue only.
template <int RM, int RN>
__device__ __forceinline__ void gemm_rb_block(const GemmArgs& g, unsigned bid) {
  constexpr int BM = 64 * RM, BN = 64 * RN;
  constexpr int RP = 32;                 // tile rows staged per pass (8 threads per 32-float row)
  constexpr int NA = BM / RP, NB = BN / RP, NOPS = NA + NB;
  static_assert(NOPS <= 8, "one memory op per k-step in each half of the tile");
  __shared__ float As[2][BM][LDK];
  __shared__ float Bs[2][BN][LDK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 31, fk = lane >> 5;
  const int K = g.k, N = g.n;
  int64_t M = g.m_cap;
  if (g.m_dev) M = min(M, (int64_t)*g.m_dev);
  const int NT = (N + BN - 1) / BN;
  const int xcd = bid & 7, s = bid >> 3;
  const int64_t mt = (int64_t)(s / NT) * 8 + xcd;
  const int nt = s % NT;
  const int64_t m0 = mt * BM;
  if (m0 >= M) return;
  const int n0 = nt * BN;
  const int ar = tid >> 3, ac4 = (tid & 7) * 4;
  const int kw0 = g.a0.w;  // A = [a0 | a1]: columns [0, kw0) from a0, the rest from a1
  const float* arow[NA];
  const float* arow1[NA];
  const float* wrow[NB];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int64_t m = min(m0 + ar + i * RP, M - 1);
    arow[i] = g.a0.p + (g.a0.idx ? g.a0.idx[m] : m) * g.a0.ld;
    arow1[i] = g.a1.p ? g.a1.p + (g.a1.idx ? g.a1.idx[m] : m) * g.a1.ld - kw0 : arow[i];
  }
#pragma unroll
  for (int i = 0; i < NB; ++i) wrow[i] = g.w + (int64_t)min(n0 + ar + i * RP, N - 1) * g.ldw;
  float bias[RN], bias2[RN];
#pragma unroll
  for (int v = 0; v < RN; ++v) {
    const int nb = min(n0 + (wn * RN + v) * 32 + fr, N - 1);
    bias[v] = g.bias ? g.bias[nb] : 0.f;
    bias2[v] = g.bias2 ? g.bias2[nb] : 0.f;
  }
  const int nkt = (K + BK - 1) / BK;
  float4 ra[2][NA], rb[2][NB];
  auto load_one = [&](int kt, int i, float4* qa, float4* qb) {
    const int k = min(kt, nkt - 1) * BK + ac4;
    const int kc = k < K ? k : 0;
    if (i < NA) qa[i] = ldg4((kc < kw0 ? arow[i] : arow1[i]) + kc);
    else qb[i - NA] = ldg4(wrow[i - NA] + kc);
  };
  auto store_one = [&](int buf, int kt, int i, const float4* qa, const float4* qb) {
    const bool kin = kt * BK + ac4 < K;
    if (i < NA) sts4(As[buf][ar + i * RP], ac4, kin ? qa[i] : zero4());
    else sts4(Bs[buf][ar + (i - NA) * RP], ac4, kin ? qb[i - NA] : zero4());
  };
  f32x16 acc[RM][RN];
#pragma unroll
  for (int u = 0; u < RM; ++u)
#pragma unroll
    for (int v = 0; v < RN; ++v)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[u][v][i] = 0.f;
  auto tile = [&](int buf, int kt, float4* la, float4* lb, const float4* sa, const float4* sb) {
    float a[RM], b[RN], na[RM], nb[RN];
#pragma unroll
    for (int u = 0; u < RM; ++u) a[u] = As[buf][(wm * RM + u) * 32 + fr][fk];
#pragma unroll
    for (int v = 0; v < RN; ++v) b[v] = Bs[buf][(wn * RN + v) * 32 + fr][fk];
#pragma unroll
    for (int st = 0; st < 16; ++st) {  // k-steps of two
      if (st < 15) {
#pragma unroll
        for (int u = 0; u < RM; ++u) na[u] = As[buf][(wm * RM + u) * 32 + fr][fk + 2 * st + 2];
#pragma unroll
        for (int v = 0; v < RN; ++v) nb[v] = Bs[buf][(wn * RN + v) * 32 + fr][fk + 2 * st + 2];
      }
#pragma unroll
      for (int u = 0; u < RM; ++u)
#pragma unroll
        for (int v = 0; v < RN; ++v) {
          acc[u][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[v], acc[u][v], 0, 0, 0);
          if (u == 0 && v == 0) {  // this k-step's memory op rides behind its first MFMA
            if (st < 8) { if (st < NOPS) load_one(kt + 2, st, la, lb); }
            else if (st - 8 < NOPS) store_one(buf ^ 1, kt + 1, st - 8, sa, sb);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
      for (int u = 0; u < RM; ++u) a[u] = na[u];
#pragma unroll
      for (int v = 0; v < RN; ++v) b[v] = nb[v];
    }
    __syncthreads();
  };
#pragma unroll
  for (int i = 0; i < NOPS; ++i) load_one(0, i, ra[0], rb[0]);
#pragma unroll
  for (int i = 0; i < NOPS; ++i) load_one(1, i, ra[1], rb[1]);
#pragma unroll
  for (int i = 0; i < NOPS; ++i) store_one(0, 0, i, ra[0], rb[0]);
  __syncthreads();
  int kt = 0;
  for (; kt + 2 <= nkt; kt += 2) {  // even tile: LDS[0], loads tile t + 2 -> set 0, stores tile t + 1 (set 1) -> LDS[1]
    tile(0, kt, ra[0], rb[0], ra[1], rb[1]);
    tile(1, kt + 1, ra[1], rb[1], ra[0], rb[0]);
  }
  if (kt < nkt) tile(0, kt, ra[0], rb[0], ra[1], rb[1]);
#pragma unroll
  for (int u = 0; u < RM; ++u)
#pragma unroll
    for (int v = 0; v < RN; ++v) {
      const int n = n0 + (wn * RN + v) * 32 + fr;
      if (n >= N) continue;
      uint8_t v2[16];  // the second bias is added on rows whose validity byte is set; all 16 bytes requested together
      int crow[16];    // ... and the output rows (c_rows: scattered)
      int c2r[16];     // ... and the rows of the second destination (c2: the write-back rider's STEP 6)
      const bool two = g.c2 && m0 + (wm * RM + u) * 32 < g.c2_m;  // wave-uniform
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t m = min(m0 + (wm * RM + u) * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk, M - 1);
        v2[r] = g.bias2 ? g.bias2_valid[m] : 0;
        crow[r] = g.c_rows ? g.c_rows[m] : (int)m;
        c2r[r] = two ? g.c2_rows[min(m, g.c2_m - 1)] : -1;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t m = m0 + (wm * RM + u) * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
        if (m >= M) continue;
        float x = g.alpha * (acc[u][v][r] + bias[v] + (v2[r] ? bias2[v] : 0.f));
        if (g.relu) x = fmaxf(x, 0.f);
        g.c[(int64_t)crow[r] * g.ldc + n] = x;
        if (two && m < g.c2_m && c2r[r] >= 0) g.c2[(int64_t)c2r[r] * g.ldc2 + n] = x;
      }
    }
}
template <int RM, int RN>
__global__ void __launch_bounds__(256) k_gemm_rb(GemmArgs g) {
  gemm_rb_block<RM, RN>(g, blockIdx.x);
}
// ---- activation-stationary blocks for short-K, wide-N products ------------------------------------------------------
// The G product of the fused attention (K = d, N = n_head (2d + d_e)) has NKT = 4 .. 8 k-tiles per output tile and many
// column tiles per row tile.  As separate 64 x 64 blocks every column tile re-stages the same 64 x K activation panel
// and pays its own prologue (first loads exposed) and epilogue; at C2 that is 816 blocks of 18 k cycles, a third of it
// outside the k-loop.  Here a block stages its activation panel ONCE (64 x K, odd row stride: conflict-free fragment
// reads) and walks `cpb` column tiles, streaming only weight tiles through the two-buffer pipeline: the stream never
// drains between column tiles (the next tile's first weight tile is already in LDS when a tile's outputs are stored),
// and per k-tile half as much is staged.  NKT is a template parameter so that the tile walk is straight-line.
template <int NKT>
__device__ __forceinline__ void gemm_astat_block(const GemmArgs& g, int cpb, unsigned bid) {
  static_assert(NKT % 2 == 0, "the LDS buffer of a weight tile follows from its k-tile index");
  constexpr int SA = NKT * BK + 1;  // panel row stride (odd)
  __shared__ float As[64][SA];
  __shared__ float Bs[2][64][LDK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 31, fk = lane >> 5;
  const int K = g.k, N = g.n;
  int64_t M = g.m_cap;
  if (g.m_dev) M = min(M, (int64_t)*g.m_dev);
  const int NT = (N + 63) / 64, NG = (NT + cpb - 1) / cpb;  // column tiles, column groups
  const int xcd = bid & 7, s = bid >> 3;
  const int64_t mt = (int64_t)(s / NG) * 8 + xcd;
  const int c0 = (s % NG) * cpb, c1 = min(c0 + cpb, NT);
  const int64_t m0 = mt * 64;
  if (m0 >= M) return;
  const int ar = tid >> 3, ac4 = (tid & 7) * 4;
  int crow[16];  // output rows of this lane's 16 accumulator rows (c_rows: scattered; requested now, used after the loop)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t m = min(m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk, M - 1);
    crow[r] = g.c_rows ? g.c_rows[m] : (int)m;
  }
  // ---- the activation panel, once
  {
    float4 pa[2][NKT];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t m = min(m0 + ar + 32 * i, M - 1);
      const float* row = g.a0.p + (g.a0.idx ? g.a0.idx[m] : m) * g.a0.ld;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        const int k = kt * BK + ac4;
        pa[i][kt] = ldg4(row + (k < K ? k : 0));
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) sts4(As[ar + 32 * i], kt * BK + ac4, kt * BK + ac4 < K ? pa[i][kt] : zero4());
  }
  // ---- weight tiles: (column tile c, k-tile j), two register sets / two LDS buffers by the parity of j
  float4 rb[2][2];
  auto load_w = [&](int c, int j, int i, float4* q) {  // i-th staged float4 (rows ar, ar + 32 of the tile)
    const int cc = min(c, c1 - 1);  // past the last column tile: a redundant reload keeps the walk branch-free
    const int k = j * BK + ac4;
    q[i] = ldg4(g.w + (int64_t)min(cc * 64 + ar + 32 * i, N - 1) * g.ldw + (k < K ? k : 0));
  };
  auto store_w = [&](int buf, int j, int i, const float4* q) {
    sts4(Bs[buf][ar + 32 * i], ac4, j * BK + ac4 < K ? q[i] : zero4());
  };
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  load_w(c0, 0, 0, rb[0]); load_w(c0, 0, 1, rb[0]);
  load_w(c0, 1, 0, rb[1]); load_w(c0, 1, 1, rb[1]);
  store_w(0, 0, 0, rb[0]); store_w(0, 0, 1, rb[0]);
  __syncthreads();
  for (int c = c0; c < c1; ++c) {
    const int n_out = min(c * 64 + wn * 32 + fr, N - 1);
    const float bias = g.bias ? g.bias[n_out] : 0.f;
#pragma unroll
    for (int j = 0; j < NKT; ++j) {  // straight-line walk over the k-tiles of column tile c
      constexpr int PP = 8;
      const int buf = j & 1;
      // tile (c, j) multiplies; tile (c, j + 2) - or (c + 1, j + 2 - NKT) - is requested into the set tile (c, j) came
      // from; tile (c, j + 1) - or (c + 1, 0) - moves from its set to the other LDS buffer
      const int lc = j + 2 < NKT ? c : c + 1, lj = (j + 2) % NKT, sj = (j + 1) % NKT;
      const float* ap = &As[wm * 32 + fr][j * BK + fk];
      const float* bp = &Bs[buf][wn * 32 + fr][fk];
      float a0 = ap[0], a1 = ap[2], b0 = bp[0], b1 = bp[2];
#pragma unroll
      for (int pr = 0; pr < PP; ++pr) {
        float na0 = 0.f, na1 = 0.f, nb0 = 0.f, nb1 = 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc, 0, 0, 0);
        if (pr < PP - 1) {
          na0 = ap[4 * pr + 4]; na1 = ap[4 * pr + 6];
          nb0 = bp[4 * pr + 4]; nb1 = bp[4 * pr + 6];
        }
        __builtin_amdgcn_sched_barrier(0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc, 0, 0, 0);
        if (pr < 2) load_w(lc, lj, pr, rb[j & 1]);
        else if (pr >= 4 && pr < 6) store_w(buf ^ 1, sj, pr - 4, rb[(j + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;
      }
      __syncthreads();
    }
    // outputs of column tile c (plain epilogue); the next tile's first weight tile is already staged
    const int n = c * 64 + wn * 32 + fr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
      float x = g.alpha * (acc[r] + bias);
      if (g.relu) x = fmaxf(x, 0.f);
      if (n < N && m < M) g.c[(int64_t)crow[r] * g.ldc + n] = x;
      acc[r] = 0.f;
    }
  }
}
// ... and for LARGE launches of such products (C5 shape: the query rows of 81 k positive nodes, K = 256 -> N = 1 024; fc2,
// K = N = 256 over 197 k rows), where the register-blocked 128 x 64 blocks re-stage their activation tile for every
// column tile and drain between tiles: eight wavefronts (4 row x 2 column) around a 128-row panel that stays in LDS
// (131 KB at K = 256) while `cpb` column tiles of weights stream through the two-buffer pipeline - 8 KB staged per
// k-tile instead of 24 KB, one float4 per thread.  One block per CU, two wavefronts per SIMD.
template <int NKT>
__global__ void __launch_bounds__(512) k_gemm_astat8(GemmArgs g, int cpb) {
  static_assert(NKT % 2 == 0, "the LDS buffer of a weight tile follows from its k-tile index");
  constexpr int SA = NKT * BK + 1;  // panel row stride (odd)
  __shared__ float As[128][SA];
  __shared__ float Bs[2][64][LDK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 31, fk = lane >> 5;
  const int K = g.k, N = g.n;
  int64_t M = g.m_cap;
  if (g.m_dev) M = min(M, (int64_t)*g.m_dev);
  const int NT = (N + 63) / 64, NG = (NT + cpb - 1) / cpb;
  const int xcd = blockIdx.x & 7, s_ = blockIdx.x >> 3;
  const int64_t mt = (int64_t)(s_ / NG) * 8 + xcd;
  const int c0 = (s_ % NG) * cpb, c1 = min(c0 + cpb, NT);
  const int64_t m0 = mt * 128;
  if (m0 >= M) return;
  const int ar = tid >> 3, ac4 = (tid & 7) * 4;  // 64 rows x 8 float4 per pass
  int crow[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t m = min(m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk, M - 1);
    crow[r] = g.c_rows ? g.c_rows[m] : (int)m;
  }
  {  // the activation panel, once
    float4 pa[2][NKT];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int64_t m = min(m0 + ar + 64 * i, M - 1);
      const float* row = g.a0.p + (g.a0.idx ? g.a0.idx[m] : m) * g.a0.ld;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        const int k = kt * BK + ac4;
        pa[i][kt] = ldg4(row + (k < K ? k : 0));
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) sts4(As[ar + 64 * i], kt * BK + ac4, kt * BK + ac4 < K ? pa[i][kt] : zero4());
  }
  float4 rb[2];  // weight tiles in flight: two register sets / two LDS buffers by the parity of the k-tile
  auto load_w = [&](int c, int j, float4& q) {
    const int cc = min(c, c1 - 1);
    const int k = j * BK + ac4;
    q = ldg4(g.w + (int64_t)min(cc * 64 + ar, N - 1) * g.ldw + (k < K ? k : 0));
  };
  auto store_w = [&](int buf, int j, const float4& q) { sts4(Bs[buf][ar], ac4, j * BK + ac4 < K ? q : zero4()); };
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  load_w(c0, 0, rb[0]);
  load_w(c0, 1, rb[1]);
  store_w(0, 0, rb[0]);
  __syncthreads();
  for (int c = c0; c < c1; ++c) {
    const int n_out = min(c * 64 + wn * 32 + fr, N - 1);
    const float bias = g.bias ? g.bias[n_out] : 0.f;
#pragma unroll
    for (int j = 0; j < NKT; ++j) {
      constexpr int PP = 8;
      const int buf = j & 1;
      const int lc = j + 2 < NKT ? c : c + 1, lj = (j + 2) % NKT, sj = (j + 1) % NKT;
      const float* ap = &As[wm * 32 + fr][j * BK + fk];
      const float* bp = &Bs[buf][wn * 32 + fr][fk];
      float a0 = ap[0], a1 = ap[2], b0 = bp[0], b1 = bp[2];
#pragma unroll
      for (int pr = 0; pr < PP; ++pr) {
        float na0 = 0.f, na1 = 0.f, nb0 = 0.f, nb1 = 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc, 0, 0, 0);
        if (pr < PP - 1) {
          na0 = ap[4 * pr + 4]; na1 = ap[4 * pr + 6];
          nb0 = bp[4 * pr + 4]; nb1 = bp[4 * pr + 6];
        }
        __builtin_amdgcn_sched_barrier(0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc, 0, 0, 0);
        if (pr == 0) load_w(lc, lj, rb[j & 1]);
        else if (pr == 4) store_w(buf ^ 1, sj, rb[(j + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;
      }
      __syncthreads();
    }
    const int n = c * 64 + wn * 32 + fr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
      float x = g.alpha * (acc[r] + bias);
      if (g.relu) x = fmaxf(x, 0.f);
      if (n < N && m < M) g.c[(int64_t)crow[r] * g.ldc + n] = x;
      acc[r] = 0.f;
    }
  }
}

// ---- weight-stationary, LDS-free blocks for short-K products with MANY rows ----------------------------------------------
// C5 shape: fc2 (196 608 x 256 -> 256) and the query rows (81 000 x 256 -> 1 024).  Every LDS-staged form pays a barrier per
// 32-k tile - 16 .. 32 MFMAs per wavefront between barriers - and reached 0.59 / 0.70 of the matrix peak there.  With K this
// short a wavefront can keep its WEIGHTS in registers for the whole launch: lane (i, kq) of a 16 x 16 x 4 MFMA holds the
// 16-byte chunks kq, kq + 4, .. of weight row n0 + i for CW column sets (gemm_direct_tile's operand form: K = 256, 32 columns
// = 128 registers) and walks row tiles of 16: the tile's activation chunks sit in a ring of NS registers, and the moment
// the 4 CW MFMAs of slot s have consumed chunk s of this tile the same register receives chunk s of the NEXT tile - a load
// has a whole tile's MFMAs (128 at K = 256, ~4 000 cycles) to arrive.  No LDS, no barrier, one load per eight MFMAs.
// A block is four wavefronts = four adjacent 32-column groups over the SAME row tiles (their activation loads meet in the
// CU's cache); persistent grid of two blocks per CU; the blocks of one row lane sit on one XCD (blockIdx % 8).
// Plain epilogue (bias, alpha, ReLU, scattered rows), gathered A rows.
template <int NS, bool CROWS, bool IDX>
__global__ void __launch_bounds__(256, 2) k_gemm_wstat(GemmArgs g) {
  constexpr int CW = 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int K = g.k, N = g.n;
  const int nch = K / 4;
  int64_t M = g.m_cap;
  if (g.m_dev) M = min(M, (int64_t)*g.m_dev);
  if (M <= 0) return;
  const int NG = (N + 127) / 128;                       // column groups of a block (4 wavefronts x 32 columns)
  const int xcd = blockIdx.x & 7, seq = blockIdx.x >> 3;
  const int cg = seq % NG;
  const int64_t lane_row = xcd + 8 * (int64_t)(seq / NG);   // this block's row lane
  const int64_t n_lanes = 8 * (int64_t)((gridDim.x >> 3) / NG);
  if (seq / NG >= (int)((gridDim.x >> 3) / NG)) return;     // (grid not a multiple of 8 NG: the surplus blocks idle)
  const int n0 = cg * 128 + wave * 32;
  if (n0 >= N) return;
  const int64_t MT = (M + 15) / 16;
  auto kc = [&](int s_) { return 4 * min(lk + 4 * s_, nch - 1); };  // element offset of this lane's chunk in slot s (clamped into the row)
  // ---- the weights, once (a clamped chunk past K repeats the last one: zeroed, it must not count twice)
  float4 w[CW][NS];
#pragma unroll
  for (int c = 0; c < CW; ++c) {
    const float* row = g.w + (int64_t)min(n0 + 16 * c + li, N - 1) * g.ldw;
#pragma unroll
    for (int s_ = 0; s_ < NS; ++s_) {
      const float4 v = ldg4(row + kc(s_));
      w[c][s_] = (lk + 4 * s_ < nch) ? v : zero4();
    }
  }
  float bias[CW];
#pragma unroll
  for (int c = 0; c < CW; ++c) bias[c] = g.bias ? g.bias[min(n0 + 16 * c + li, N - 1)] : 0.f;
  auto arow_id = [&](int64_t mt) {  // the row of A this lane reads in row tile mt (IDX: gathered - a load)
    const int64_t m = min(mt * 16 + li, M - 1);
    if constexpr (IDX) return (int64_t)g.a0.idx[m];
    else return m;
  };
  auto arow = [&](int64_t mt) { return g.a0.p + arow_id(mt) * g.a0.ld; };
  int64_t mt = lane_row;
  if (mt >= MT) return;
  // ring of RS chunk registers: chunk s lives in a[s % RS]; once slot s is multiplied its register receives chunk s + RS - of
  // this tile, or of the next one (K = 256: half a tile = 64 MFMAs ahead; a full-tile ring spills at 256 registers)
  constexpr int RS = (NS > 8 && NS % 2 == 0) ? NS / 2 : NS;  // (the ring is consistent only when RS divides NS)
  float4 a[RS];
  const float* crow_p = arow(mt);
#pragma unroll
  for (int s_ = 0; s_ < RS; ++s_) a[s_] = ldg4(crow_p + kc(s_));
  // One tile: 4 CW NS MFMAs with the next tile's chunk loads threaded between them, then the stores.  The loop body must
  // hold NO branch around a memory instruction (a join makes the wait-count pass wait for everything in flight - the ring
  // lives on loads that stay in flight across a whole tile): full tiles store unconditionally (FULL), the ragged last row
  // tile / column group takes the predicated copy of the body.
  auto tile = [&](auto full_tag, int64_t mt_, int64_t mt_next) {
    constexpr bool FULL = decltype(full_tag)::value;
    const float* const trow = crow_p;  // this tile's rows (the second half of its chunks is still to be requested)
    // the next tile's row id and this tile's output rows are requested FIRST: loads complete in order, so waiting for
    // them later must not mean waiting for the chunk loads that follow
    const int64_t nid = arow_id(mt_next);
    int orow_[4];
    if constexpr (CROWS) {
#pragma unroll
      for (int q = 0; q < 4; ++q) orow_[q] = g.c_rows[min(mt_ * 16 + 4 * lk + q, M - 1)];
    }
    const float* nrow = nullptr;
    f32x4m acc[CW];
#pragma unroll
    for (int c = 0; c < CW; ++c) acc[c] = f32x4m{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s_ = 0; s_ < NS; ++s_) {
      const float4 x = a[s_ % RS];
      const float av[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < CW; ++c) {
          const float wv = j == 0 ? w[c][s_].x : j == 1 ? w[c][s_].y : j == 2 ? w[c][s_].z : w[c][s_].w;
          acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], wv, acc[c], 0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
      // chunk s + RS into the register this slot has just been multiplied from
      if (s_ + RS == NS || (RS == NS && s_ == 0)) nrow = g.a0.p + nid * g.a0.ld;
      a[s_ % RS] = (s_ + RS < NS) ? ldg4(trow + kc(s_ + RS)) : ldg4(nrow + kc(s_ + RS - NS));
      __builtin_amdgcn_sched_barrier(0);
    }
    crow_p = nrow;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t m = mt_ * 16 + 4 * lk + q;
      int64_t orow = m;
      if constexpr (CROWS) orow = orow_[q];
      float* dst = g.c + orow * g.ldc + n0 + li;
#pragma unroll
      for (int c = 0; c < CW; ++c) {
        float x = g.alpha * (acc[c][q] + bias[c]);
        if (g.relu) x = fmaxf(x, 0.f);
        if (FULL) dst[16 * c] = x;
        else if (n0 + 16 * c + li < N && m < M) dst[16 * c] = x;
      }
    }
  };
  using Full = std::integral_constant<bool, true>;
  using Ragged = std::integral_constant<bool, false>;
  const bool cols_full = n0 + 32 <= N;  // wave-uniform
  if (cols_full) {
    for (; (mt + 1) * 16 <= M; mt += n_lanes) {
      const int64_t mt_next = mt + n_lanes < MT ? mt + n_lanes : mt;  // past the end: a redundant reload of this tile
      tile(Full{}, mt, mt_next);
    }
  }
  for (; mt < MT; mt += n_lanes) {
    const int64_t mt_next = mt + n_lanes < MT ? mt + n_lanes : mt;
    tile(Ragged{}, mt, mt_next);
  }
}

template <int NKT>
__global__ void __launch_bounds__(256) k_gemm_astat(GemmArgs g, int cpb) {
  gemm_astat_block<NKT>(g, cpb, blockIdx.x);
}
template <class R, int NKT>
__global__ void __launch_bounds__(256) k_gemm_astat_r(GemmArgs g, int cpb, R r) {
  const unsigned own = gridDim.x - r.blocks;  // the product's blocks: before the riders (r.last) or after them
  if (r.last ? blockIdx.x >= own : blockIdx.x < r.blocks) {
    r.run(r.last ? blockIdx.x - own : blockIdx.x);
    return;
  }
  gemm_astat_block<NKT>(g, cpb, r.last ? blockIdx.x : blockIdx.x - r.blocks);
}

// ---- LDS-free blocks for short-K products with few rows ---------------------------------------------------------------
// The query-row product of the eager step (G_v = c_v Wqk^T + gconst for the ~1 000 positive nodes of a C2 batch: K = d,
// N = n_head (2d + d_e)) is 0.37 GFLOP - 3 us of the matrix pipe - but took 12.8 us as activation-stationary blocks: panel
// through LDS, twelve weight tiles through the two-buffer pipeline, a barrier per tile.  With K this short a wavefront can
// hold its WHOLE operands in registers: lane (i, kq) of a 16 x 16 x 4 MFMA loads the 16-byte chunks kq, kq + 4, kq + 8, ..
// of row i - every chunk of a row exactly once over the four lane quarters - for each of its RW row sets and CW weight-row
// sets, all loads issued back to back (ONE exposed memory latency per block), then NS x 4 x RW x CW MFMAs (step (s, j)
// multiplies element j of chunk slot s on both operands: the sum over k does not care which k values share a step).  No
// LDS, no barrier.  Four wavefronts per block own 2 x 2 wave tiles; a row tile's blocks run on one XCD (chunks of the tile
// sequence, as k_gru_direct16); the grid is 256 persistent blocks sized for the live rows.  Plain epilogue (bias, alpha,
// ReLU, scattered rows).
template <int NS, int RW, int CW>
__device__ __forceinline__ void gemm_direct_tile(const GemmArgs& g, int64_t M, int64_t m0, int n0) {
  TG_PT(const unsigned long long pt_entry = (g.dbg & 16) ? __builtin_amdgcn_s_memtime() : 0ull;)  // (diagnostic, as in gemm_ks16_tile)
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int K = g.k, N = g.n;
  const int nch = K / 4;  // 16-byte chunks per row
  float4 a[RW][NS], w[CW][NS];
  unsigned livem = 0u;    // bit s: chunk slot s of this lane quarter lies inside K
#pragma unroll
  for (int s_ = 0; s_ < NS; ++s_)
    if (lk + 4 * s_ < nch) livem |= 1u << s_;
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    const int64_t m = min(m0 + 16 * r + li, M - 1);
    const float* row = g.a0.p + (g.a0.idx ? g.a0.idx[m] : m) * g.a0.ld;
#pragma unroll
    for (int s_ = 0; s_ < NS; ++s_) a[r][s_] = ldg4(row + 4 * min(lk + 4 * s_, nch - 1));
  }
#pragma unroll
  for (int c = 0; c < CW; ++c) {
    const float* row = g.w + (int64_t)min(n0 + 16 * c + li, N - 1) * g.ldw;
#pragma unroll
    for (int s_ = 0; s_ < NS; ++s_) w[c][s_] = ldg4(row + 4 * min(lk + 4 * s_, nch - 1));
  }
  float bias[CW];
  int crow[RW][4], c2r[RW][4];
  const bool two = g.c2 && m0 < g.c2_m;  // second destination (write-back rider: STEP 6's rows), wave-uniform
  f32x4m acc[RW][CW];
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int c = 0; c < CW; ++c) acc[r][c] = f32x4m{0.f, 0.f, 0.f, 0.f};
  TG_PT(const unsigned long long pt_loop0 = (g.dbg & 16) ? __builtin_amdgcn_s_memtime() : 0ull;)
#pragma unroll
  for (int s_ = 0; s_ < NS; ++s_) {
    if (s_ == NS / 2) {
      // epilogue operands (bias of this lane's column in each column set, output rows): requested here, behind half of the
      // MFMAs - early enough to arrive before the epilogue, late enough that the operand registers of the slots already
      // consumed are free (requested with the operands they push the kernel past 256 registers: one block per CU)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < CW; ++c) bias[c] = g.bias ? g.bias[min(n0 + 16 * c + li, N - 1)] : 0.f;
#pragma unroll
      for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int64_t m = min(m0 + 16 * r + 4 * lk + q, M - 1);
          crow[r][q] = g.c_rows ? g.c_rows[m] : (int)m;
          c2r[r][q] = two ? g.c2_rows[min(m, g.c2_m - 1)] : -1;
        }
      __builtin_amdgcn_sched_barrier(0);
    }
    const bool lv = (livem >> s_) & 1u;
    float av[RW][4], wv[CW][4];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const float4 x = lv ? a[r][s_] : zero4();  // (a clamped chunk past K repeats the last one: it must not count twice)
      av[r][0] = x.x; av[r][1] = x.y; av[r][2] = x.z; av[r][3] = x.w;
    }
#pragma unroll
    for (int c = 0; c < CW; ++c) {
      wv[c][0] = w[c][s_].x; wv[c][1] = w[c][s_].y; wv[c][2] = w[c][s_].z; wv[c][3] = w[c][s_].w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < RW; ++r)
#pragma unroll
        for (int c = 0; c < CW; ++c)
          acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r][j], wv[c][j], acc[r][c], 0, 0, 0);
  }
  TG_PT(unsigned long long pt_loop1 = 0ull; if (g.dbg & 16) {
    asm volatile("s_nop 0" ::"v"(acc[0][0][0]));
    pt_loop1 = __builtin_amdgcn_s_memtime();
  })
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int c = 0; c < CW; ++c) {
      const int n = n0 + 16 * c + li;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t m = m0 + 16 * r + 4 * lk + q;
        float x = g.alpha * (acc[r][c][q] + bias[c]);
        if (g.relu) x = fmaxf(x, 0.f);
        if (n < N && m < M) {
          g.c[(int64_t)crow[r][q] * g.ldc + n] = x;
          if (two && m < g.c2_m && c2r[r][q] >= 0) g.c2[(int64_t)c2r[r][q] * g.ldc2 + n] = x;
        }
      }
    }
  TG_PT(if ((g.dbg & 16) && threadIdx.x == 0 && blockIdx.x < 4096) {
    g_gemm_trace[blockIdx.x * 4 + 0] = pt_entry;
    g_gemm_trace[blockIdx.x * 4 + 1] = pt_loop0;
    g_gemm_trace[blockIdx.x * 4 + 2] = pt_loop1;
    g_gemm_trace[blockIdx.x * 4 + 3] = __builtin_amdgcn_s_memtime();
  })
}

// block = 2 x 2 wavefronts of (16 RW) x (16 CW) wave tiles; `own` persistent blocks (riders, if any, sit behind them)
template <int NS, int RW, int CW>
__device__ __forceinline__ void gemm_direct_block(const GemmArgs& g, unsigned bid, unsigned own) {
  int64_t M = g.m_cap;
  if (g.m_dev) M = min(M, (int64_t)*g.m_dev);
  if (M <= 0) return;
  constexpr int BM = 32 * RW, BN = 32 * CW;
  const int NT = (g.n + BN - 1) / BN;
  const int64_t total = ((M + BM - 1) / BM) * NT;
  const int64_t per = (total + 7) / 8;  // XCD x works through the chunk [x per, (x + 1) per) of the tile sequence
  const int wave = threadIdx.x >> 6;
  for (int64_t jx = bid >> 3; jx < per; jx += own >> 3) {
    const int64_t b = (int64_t)(bid & 7) * per + jx;
    if (b >= total) break;
    const int64_t mt = b / NT;
    const int nt = (int)(b - mt * NT);
    const int64_t m0 = mt * BM + (wave >> 1) * (16 * RW);
    const int n0 = nt * BN + (wave & 1) * (16 * CW);
    if (m0 < M && n0 < g.n) gemm_direct_tile<NS, RW, CW>(g, M, m0, n0);
  }
}
template <int NS, int RW, int CW>
__global__ void __launch_bounds__(256) k_gemm_direct(GemmArgs g) {
  gemm_direct_block<NS, RW, CW>(g, blockIdx.x, gridDim.x);
}
template <class R, int NS, int RW, int CW>
__global__ void __launch_bounds__(256) k_gemm_direct_r(GemmArgs g, R r) {
  const unsigned own = gridDim.x - r.blocks;  // riders behind the product's blocks
  if (blockIdx.x >= own) {
    r.run(blockIdx.x - own);
    return;
  }
  gemm_direct_block<NS, RW, CW>(g, blockIdx.x, own);
}

// ... and a second product `g2` of the same family beside the first: its 64 x 64 tiles (2 x 2 wave tiles, the instance a launch
// of its own takes at these sizes - same chunk slots, same k order per lane, hence the same bits) are dealt to `own2`
// workgroups behind the first product's, in front of the riders.  own and own2 are multiples of 8: both XCD maps are those
// of the separate launches.  The two products are independent (neither reads what the other writes).
template <class R, int NS, int RW, int CW>
__global__ void __launch_bounds__(256) k_gemm_direct_r2(GemmArgs g, GemmArgs g2, unsigned own2, R r) {
  const unsigned own = gridDim.x - r.blocks - own2;
  if (blockIdx.x >= own + own2) {
    r.run(blockIdx.x - own - own2);
    return;
  }
  if (blockIdx.x >= own) gemm_direct_block<NS, 2, 2>(g2, blockIdx.x - own, own2);
  else gemm_direct_block<NS, RW, CW>(g, blockIdx.x, own);
}

// ---- LDS-free K-split blocks for long-K products with few tiles ------------------------------------------------------
// The merged value / out / fc1 product of the fused attention (C2: M = 3 072, N = 172, K = 1 204) has 144 tiles of 64 x 64
// for 256 CUs; as stream-K pieces (below) it fills the chip but leaves its result in two or three pieces per element for
// the consumer to sum.  This is k_gru_direct16's scheme with one plane: a block owns (16 RT) x (16 CT) outputs - 48 x 48
// makes 64 x 4 = 256 blocks of exactly that product - the 32-k tiles are dealt to NW wavefronts, lane (i, kq) of a
// 16 x 16 x 4 MFMA feeds the matrix unit from the 32 contiguous bytes A[i][k0 + 8 kq ..] / W[j][k0 + 8 kq ..] it loads
// itself (no LDS in the k-loop; A may be two column segments, rows optionally gathered), the wavefronts' accumulators meet
// in one reduce-scatter round through LDS (summed in wavefront order: bit-reproducible) and the first four wavefronts
// run the epilogue (bias, second bias on valid rows, alpha, ReLU) - the product leaves its final values, so its consumer
// is a plain product.  256 persistent blocks, XCD chunks of the tile sequence.
template <int RT, int CT, int NW>
__device__ __forceinline__ void gemm_ks16_tile(const GemmArgs& g, int64_t M, int64_t m0, int n0, float* sc_raw) {
  constexpr int NS = RT * CT;  // 16 x 16 subtiles of the block
  // diagnostic only (g.dbg & 16; tools/phase_budget.py): s_memtime stamps {entry, first tile requested, k-loop done, exit}
  // of the block's first tile, wavefront 0
  TG_PT(const unsigned long long pt_entry = (g.dbg & 16) ? __builtin_amdgcn_s_memtime() : 0ull;)
  float (*sc)[NW - 1][NS][64] = reinterpret_cast<float (*)[NW - 1][NS][64]>(sc_raw);  // [owner 0..3][slot][subtile][lane]
  const int tid = threadIdx.x, lane = tid & 63, ks = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int K = g.k, N = g.n, kw0 = g.a0.w;
  const float* ar0[RT];
  const float* ar1[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int64_t m = min(m0 + 16 * rt + li, M - 1);
    ar0[rt] = g.a0.p + (g.a0.idx ? g.a0.idx[m] : m) * g.a0.ld;
    ar1[rt] = g.a1.p ? g.a1.p + (g.a1.idx ? g.a1.idx[m] : m) * g.a1.ld - kw0 : ar0[rt];
  }
  const float* wr[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) wr[ct] = g.w + (int64_t)min(n0 + 16 * ct + li, N - 1) * g.ldw;
  const int nkt = (K + BK - 1) / BK;
  const int n_my = ks < nkt ? (nkt - ks + NW - 1) / NW : 0;
  struct Tile {
    float4 a[RT][2], w[CT][2];
  };
  // raw loads from clamped addresses (see k_gru_direct), split in two: the addresses of a tile, then its 2 (RT + CT)
  // loads one at a time - threaded between the MFMAs of the tile before (a burst of twelve loads in front of a tile's 72
  // MFMAs holds the matrix pipe for the time it takes to issue them)
  struct Addr {
    int kc[2];
    unsigned live;
  };
  auto tile_addr = [&](int i, Addr& A) {
    const int t = ks + NW * max(0, min(i, n_my - 1));
    const int kb = min(t, nkt - 1) * BK + 8 * lk;
    A.live = 0u;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int k = kb + 4 * q;
      if (k < K && ks < nkt) A.live |= 1u << q;
      A.kc[q] = k < K ? k : 0;
    }
  };
  auto load_one = [&](int l, const Addr& A, Tile& T) {  // l = 0 .. 2 (RT + CT) - 1
    const int q = l & 1, r = l >> 1;
    if (r < RT) {
      const int k = A.kc[q];
      T.a[r][q] = ldg4((k < kw0 ? ar0[r] : ar1[r]) + k);
    } else {
      T.w[r - RT][q] = ldg4(wr[r - RT] + A.kc[q]);
    }
  };
  f32x4m acc[RT][CT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f32x4m{0.f, 0.f, 0.f, 0.f};
  constexpr int NL = 2 * (RT + CT), NM = 8 * RT * CT;  // loads / MFMAs per tile
  // multiply tile T (live mask lv) and, threaded through it, request the next tile (addresses An) into Tn
  auto mma_tile = [&](const Tile& T, unsigned lv, const Addr& An, Tile& Tn, bool prefetch) {
    int mi = 0, li_ = 0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      float av[RT][4], wv[CT][4];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const float4 a = ((lv >> q) & 1u) ? T.a[rt][q] : zero4();
        av[rt][0] = a.x; av[rt][1] = a.y; av[rt][2] = a.z; av[rt][3] = a.w;
      }
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        wv[ct][0] = T.w[ct][q].x; wv[ct][1] = T.w[ct][q].y; wv[ct][2] = T.w[ct][q].z; wv[ct][3] = T.w[ct][q].w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) {
            acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][j], wv[ct][j], acc[rt][ct], 0, 0, 0);
            ++mi;
            if (prefetch && li_ < NL && mi * NL >= (li_ + 1) * NM / 2) {  // the loads ride in the first half of the tile
              load_one(li_, An, Tn);
              ++li_;
              __builtin_amdgcn_sched_barrier(0);
            }
          }
    }
  };
  // epilogue operands of the outputs wavefront ks < 4 finishes (accumulator register ks of every subtile: row 4 lk + ks),
  // requested before the loop
  float bias[CT], bias2[CT];
  uint8_t v2[RT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const int n = min(n0 + 16 * ct + li, N - 1);
    bias[ct] = g.bias ? g.bias[n] : 0.f;
    bias2[ct] = g.bias2 ? g.bias2[n] : 0.f;
  }
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) v2[rt] = g.bias2 ? g.bias2_valid[min(m0 + 16 * rt + 4 * lk + (ks & 3), M - 1)] : 0;
  // (ablations at C2's fc1 shape, 3 072 x 1 204 -> 172: loads alone 7.2 us, MFMAs alone 16.6 us, both 19.6 us - the block is
  // bound by its four wavefronts' MFMA streams, 720 dependent-free MFMAs of 32 cycles each; a third register set, two
  // tiles ahead, costs the second block per CU and is slower: 20.4 us)
  Tile T0, T1;
  Addr A0, A1;
  tile_addr(0, A0);
#pragma unroll
  for (int l = 0; l < NL; ++l) load_one(l, A0, T0);
  TG_PT(const unsigned long long pt_loop0 = (g.dbg & 16) ? __builtin_amdgcn_s_memtime() : 0ull;)
  int i = 0;
  for (; i + 2 <= n_my; i += 2) {
    tile_addr(i + 1, A1);
    __builtin_amdgcn_sched_barrier(0);
    mma_tile(T0, A0.live, A1, T1, true);
    __builtin_amdgcn_sched_barrier(0);
    tile_addr(i + 2, A0);
    __builtin_amdgcn_sched_barrier(0);
    mma_tile(T1, A1.live, A0, T0, true);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (i < n_my) mma_tile(T0, A0.live, A1, T1, false);
  TG_PT(unsigned long long pt_loop1 = 0ull; if (g.dbg & 16) {  /* the stamp waits for the last MFMA */
    asm volatile("s_nop 0" ::"v"(acc[0][0][0]));
    pt_loop1 = __builtin_amdgcn_s_memtime();
  })
  // reduce-scatter: wavefront v < 4 finishes accumulator register v of every subtile; everybody parks the registers the
  // others own (one round, one barrier); sums run in wavefront order 0 .. NW - 1
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    if (v != ks) {  // wave-uniform
      const int slot = ks < v ? ks : ks - 1;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) sc[v][slot][rt * CT + ct][lane] = acc[rt][ct][v];
    }
  }
  __syncthreads();
  if (ks >= 4) return;
  float o[RT][CT];
#pragma unroll
  for (int src = 0; src < NW; ++src) {
    float t[RT][CT];
    if (src == ks) {  // wave-uniform
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if (v == ks) {
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) t[rt][ct] = acc[rt][ct][v];
        }
    } else {
      const int slot = src < ks ? src : src - 1;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) t[rt][ct] = sc[ks][slot][rt * CT + ct][lane];
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) o[rt][ct] = src == 0 ? t[rt][ct] : o[rt][ct] + t[rt][ct];
  }
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int64_t m = m0 + 16 * rt + 4 * lk + ks;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int n = n0 + 16 * ct + li;
      float x = g.alpha * (o[rt][ct] + bias[ct] + (v2[rt] ? bias2[ct] : 0.f));
      if (g.relu) x = fmaxf(x, 0.f);
      if (n < N && m < M) g.c[m * g.ldc + n] = x;
    }
  }
  TG_PT(if ((g.dbg & 16) && tid == 0 && blockIdx.x < 4096) {
    g_gemm_trace[blockIdx.x * 4 + 0] = pt_entry;
    g_gemm_trace[blockIdx.x * 4 + 1] = pt_loop0;
    g_gemm_trace[blockIdx.x * 4 + 2] = pt_loop1;
    g_gemm_trace[blockIdx.x * 4 + 3] = __builtin_amdgcn_s_memtime();
  })
}

// persistent blocks of one product: block `bid` of `nblk` (a multiple of 8) works through its XCD's chunk of the tile sequence
template <int RT, int CT, int NW>
__device__ __forceinline__ void gemm_ks16_blocks(const GemmArgs& g, unsigned bid, unsigned nblk, float* sc_raw) {
  int64_t M = g.m_cap;
  if (g.m_dev) M = min(M, (int64_t)*g.m_dev);
  if (M <= 0) return;
  constexpr int BM = 16 * RT, BN = 16 * CT;
  const int NT = (g.n + BN - 1) / BN;
  const int64_t total = ((M + BM - 1) / BM) * NT;
  const int64_t per = (total + 7) / 8;
  for (int64_t jx = bid >> 3; jx < per; jx += nblk >> 3) {
    const int64_t b = (int64_t)(bid & 7) * per + jx;
    if (b >= total) break;
    const int64_t mt = b / NT;
    const int nt = (int)(b - mt * NT);
    gemm_ks16_tile<RT, CT, NW>(g, M, mt * BM, nt * BN, sc_raw);
    __syncthreads();  // the fold's LDS is re-used by the next tile
  }
}
template <class R, int RT, int CT, int NW>
__global__ void __launch_bounds__(64 * NW) k_gemm_ks16(GemmArgs g, R r) {
  __shared__ float sc_raw[4 * (NW - 1) * RT * CT * 64];
  const unsigned own = gridDim.x - r.blocks;  // persistent blocks of the product; riders behind them
  if (blockIdx.x >= own) {
    r.run(blockIdx.x - own);
    return;
  }
  gemm_ks16_blocks<RT, CT, NW>(g, blockIdx.x, own, sc_raw);
}

// Is the product one for k_gemm_ks16?  Long K, plain epilogue (+ second bias), few enough 48 x 48 tiles that the blocks
// fit the chip in one round or two.  TG_GEMM_KS16: 0 = off, 8 = eight wavefronts per block.
// What the "plain epilogue" conditions of the specialised kernels have in common: one unbatched product, W row-major, A read
// from memory (no stream-K pieces), no per-row bias scale / validity / ReLU mask and no C +=.  Each site spells out its
// own further terms (bias2, c_rows, c2, a1, ...): they differ on purpose.
static bool plain_epilogue(const GemmArgs& g) {
  return !g.ask_part && g.nbatch == 1 && !g.w_kmajor && !g.bias_rs && !g.row_valid && !g.relu_mask && !g.accumulate;
}
static unsigned rider_blocks(int64_t live, int threads, int64_t rows);  // (below, with gemm_launch)
struct NoRider {  // (k_gemm_ks16 without riders)
  unsigned blocks;
  __device__ __forceinline__ void run(unsigned) const {}
};
// diagnostic stand-in for a rider (tg_debug_gemm2): rider workgroup b of `blocks` stamps its share of out[0, n) - every
// word exactly once if and only if the launch hands each rider its own index in [0, blocks)
struct FillRider {
  unsigned blocks;
  uint32_t* out;
  int64_t n;
  __device__ __forceinline__ void run(unsigned bid) const {
    for (int64_t i = (int64_t)bid * blockDim.x + threadIdx.x; i < n; i += (int64_t)blocks * blockDim.x)
      atomicAdd(out + i, 0x10000u + bid);
  }
};
bool gemm_ks16_launch(const GemmArgs& g, hipStream_t st, const WbRider* rider, bool* rode, bool dry) {
  static const int knob = env_int("TG_GEMM_KS16", 1);
  if (rode) *rode = false;
  if (!knob || g.m_cap <= 0 || !plain_epilogue(g) || g.c_rows || g.c2 || (g.k % 4) || (g.a0.w % 4) || (g.ldw % 4) ||
      g.a0.w + (g.a1.p ? g.a1.w : 0) != g.k)
    return false;
  // column tiles of 48 (CT = 3), or - narrow outputs (N <= 112, e.g. LastFM's --dim 100: 64-column tiles waste 28 % of the
  // MFMAs, 48-column tiles 44 %) - ONE column tile of 16 CT = 64 / 112 columns with 32-row blocks
  const int ct = g.n <= 64 ? 4 : g.n <= 112 ? 7 : 3;
  // (measured, N = 100: 24 576 x 500 42.2 -> 39.6 us, 6 144 x 500 17.7 -> 13.3 us, 600 x 500 16.6 -> 9.2 us; 3 072 x 400 -> 64
  // 14.5 -> 6.4 us; at K = 300 the 64 x 64 blocks are faster: 27.9 against 30.9 us)
  // (a launch of at most one 48 x 48 block per CU pays from K = 320: the score head's product, 2 B x 2 d -> d, at d = 172
  // 2 048 rows 13.3 -> 6.8 us, 400 rows 12.9 -> 4.9 us against the 64 x 64 LDS blocks; 4 096 rows and more: no gain)
  static const int mink_knob = env_int("TG_GEMM_KS16_MINK", 0);  // tuning knob
  const bool one_round = ct == 3 && cdiv(g.m_cap, 48) * cdiv(g.n, 48) <= 256;
  if (g.k < (mink_knob ? mink_knob : (ct == 3 ? (one_round ? 320 : 512) : 384))) return false;
  const int64_t ntc = cdiv(g.n, 16 * ct);
  static const int64_t max_tiles = env_int("TG_GEMM_KS16_TILES", 1100);  // tuning knob (measured, K = 1 204, N = 172: 6 144 rows 54.5 -> 37.1 us, 12 288 rows 78.2 -> 72.1 us, 24 576 rows 123 -> 129 us)
  if (cdiv(g.m_cap, ct == 3 ? 48 : 32) * ntc > max_tiles) return false;
  GemmArgs gd = g;
  static const int gdbg16 = env_int("TG_GEMM_DBG", 0) & 16;  // diagnostic: phase stamps
  gd.dbg = (gdbg16 && phase_selected(g)) ? 16 : 0;
  const NoRider nr{0u};
  if (ct != 3) {
    if (dry) return true;
    // (rows per block: 16 when that fits the chip at once, else 32)
    const bool r1 = cdiv(g.m_cap, 16) * ntc <= 256;
    if (ct == 4) {
      TG_FORM(r1 ? "ks16<1,4,4>" : "ks16<2,4,4>");
      if (r1) TG_KLAUNCH((k_gemm_ks16<NoRider, 1, 4, 4>), dim3(256), dim3(256), 0, st, gd, nr);
      else TG_KLAUNCH((k_gemm_ks16<NoRider, 2, 4, 4>), dim3(256), dim3(256), 0, st, gd, nr);
    } else {
      TG_FORM(r1 ? "ks16<1,7,4>" : "ks16<2,7,4>");
      if (r1) TG_KLAUNCH((k_gemm_ks16<NoRider, 1, 7, 4>), dim3(256), dim3(256), 0, st, gd, nr);
      else TG_KLAUNCH((k_gemm_ks16<NoRider, 2, 7, 4>), dim3(256), dim3(256), 0, st, gd, nr);
    }
    return true;
  }
  const int64_t nt48 = ntc;
  // rows per block: the smallest of 16 / 32 / 48 whose blocks fit the chip at once (fewer rows = a shorter block)
  const int rt = cdiv(g.m_cap, 16) * nt48 <= 256 ? 1 : cdiv(g.m_cap, 32) * nt48 <= 256 ? 2 : 3;
  if (rider && rode && knob != 8) {
    // the write-back rider (STEP 4-5 depend on nothing the attention block computes) on THIS launch, the longest of the
    // block: its chain of dependent round trips (~9 us) hides behind the product instead of extending fc2's launch
    // (C2: fc1 22.9 -> 25.8 us, fc2 + riders 16.8 -> 12.9 us; with the short blocks of a small batch fc2's launch hides the
    // rider as well and fc1 only gets longer: C1 13.1 -> 14.5 us)
    static const int here = env_int("TG_WB_RIDER_FC1", 1);  // tuning knob: 0 = on fc2
    if (here && rt == 3 && cdiv(g.m_cap, 48) * nt48 <= 256) {
      if (dry) {
        *rode = true;
        return true;
      }
      WbRider wr = *rider;
      const int64_t live = std::min<int64_t>(256, cdiv(g.m_cap, 16 * rt) * nt48);
      wr.blocks = rider_blocks(live, 256, 2 * wr.a.B);
      wr.last = 1u;
      const dim3 gr(256 + wr.blocks);
      TG_FORM("ks16<3,3,4>+wb");
      TG_KLAUNCH((k_gemm_ks16<WbRider, 3, 3, 4>), gr, dim3(256), 0, st, gd, wr);
      *rode = true;
      return true;
    }
  }
  if (dry) return true;
  TG_FORM(knob == 8 ? "ks16<3,3,8>" : rt == 1 ? "ks16<1,3,4>" : rt == 2 ? "ks16<2,3,4>" : "ks16<3,3,4>");
  if (knob == 8) TG_KLAUNCH((k_gemm_ks16<NoRider, 3, 3, 8>), dim3(256), dim3(512), 0, st, gd, nr);
  else if (rt == 1) TG_KLAUNCH((k_gemm_ks16<NoRider, 1, 3, 4>), dim3(256), dim3(256), 0, st, gd, nr);
  else if (rt == 2) TG_KLAUNCH((k_gemm_ks16<NoRider, 2, 3, 4>), dim3(256), dim3(256), 0, st, gd, nr);
  else TG_KLAUNCH((k_gemm_ks16<NoRider, 3, 3, 4>), dim3(256), dim3(256), 0, st, gd, nr);
  return true;
}

// ---- stream-K for launches that cannot fill the chip --------------------------------------------------
// A product with fewer 64x64 tiles than CUs and a long K (the merged value/out/fc1 product of the fused
// attention: 144 tiles x 38 k-tiles on 256 CUs) leaves CUs idle for its whole duration.  Here the
// (tile, k-tile) units are dealt evenly: worker w owns units [w U, (w+1) U) of the tile-major sequence, i.e.
// the tail of one tile and/or the head of the next, and stores each piece's accumulators in its own slot.
// Nobody waits for anybody: the pieces of a tile are summed, in worker order (a fixed order: deterministic),
// by the CONSUMER of the product while it stages its A operand (gemm_tile<..., ASK>), together with the
// producer's bias / activation.  U < nkt is required (every tile is split); with few tiles a tile is cut into up to
// eight pieces (consumer instance AP = 8), with 128 .. 255 tiles into two or three (AP = 3).
template <int KS, int D>
__global__ void __launch_bounds__(256 * KS) k_gemm_sk(GemmArgs g, SkPlan sk) {
  // Units are dealt per XCD (blockIdx % 8, as the hardware deals blocks): the row tiles mt = x (mod 8) belong to
  // XCD x, as in k_gemm's map, and so do the consumer's blocks of these rows - every piece is written and read
  // inside one XCD's L2 (32 workers x 2 slots x 16 KB = 1 MB of its 4 MB).
  const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
  const int64_t total = (int64_t)((sk.MT - x + 7) / 8) * sk.NT * sk.nkt;
  int64_t u = (int64_t)j * sk.U;
  const int64_t u1 = min(u + sk.U, total);
  int piece = 0;
  while (u < u1) {  // at most two pieces (U < nkt)
    const int lt = (int)(u / sk.nkt), kt0 = (int)(u % sk.nkt);
    const int kt1 = (int)min((int64_t)sk.nkt, kt0 + (u1 - u));
    gemm_tile<2, 2, KS, D>(g, (int64_t)(lt / sk.NT) * 8 + x, lt % sk.NT, 0, kt0, kt1,
                           sk.part + ((size_t)blockIdx.x * 2 + piece) * 4096, -1);
    __syncthreads();  // the LDS tiles are re-used by the next piece
    u += kt1 - kt0;
    ++piece;
  }
}

bool gemm_sk_partials(const GemmArgs& g, float* ws, size_t ws_floats, hipStream_t st, SkPlan* plan) {
  static const int sk_knob = env_int("TG_GEMM_SK", 1);  // tuning knob: 0 = off
  if (!sk_knob || !ws || g.m_cap <= 0 || g.nbatch != 1 || g.m_dev || (g.k % 4) || (g.a0.w % 4) || (g.ldw % 4) ||
      g.a0.w + (g.a1.p ? g.a1.w : 0) != g.k)
    return false;
  SkPlan p{};
  p.NT = (int)cdiv(g.n, 64);
  p.MT = (int)cdiv(g.m_cap, 64);
  p.tiles = p.MT * p.NT;
  p.nkt = (int)cdiv(g.k, BK);
  static const int wk_knob = env_int("TG_SK_WORKERS", TG_SK_WORKERS);  // tuning knob
  const int workers = std::min(std::max(wk_knob & ~7, 8), TG_SK_WORKERS_MAX);
  if (p.tiles >= TG_SK_WORKERS || p.nkt < 16) return false;  // (also covers few tiles: then a tile is cut into more pieces)
  const int64_t units_xcd = cdiv((int64_t)p.MT, 8) * p.NT * p.nkt;  // of the fullest XCD
  p.U = (int)cdiv(units_xcd, (int64_t)(workers / 8));
  p.pieces = (int)cdiv(p.nkt, p.U) + 1;  // most pieces a tile can be cut into (its range may start mid-worker)
  if (p.U >= p.nkt || p.pieces > 8 || p.U < 3 || ws_floats < (size_t)workers * 2 * 4096) return false;
  p.part = ws;
  static const int gdbg = env_int("TG_GEMM_DBG", 0);
  GemmArgs gd = g;
  gd.dbg = gdbg & ~16;
  TG_KLAUNCH((k_gemm_sk<2, 2>), dim3(workers), dim3(512), 0, st, gd, p);
  *plan = p;
  return true;
}

// Riders (WbRider, CollateRider) pay where the product's launch is small: its live blocks leave CUs idle (C2: 144 blocks of
// fc2 + 112 write-back riders, one block per CU either way) or fill the chip for a round or so.  Large launches take no
// rider - measured at C5 shape: the write-back as 512 riders of fc2 costs 240 us where its own launch takes 180 us, and
// the collate riders of the query-row product change nothing - the caller then launches that work itself.  `live`: the
// product's blocks that have rows (a launch may be sized for a capacity several times its live rows: GemmArgs.m_hint).
// Riders sit BEHIND the product's blocks in the grid: the dispatcher starts the product - the critical path - first, the
// riders take what is left.
constexpr int64_t RIDER_MAX_LIVE = 1024;
static int64_t live_blocks(const GemmArgs& g, int64_t grid, int bm) {
  if (g.m_hint <= 0 || g.m_hint >= g.m_cap) return grid;
  return std::max<int64_t>(1, grid * cdiv(g.m_hint, (int64_t)bm) / std::max<int64_t>(1, cdiv(g.m_cap, (int64_t)bm)));
}
// write-back riders: one wavefront per listed row at most; the idle CUs of an under-filled launch, else two per CU; a
// multiple of 8 (the product's XCD map stays)
static unsigned rider_blocks(int64_t live, int threads, int64_t rows) {
  const int64_t want = cdiv(rows, (int64_t)(threads / 64));
  const int64_t room = live <= 248 ? (256 - live) * (threads <= 256 ? 2 : 1) : 512;  // (idle CUs host two 4-wave blocks)
  return (unsigned)std::max<int64_t>(8, std::min(want, room) & ~(int64_t)7);
}
// collate riders: the sampler is a chain of dependent memory round trips per query and wants many wavefronts (its own
// launch has one group of 16 lanes per query); the centres are a gather with four elements per thread in flight
static void collate_blocks(CollateRider& c) {
  const int64_t Q = 3 * c.s.B;
  // (a centres pass that neither copies centre rows nor takes the snapshot walks no rows: one thread per centre for its checks)
  const bool walks = c.cr.out || c.cr.da.snap;
  const int64_t sg = cdiv(Q, (int64_t)16), cg = walks ? cdiv(Q * (c.cr.m.d / 4), (int64_t)256) : 4 * cdiv(Q, (int64_t)256);
  c.sblocks = (unsigned)std::min<int64_t>(sg, 1024);
  c.cr.blocks = (unsigned)std::min<int64_t>(cdiv(cg, (int64_t)4), 512);
  c.blocks = (c.sblocks + c.cr.blocks + 7u) & ~7u;
  c.last = 1u;
}

// the register-operand form (k_gemm_direct) for `g`: chunk slots per lane quarter and the 64 x 64 tiles of the estimated
// live rows, or false.  One place for gemm_launch and for callers that must know the form before they launch.
static bool direct_form(const GemmArgs& g, int* nsl_out, int64_t* tiles64_out) {
  static const int dir_knob = env_int("TG_GEMM_DIRECT", 1);  // tuning knob: 0 = off
  static const int64_t dir_tiles = env_int("TG_GEMM_DIRECT_TILES", 512);  // tuning knob
  const int nsl = (int)cdiv(cdiv(g.k, 4), 4);  // chunk slots per lane quarter
  const int64_t rows_e = g.m_hint > 0 ? std::min(g.m_hint, g.m_cap) : g.m_cap;
  const bool plain_d = plain_epilogue(g) && !g.a1.p && !g.bias2 && (!g.c2 || !g.c_rows) && g.a0.w == g.k;
  const int64_t tiles64 = cdiv(rows_e, 64) * cdiv(g.n, 64);
  *nsl_out = nsl;
  *tiles64_out = tiles64;
  return dir_knob && plain_d && nsl <= 12 && tiles64 <= dir_tiles;
}
// a second product rides only where both are register-operand products of the same instance (NS <= 11: the instance that
// hosts riders) and no earlier branch of gemm_launch claims the first: not the K-split family (K >= 320 at the least),
// not the many-row forms (>= 4 096 blocks of 128 rows)
bool gemm_hosts_second(const GemmArgs& g, const GemmArgs& s) {
  int nsl = 0, nsl2 = 0;
  int64_t t1 = 0, t2 = 0;
  if (g.m_cap <= 0 || s.m_cap <= 0 || g.k >= 320 || s.k >= 320 || (g.k % 4) || (s.k % 4) || (g.ldw % 4) || (s.ldw % 4)) return false;
  if (cdiv(g.m_cap, 128) * cdiv(g.n, 64) >= 4096 || s.c_rows) return false;
  // (the K-split family is asked itself: its least K is a knob, and without a rider gemm_launch offers it the first product)
  if (gemm_ks16_launch(g, nullptr, nullptr, nullptr, true)) return false;
  if (!direct_form(g, &nsl, &t1) || !direct_form(s, &nsl2, &t2)) return false;
  // (at most 256 tiles in the second product: the size at which a launch of its own takes the 2 x 2 wave tiles it gets here)
  return nsl <= 11 && nsl2 <= 11 && (nsl <= 7) == (nsl2 <= 7) && t2 <= 256;
}
// one grid for `gd` (256 persistent blocks), `second` (blocks for its 64 x 64 tiles, a multiple of 8) and the rider's r.blocks
template <class R>
static void direct2_launch(const GemmArgs& gd, const GemmArgs& second, const R& r, int nsl, bool wide, hipStream_t st) {
  GemmArgs gd2 = second;
  gd2.dbg = 0;
  const int64_t rows2 = gd2.m_hint > 0 ? std::min(gd2.m_hint, gd2.m_cap) : gd2.m_cap;
  const unsigned own2 = (unsigned)std::min<int64_t>(256, 8 * cdiv(cdiv(rows2, 64) * cdiv(gd2.n, 64), 8));
  const dim3 gr(256 + own2 + r.blocks);
  if (nsl <= 7) {
    TG_FORM(r.blocks ? (wide ? "direct<7,2x3>+direct<2x2>+rider" : "direct<7,2x2>+direct<2x2>+rider")
                     : (wide ? "direct<7,2x3>+direct<2x2>" : "direct<7,2x2>+direct<2x2>"));
    if (wide) TG_KLAUNCH((k_gemm_direct_r2<R, 7, 2, 3>), gr, dim3(256), 0, st, gd, gd2, own2, r);
    else TG_KLAUNCH((k_gemm_direct_r2<R, 7, 2, 2>), gr, dim3(256), 0, st, gd, gd2, own2, r);
  } else {
    TG_FORM(r.blocks ? (wide ? "direct<11,2x3>+direct<2x2>+rider" : "direct<11,2x2>+direct<2x2>+rider")
                     : (wide ? "direct<11,2x3>+direct<2x2>" : "direct<11,2x2>+direct<2x2>"));
    if (wide) TG_KLAUNCH((k_gemm_direct_r2<R, 11, 2, 3>), gr, dim3(256), 0, st, gd, gd2, own2, r);
    else TG_KLAUNCH((k_gemm_direct_r2<R, 11, 2, 2>), gr, dim3(256), 0, st, gd, gd2, own2, r);
  }
}

int gemm_launch(const GemmArgs& g, hipStream_t st, const WbRider* rider, bool* rode, const CollateRider* collate,
                const GemmArgs* second, bool* second_done) {
  if (rode) *rode = false;
  if (second_done) *second_done = false;
  if (second && (!second_done || rider)) return TG_EINVAL;
  if ((rider || collate) && (!rode || (rider && collate))) return TG_EINVAL;
  if (g.c2 && (g.bias_rs || g.bias2 || g.row_valid || g.relu_mask || g.c_rows || g.accumulate || !g.c2_rows || g.nbatch != 1))
    return TG_EINVAL;  // the second destination exists in the plain epilogue only
  if (g.m_cap <= 0) return TG_OK;
  if (g.n <= 0 || g.k <= 0 || (g.k % 4) || (g.a0.w % 4) || (g.ldw % 4) || g.nbatch <= 0) return TG_EINVAL;
  if (g.w_kmajor && (g.n % 4)) return TG_EINVAL;
  static const int log_knob = env_int("TG_GEMM_LOG", 0);  // diagnostic: one line per product
  if (log_knob)
    fprintf(stderr, "gemm m_cap=%lld m_dev=%d hint=%lld n=%d k=%d nbatch=%d kmajor=%d a1=%d idx=%d relu=%d mask=%d acc=%d c_rows=%d bias2=%d brs=%d\n",
            (long long)g.m_cap, g.m_dev != nullptr, (long long)g.m_hint, g.n, g.k, g.nbatch, g.w_kmajor, g.a1.p != nullptr,
            g.a0.idx != nullptr, g.relu, g.relu_mask != nullptr, g.accumulate, g.c_rows != nullptr, g.bias2 != nullptr, g.bias_rs != nullptr);
  if (g.a0.w + (g.a1.p ? g.a1.w : 0) != g.k) return TG_EINVAL;
  // long K, few tiles: LDS-free K-split blocks (k_gemm_ks16)
  if (!rider && !collate && !g.bias2 && gemm_ks16_launch(g, st)) return check_launch("gemm(ks16)");
  constexpr int BM = 64, BN = 64;
  const int64_t MT = cdiv(g.m_cap, BM);
  const int NT = (int)cdiv(g.n, BN);
  const int64_t grid = 8 * cdiv(MT, 8) * NT * g.nbatch;
  static const int ks_knob = env_int("TG_GEMM_KS", 0);  // tuning knob: 1 / 2, 0 = auto
  // measured at C2: a second k-group helps only launches that leave CUs idle AND have a long K (the merged
  // value/out/fc1 product: 144 tiles x 38 k-steps, 37 -> 35 us); elsewhere it is neutral or slightly worse
  const bool split = ks_knob ? ks_knob == 2 : (grid <= 256 && g.k >= 512);
  static const int gdbg = env_int("TG_GEMM_DBG", 0);
  GemmArgs gd = g;
  gd.dbg = phase_selected(g) ? gdbg : (gdbg & ~16);
  static const int depth_knob = env_int("TG_GEMM_DEPTH", 2);  // tuning knob: 2 / 4
  // a write-back rider that is not hosted: the caller runs the whole write-back itself, STEP 6's rows included - this
  // launch then stores no second copy of them
  auto no_ride = [&]() { if (rider) gd.c2 = nullptr; };
  // plain row-major products with MANY rows: register-blocked 128 x 64 blocks (three quarters of the staged bytes per
  // MFMA, half the fragment reads).  Measured: C5 shape (24 576 / 6 144 / 6 144 blocks) G 1.00 -> 0.96 ms, fc1 1.19 ->
  // 1.08 ms, fc2 0.261 -> 0.253 ms; at C3 / C4 sizes (288 .. 2 500 blocks) 3 .. 17 % SLOWER than the 64 x 64 blocks (whose
  // several co-resident blocks per CU cover each other's prologue and epilogue); 128 x 128 blocks are slower still there
  static const int rb_knob = env_int("TG_GEMM_RB", 1);  // tuning knob: 0 = off, 2 = 128 x 128
  // short K (4 / 6 / 8 k-tiles), plain epilogue, MANY rows: panel-stationary blocks of eight wavefronts (k_gemm_astat8)
  // (measured, 81 000 x 256 -> 1 024: 434 us as register-blocked blocks, 396 / 375 / 434 us with 4 / 8 / 16 column tiles per
  // panel block; 196 608 x 256 -> 256: 267 us with 4 against 260-280)
  static const int as8_knob = env_int("TG_GEMM_ASTAT8", 8);  // tuning knob: column tiles per block, 0 = off
  {
    const int nkt8 = (int)cdiv(g.k, BK);
    const bool plain8 = plain_epilogue(g) && !g.a1.p && !g.bias2 && !g.c2 && g.a0.w == g.k;
    // short K, plain epilogue, MANY rows: weight-stationary LDS-free blocks (k_gemm_wstat; TG_GEMM_WSTAT=0: off)
    static const int ws_knob = env_int("TG_GEMM_WSTAT", 1);  // tuning knob
    // Measured (1x MI355X): 196 608 x 256 -> 256 (fc2 at C5 shape) 265 -> 245 us (105 TF/s); 81 920 x 256 -> 1 024 383 us against
    // 378 us for the panel-stationary blocks below, 140 001 x 172 -> 1 032 536 against 568 us.  Ablation: without the chunk
    // reloads (MFMA stream + epilogue alone) 328 us = 0.83 of the matrix peak - the reloads cost the rest although they
    // are requested half a tile ahead.  Taken for N <= 256 (TG_GEMM_WSTAT=2: every N).
    if (ws_knob && plain8 && g.k <= 256 && g.k >= 64 && (g.n <= 256 || ws_knob == 2) && cdiv(g.m_cap, 128) * NT >= 4096) {
      no_ride();
      const int NG = (int)cdiv(g.n, 128);
      const unsigned lanes8 = (unsigned)std::max<int64_t>(1, std::min<int64_t>(512 / 8 / NG, cdiv(cdiv(g.m_cap, 16), 8)));
      const dim3 gr(8u * (unsigned)NG * lanes8);
      const int nsl = (int)cdiv(cdiv(g.k, 4), 4);
#define TG_WSTAT(NS_)                                                                                   \
  do {                                                                                                  \
    TG_FORM(g.c_rows && g.a0.idx ? "wstat<" #NS_ ",crows,idx>" : g.c_rows ? "wstat<" #NS_ ",crows>"     \
            : g.a0.idx ? "wstat<" #NS_ ",idx>" : "wstat<" #NS_ ">");                                    \
    if (g.c_rows && g.a0.idx) TG_KLAUNCH((k_gemm_wstat<NS_, true, true>), gr, dim3(256), 0, st, gd);    \
    else if (g.c_rows) TG_KLAUNCH((k_gemm_wstat<NS_, true, false>), gr, dim3(256), 0, st, gd);          \
    else if (g.a0.idx) TG_KLAUNCH((k_gemm_wstat<NS_, false, true>), gr, dim3(256), 0, st, gd);          \
    else TG_KLAUNCH((k_gemm_wstat<NS_, false, false>), gr, dim3(256), 0, st, gd);                       \
  } while (0)
      if (nsl <= 8) TG_WSTAT(8);
      else if (nsl <= 11) TG_WSTAT(11);
      else TG_WSTAT(16);
#undef TG_WSTAT
      return check_launch("gemm(wstat)");
    }
    if (as8_knob && plain8 && (nkt8 == 4 || nkt8 == 6 || nkt8 == 8) && cdiv(g.m_cap, 128) * NT >= 4096) {
      no_ride();
      const int cpb = std::min(as8_knob, NT);
      const dim3 gr((unsigned)(8 * cdiv(cdiv(g.m_cap, 128), 8) * cdiv(NT, cpb)));
      TG_FORM(nkt8 == 4 ? "astat8<4>" : nkt8 == 6 ? "astat8<6>" : "astat8<8>");
      if (nkt8 == 4) TG_KLAUNCH((k_gemm_astat8<4>), gr, dim3(512), 0, st, gd, cpb);
      else if (nkt8 == 6) TG_KLAUNCH((k_gemm_astat8<6>), gr, dim3(512), 0, st, gd, cpb);
      else TG_KLAUNCH((k_gemm_astat8<8>), gr, dim3(512), 0, st, gd, cpb);
      return check_launch("gemm(astat8)");
    }
  }
  if (rb_knob && plain_epilogue(g) && cdiv(g.m_cap, 128) * NT >= 4096) {
    no_ride();
    // (128 x 128 blocks - four 32 x 32 accumulators per wavefront, twice the MFMAs between barriers - where N is a multiple
    // of 128 and K long: 196 608 x 1 280 -> 256 1 072 -> 1 041 us; K = 256: no difference)
    if ((rb_knob == 2 && g.n >= 512) || (rb_knob == 1 && g.n % 128 == 0 && g.k >= 512) || (rb_knob == 3 && g.n >= 128)) {
      TG_FORM("rb<2,2>");
      TG_KLAUNCH((k_gemm_rb<2, 2>), dim3((unsigned)(8 * cdiv(cdiv(g.m_cap, 128), 8) * cdiv(g.n, 128))), dim3(256), 0, st, gd);
    } else {
      TG_FORM("rb<2,1>");
      TG_KLAUNCH((k_gemm_rb<2, 1>), dim3((unsigned)(8 * cdiv(cdiv(g.m_cap, 128), 8) * NT)), dim3(256), 0, st, gd);
    }
    return check_launch("gemm(rb)");
  }
  // short K and few (live) rows: whole operands in registers (see gemm_direct_tile).  Wave tiles of 32 x 32, or 32 x 48
  // when that brings the blocks of the estimated live rows under the CU count
  {
    int nsl = 0;
    int64_t tiles64 = 0;
    if (direct_form(g, &nsl, &tiles64)) {
      const bool wide = tiles64 > 256 && nsl <= 11;  // (32 x 48 wave tiles: 5 x 44 operand registers)
      const unsigned own = 256;
      const bool ride = nsl <= 11;  // (the K <= 192 instance hosts no riders)
      CollateRider co = (collate && ride) ? *collate : CollateRider{};
      WbRider wr = (rider && ride) ? *rider : WbRider{};
      if (collate && ride) collate_blocks(co);
      if (rider && ride) {
        wr.blocks = rider_blocks(std::min<int64_t>(tiles64, 256), 256, 2 * wr.a.B);
        wr.last = 1u;
      } else {
        no_ride();
      }
      // a second product (see k_gemm_direct_r2) beside it, riders behind both
      if (second && gemm_hosts_second(g, *second)) {
        *second_done = true;
        if (co.blocks) direct2_launch(gd, *second, co, nsl, wide, st);
        else direct2_launch(gd, *second, NoRider{0u}, nsl, wide, st);
        if (collate && ride) *rode = true;
        return check_launch("gemm(direct + direct)");
      }
      const dim3 gr(own + co.blocks + wr.blocks);
#define TG_DIRECT(NS_)                                                                                                  \
  do {                                                                                                                  \
    TG_FORM(wr.blocks ? (wide ? "direct<" #NS_ ",2x3>+wb" : "direct<" #NS_ ",2x2>+wb")                                  \
            : co.blocks ? (wide ? "direct<" #NS_ ",2x3>+collate" : "direct<" #NS_ ",2x2>+collate")                      \
            : (wide ? "direct<" #NS_ ",2x3>" : "direct<" #NS_ ",2x2>"));                                                \
    if (wr.blocks && wide) TG_KLAUNCH((k_gemm_direct_r<WbRider, NS_, 2, 3>), gr, dim3(256), 0, st, gd, wr);      \
    else if (wr.blocks) TG_KLAUNCH((k_gemm_direct_r<WbRider, NS_, 2, 2>), gr, dim3(256), 0, st, gd, wr);        \
    else if (co.blocks && wide) TG_KLAUNCH((k_gemm_direct_r<CollateRider, NS_, 2, 3>), gr, dim3(256), 0, st, gd, co); \
    else if (co.blocks) TG_KLAUNCH((k_gemm_direct_r<CollateRider, NS_, 2, 2>), gr, dim3(256), 0, st, gd, co);   \
    else if (wide) TG_KLAUNCH((k_gemm_direct<NS_, 2, 3>), gr, dim3(256), 0, st, gd);                            \
    else TG_KLAUNCH((k_gemm_direct<NS_, 2, 2>), gr, dim3(256), 0, st, gd);                                      \
  } while (0)
      if (nsl <= 7) TG_DIRECT(7);
      else if (nsl <= 11) TG_DIRECT(11);
      else {
        TG_FORM("direct<12,2x2>");
        TG_KLAUNCH((k_gemm_direct<12, 2, 2>), dim3(own), dim3(256), 0, st, gd);
      }
#undef TG_DIRECT
      if ((collate || rider) && ride) *rode = true;
      return check_launch("gemm(direct)");
    }
  }
  // short K, many column tiles, a launch of a few blocks per CU: activation-stationary blocks (see k_gemm_astat)
  static const int as_knob = env_int("TG_GEMM_ASTAT", 1);  // tuning knob: 0 = off, n = column tiles per block
  {
    const int nkt = (int)cdiv(g.k, BK);
    const bool plain_as = plain_epilogue(g) && !g.a1.p && !g.bias2 && g.a0.w == g.k;
    if (as_knob && plain_as && NT >= 8 && (nkt == 4 || nkt == 6 || nkt == 8) && MT * NT <= 1024) {  // (C3's 3 264 tiles: no gain)
      // two column tiles per block (measured at C2, 48 x 17 tiles: 21.6 us; three: 28.1, four: 24.6, six: 29.8, nine:
      // 40.8; separate 64 x 64 blocks: 24.4): two such blocks share a CU and cover each other's barriers, which matters
      // more than the shared panel
      static const int cpb_knob = env_int("TG_GEMM_ASTAT_CPB", 0);
      const int cpb = cpb_knob > 0 ? std::min(cpb_knob, NT) : as_knob > 1 ? std::min(as_knob, NT) : 2;
      const int64_t gb = 8 * cdiv(MT, 8) * cdiv(NT, cpb);
      if (collate && live_blocks(g, gb, 64) <= RIDER_MAX_LIVE) {
        CollateRider co = *collate;
        collate_blocks(co);
        const dim3 grid_r((unsigned)(gb + co.blocks));
        TG_FORM(nkt == 4 ? "astat<4>+collate" : nkt == 6 ? "astat<6>+collate" : "astat<8>+collate");
        if (nkt == 4) TG_KLAUNCH((k_gemm_astat_r<CollateRider, 4>), grid_r, dim3(256), 0, st, gd, cpb, co);
        else if (nkt == 6) TG_KLAUNCH((k_gemm_astat_r<CollateRider, 6>), grid_r, dim3(256), 0, st, gd, cpb, co);
        else TG_KLAUNCH((k_gemm_astat_r<CollateRider, 8>), grid_r, dim3(256), 0, st, gd, cpb, co);
        *rode = true;
        return check_launch("gemm(astat+collate)");
      }
      no_ride();
      const dim3 grid_as((unsigned)gb);
      TG_FORM(nkt == 4 ? "astat<4>" : nkt == 6 ? "astat<6>" : "astat<8>");
      if (nkt == 4) TG_KLAUNCH((k_gemm_astat<4>), grid_as, dim3(256), 0, st, gd, cpb);
      else if (nkt == 6) TG_KLAUNCH((k_gemm_astat<6>), grid_as, dim3(256), 0, st, gd, cpb);
      else TG_KLAUNCH((k_gemm_astat<8>), grid_as, dim3(256), 0, st, gd, cpb);
      return check_launch("gemm(astat)");
    }
  }
  if (g.ask_part) {  // A assembled from stream-K pieces of a 64-row-tiled producer with g.k output columns
    if (g.nbatch != 1 || g.w_kmajor || g.k != g.a0.w || !g.ask_bias || g.ask_NT != (int)cdiv(g.k, 64)) return TG_EINVAL;
    static const int ask_depth = env_int("TG_GEMM_ASK_DEPTH", 2);  // tuning knob: 2 / 4
    gd.ask_rcpU = 1.0f / (float)g.ask_U;
    static const int ask_ks = env_int("TG_GEMM_ASK_KS", 2);  // tuning knob: 1 / 2 (measured 12.6 / 11.1 us)
    WbRider wr = rider ? *rider : WbRider{};
    if (rider && (g.ask_pieces > 3 || ask_ks == 2)) {  // (stream-K consumers: the producer had fewer tiles than CUs)
      wr.blocks = rider_blocks(grid, 512, 2 * wr.a.B);
      wr.last = 1u;
      TG_FORM("gemm<ask,ks2>+wb");
      if (g.ask_pieces > 3)
        TG_KLAUNCH((k_gemm_r<WbRider, 2, 2, 2, 2, true, 8>), dim3((unsigned)grid + wr.blocks), dim3(512), 0, st, gd, wr);
      else
        TG_KLAUNCH((k_gemm_r<WbRider, 2, 2, 2, 2, true>), dim3((unsigned)grid + wr.blocks), dim3(512), 0, st, gd, wr);
      *rode = true;
    } else {
      no_ride();
      TG_FORM(g.ask_pieces > 3 || ask_ks == 2 ? "gemm<ask,ks2>" : ask_depth == 4 ? "gemm<ask,ks1,d4>" : "gemm<ask,ks1,d2>");
      if (g.ask_pieces > 3) TG_KLAUNCH((k_gemm<2, 2, 2, 2, true, 8>), dim3((unsigned)grid), dim3(512), 0, st, gd);
      else if (ask_ks == 2) TG_KLAUNCH((k_gemm<2, 2, 2, 2, true>), dim3((unsigned)grid), dim3(512), 0, st, gd);
      else if (ask_depth == 4) TG_KLAUNCH((k_gemm<2, 2, 1, 4, true>), dim3((unsigned)grid), dim3(256), 0, st, gd);
      else TG_KLAUNCH((k_gemm<2, 2, 1, 2, true>), dim3((unsigned)grid), dim3(256), 0, st, gd);
    }
  } else if (split) {
    no_ride();
    TG_FORM("gemm<ks2>");
    TG_KLAUNCH((k_gemm<2, 2, 2, 2>), dim3((unsigned)grid), dim3(512), 0, st, gd);
  } else if (depth_knob == 2 && rider && live_blocks(g, grid, 64) <= RIDER_MAX_LIVE) {
    WbRider wr = *rider;
    wr.blocks = rider_blocks(live_blocks(g, grid, 64), 256, 2 * wr.a.B);
    wr.last = 1u;
    TG_FORM("gemm<ks1,d2>+wb");
    TG_KLAUNCH((k_gemm_r<WbRider, 2, 2, 1, 2>), dim3((unsigned)grid + wr.blocks), dim3(256), 0, st, gd, wr);
    *rode = true;
  } else if (depth_knob == 2 && collate && live_blocks(g, grid, 64) <= RIDER_MAX_LIVE) {
    CollateRider co = *collate;
    collate_blocks(co);
    TG_FORM("gemm<ks1,d2>+collate");
    TG_KLAUNCH((k_gemm_r<CollateRider, 2, 2, 1, 2>), dim3((unsigned)grid + co.blocks), dim3(256), 0, st, gd, co);
    *rode = true;
  } else if (depth_knob == 2) {
    no_ride();
    TG_FORM("gemm<ks1,d2>");
    TG_KLAUNCH((k_gemm<2, 2, 1, 2>), dim3((unsigned)grid), dim3(256), 0, st, gd);
  } else {
    no_ride();
    TG_FORM("gemm<ks1,d4>");
    TG_KLAUNCH((k_gemm<2, 2, 1, 4>), dim3((unsigned)grid), dim3(256), 0, st, gd);
  }
  return check_launch("gemm");
}

}  // namespace tg

// diagnostic: one product straight through gemm_launch (no riders, no second destination, no stream-K operand), and
// which kernel it picked.  Every argument check runs before anything touches the GPU.
extern "C" int tg_debug_gemm(const tg_gemm_probe* p, const char** form_out, void* stream) {
  using namespace tg;
  if (form_out) *form_out = nullptr;
  if (!p || !p->a0 || !p->w || !p->c) return TG_EINVAL;
  if (p->k <= 0 || p->n <= 0 || (p->k % 4) || (p->a0_w % 4) || (p->ldw % 4) || p->nbatch < 1) return TG_EINVAL;
  if (p->a1 && (p->a1_w % 4)) return TG_EINVAL;
  if (p->bias2 && !p->bias2_valid) return TG_EINVAL;
  GemmArgs g{};
  g.m_cap = p->m_cap; g.m_dev = p->m_dev; g.m_hint = p->m_hint;
  g.n = p->n; g.k = p->k;
  g.a0 = ASeg{p->a0, p->a0_ld, p->a0_w, p->a0_idx};
  if (p->a1) g.a1 = ASeg{p->a1, p->a1_ld, p->a1_w, p->a1_idx};
  g.w = p->w; g.ldw = p->ldw; g.w_kmajor = p->w_kmajor;
  g.bias = p->bias; g.bias2 = p->bias2; g.bias2_valid = p->bias2_valid;
  g.bias_rs = p->bias_rs; g.ld_brs = p->ld_brs;
  g.row_valid = p->row_valid; g.relu_mask = p->relu_mask; g.ld_mask = p->ld_mask;
  g.c_rows = p->c_rows; g.accumulate = p->accumulate;
  g.alpha = p->alpha; g.relu = p->relu;
  g.c = p->c; g.ldc = p->ldc;
  g.nbatch = p->nbatch; g.a0_bs = p->a0_bs; g.w_bs = p->w_bs; g.bias_bs = p->bias_bs; g.c_bs = p->c_bs;
  t_gemm_form = nullptr;
  // gemm_launch never hands a product with a second bias to the K-split family; the fused attention's fc1 (tg_attn.hip), the
  // one caller with such a product, offers it to gemm_ks16_launch itself first - and so does the probe
  int rc;
  if (g.bias2 && g.m_cap > 0 && g.a0.w + (g.a1.p ? g.a1.w : 0) == g.k && gemm_ks16_launch(g, as_stream(stream)))
    rc = check_launch("gemm(ks16)");
  else
    rc = gemm_launch(g, as_stream(stream));
  if (form_out) *form_out = t_gemm_form;
  return rc;
}

extern "C" int tg_debug_gemm2(const tg_gemm_probe* p, const tg_gemm_probe* q, float* second_c2, int32_t* hosted,
                              uint32_t* rider_out, int64_t rider_n, int32_t rider_blocks, void* stream) {
  using namespace tg;
  if (hosted) *hosted = 0;
  if (!p || !q || !hosted || !p->a0 || !p->w || !p->c || !q->a0 || !q->w || !q->c) return TG_EINVAL;
  if (p->k <= 0 || p->n <= 0 || (p->k % 4) || (p->a0_w % 4) || (p->ldw % 4) || p->nbatch != 1 || p->a0_w != p->k) return TG_EINVAL;
  if (q->k <= 0 || q->n <= 0 || (q->k % 4) || (q->a0_w % 4) || (q->ldw % 4) || q->nbatch != 1 || q->a0_w != q->k) return TG_EINVAL;
  if (p->a1 || q->a1 || q->a0_idx || q->m_dev || (q->c_rows && !second_c2)) return TG_EINVAL;
  if (rider_blocks < 0 || rider_blocks > 1024 || (rider_blocks % 8) || (rider_blocks && (!rider_out || rider_n <= 0))) return TG_EINVAL;
  GemmArgs g{}, s{};
  g.m_cap = p->m_cap; g.m_dev = p->m_dev; g.m_hint = p->m_hint; g.n = p->n; g.k = p->k;
  g.a0 = ASeg{p->a0, p->a0_ld, p->a0_w, p->a0_idx};
  g.w = p->w; g.ldw = p->ldw; g.bias = p->bias; g.c_rows = p->c_rows; g.alpha = p->alpha; g.relu = p->relu;
  g.c = p->c; g.ldc = p->ldc; g.nbatch = 1;
  s.m_cap = q->m_cap; s.n = q->n; s.k = q->k; s.a0 = ASeg{q->a0, q->a0_ld, q->a0_w, nullptr};
  s.w = q->w; s.ldw = q->ldw; s.bias = q->bias; s.alpha = q->alpha; s.relu = q->relu; s.c = q->c; s.ldc = q->ldc; s.nbatch = 1;
  if (q->c_rows) { s.c2 = second_c2; s.c2_rows = q->c_rows; s.c2_m = q->m_cap; s.ldc2 = q->ldc; }
  if (rider_blocks) {  // the grid gemm_launch forms with a collate rider, with the stand-in in the rider's place
    int nsl = 0;
    int64_t tiles64 = 0;
    if (g.m_cap <= 0 || !gemm_hosts_second(g, s) || !direct_form(g, &nsl, &tiles64)) return TG_OK;
    direct2_launch(g, s, FillRider{(unsigned)rider_blocks, rider_out, rider_n}, nsl, tiles64 > 256 && nsl <= 11, as_stream(stream));
    *hosted = 1;
    return check_launch("tg_debug_gemm2");
  }
  bool done = false;
  const int rc = gemm_launch(g, as_stream(stream), nullptr, nullptr, nullptr, &s, &done);
  *hosted = done ? 1 : 0;
  return rc;
}
