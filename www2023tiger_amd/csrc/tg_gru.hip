// The fused GRU cell on the float32 MFMA: gates in the GEMM epilogue (a15).
// Reference: nn.GRUCell as used at tiger/model/update_modules.py:30-37.
// Holds the LDS-staged blocks (k_gru<NW, KS> with the 16-column tail gru_tail16), the LDS-free blocks (k_gru_direct,
// k_gru_direct16) and their dispatcher gru_launch.
#include <cstdlib>

#include "tg_mfma.h"

namespace tg {

// diagnostic (tg_debug_gru): family and instance of the last cell this thread launched - a string literal picked in
// the branch that launches (as TG_FORM in tg_gemm.hip; nothing is formatted on the launch path)
static thread_local const char* t_gru_form = nullptr;
#define TG_GRU_FORM(lit_) (t_gru_form = (lit_))

// ---------------------------------------------------------------------------------
// GRU cell, gates fused into the GEMM epilogue.  A block owns 128 rows x 32 hidden
// columns and accumulates four planes per column: r and z over K = [x | h], i_n over x
// only, h_n over h only (no wasted MFMAs on the zero blocks of a packed [4d, 5d] weight).
// ---------------------------------------------------------------------------------
// The last hidden columns of the GRU when d is not a multiple of 32: a 16-column tile on
// v_mfma_f32_16x16x4_f32 instead of a 32-column tile that is mostly padding (d = 172: 12 columns of 32).
// One block owns 144 rows x 16 columns x 3 planes - three quarters of the MFMA work of a 96 x 32 block of
// k_gru<3, 4>, whose launch it shares, but the same 24 KB of operands staged per tile, which is what sets the
// pace (12 wavefronts: 3 row groups of 48 rows x 4 k-groups).
// Lane l feeds A[i = l % 16][k = l / 16] and B[k = l / 16][j = l % 16] and receives D[4 (l / 16) + r][l % 16].
// Tiles are [row][k] with a 34-float stride: (34 r + k) mod 32 is injective over the 16 rows x 2 k of a
// 32-lane read group.  Plain pipeline (next tile in registers while this one is multiplied).
constexpr int T16_RT = 3;                       // 16-row MFMA tiles per row group
constexpr int T16_RG = 16 * T16_RT;             // rows per row group (three groups)
constexpr int T16_ROWS = 3 * T16_RG, T16_LD = 34;
constexpr int T16_A = 2 * T16_ROWS * T16_LD, T16_B = 2 * 48 * T16_LD;  // floats
__device__ __forceinline__ void gru_tail16(const GruArgs& g, int tb, int j0, float* __restrict__ arena,
                                           float* __restrict__ hs, int* __restrict__ orow_s) {
  constexpr int THREADS = 768;
  float (*As)[T16_ROWS][T16_LD] = reinterpret_cast<float (*)[T16_ROWS][T16_LD]>(arena);
  float (*Bs)[48][T16_LD] = reinterpret_cast<float (*)[48][T16_LD]>(arena + T16_A);
  float (*red)[4][3][16][64] = reinterpret_cast<float (*)[4][3][16][64]>(arena);
  float (*Hs)[17] = reinterpret_cast<float (*)[17]>(hs);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rg = wave % 3, ks = wave / 3;
  const int d = g.d, xw = g.xw;
  int64_t M = g.cap;
  if (g.n_dev) M = min(M, (int64_t)*g.n_dev);
  const int64_t m0 = (int64_t)tb * T16_ROWS;
  if (m0 >= M) return;
  if (tid < T16_ROWS) {
    const int64_t m = min(m0 + tid, M - 1);
    orow_s[tid] = g.out_rows ? g.out_rows[m] : (int)m;
  }
  const int li = lane & 15, lk = lane >> 4;
  const int jb = min(j0 + li, d - 1);
  const float br = g.b_ih[jb] + g.b_hh[jb];
  const float bz = g.b_ih[d + jb] + g.b_hh[d + jb];
  const float bin = g.b_ih[2 * d + jb], bhn = g.b_hh[2 * d + jb];
  // staging: two activation float4 per thread (rows ar, ar + 96), one weight float4 for the first 384 threads
  const int ar = tid >> 3, ac4 = (tid & 7) * 4;
  const float* xrow[2];
  const float* hrow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t m = min(m0 + min(ar + 96 * i, T16_ROWS - 1), M - 1);
    xrow[i] = g.x.p + (g.x.idx ? g.x.idx[m] : m) * g.x.ld;
    hrow[i] = g.h.p + (g.h.idx ? g.h.idx[m] : m) * g.h.ld;
  }
  const int wl = min(ar, 47);  // weight-tile row: plane wl / 16, column wl % 16
  const int wj = min(j0 + (wl & 15), d - 1);
  const float* wx = g.w_ih + ((int64_t)(wl >> 4) * d + wj) * xw;
  const float* wh = g.w_hh + ((int64_t)(wl >> 4) * d + wj) * d;
  const int nkx = (xw + BK - 1) / BK - g.x_skip_n, nkh = (d + BK - 1) / BK;  // message tiles that are processed
  const int nkt = nkx + nkh;
  // processed message tile t holds k-tile t, or t + x_skip_n past the skipped run: a column shift on the ADDRESSES of
  // those tiles (xs_sh), the k arithmetic itself runs on the compacted width xwe
  const int xs_at = g.x_skip_at, xs_sh = g.x_skip_n * BK, xwe = xw - xs_sh;
  struct Stage {
    float4 a0, a1, b;
  };
  auto load_tile = [&](int t, Stage& r) {  // raw loads from clamped addresses (tiles past the end: the last one again)
    t = min(t, nkt - 1);
    const bool hp = t >= nkx;
    const int k = (hp ? t - nkx : t) * BK + ac4;
    const int kc = (k < (hp ? d : xwe) ? k : 0) + ((!hp && t >= xs_at) ? xs_sh : 0);
    r.a0 = ldg4((hp ? hrow[0] : xrow[0]) + kc);
    r.a1 = ldg4((hp ? hrow[1] : xrow[1]) + kc);
    r.b = ldg4((hp ? wh : wx) + kc);
  };
  auto store_tile = [&](int buf, int t, const Stage& r) {
    const bool hp = t >= nkx;
    const bool kin = (hp ? t - nkx : t) * BK + ac4 < (hp ? d : xwe);
    sts4(As[buf][ar], ac4, kin ? r.a0 : zero4());
    if (ar + 96 < T16_ROWS) sts4(As[buf][ar + 96], ac4, kin ? r.a1 : zero4());
    if (ar < 48) sts4(Bs[buf][ar], ac4, kin ? r.b : zero4());
  };
  f32x4m acc_r[T16_RT], acc_z[T16_RT], acc_in[T16_RT], acc_hn[T16_RT];
#pragma unroll
  for (int i = 0; i < T16_RT; ++i) acc_r[i] = acc_z[i] = acc_in[i] = acc_hn[i] = f32x4m{0.f, 0.f, 0.f, 0.f};
  const int ht = nkx + (j0 >> 5), hc = j0 & 31;  // the memory tile / column offset that holds h[., j0 .. j0 + 16)
  // tile t in LDS[buf]: tile t + 2 is requested into `ld`, the k-steps run, tile t + 1 (`stv`, requested a tile
  // ago) moves to LDS[buf ^ 1]; straight-line body, all loads unconditional
  auto step = [&](auto hp_tag, int buf, int t, Stage& ld, const Stage& stv) {
    constexpr bool HP = decltype(hp_tag)::value;
    load_tile(t + 2, ld);
    float a[2][T16_RT], b[2][3];
    auto read = [&](int st, float* av, float* bv) {  // this k-group's k-step st: columns ks * 8 + 4 st + lk
      const int k = ks * 8 + st * 4 + lk;
#pragma unroll
      for (int rt = 0; rt < T16_RT; ++rt) av[rt] = As[buf][rg * T16_RG + rt * 16 + li][k];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) bv[pl] = Bs[buf][pl * 16 + li][k];
    };
    read(0, a[0], b[0]);
#pragma unroll
    for (int st = 0; st < 2; ++st) {
#pragma unroll
      for (int rt = 0; rt < T16_RT; ++rt) {
        acc_r[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st][rt], b[st][0], acc_r[rt], 0, 0, 0);
        if (st == 0 && rt == 0) read(1, a[1], b[1]);
        acc_z[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st][rt], b[st][1], acc_z[rt], 0, 0, 0);
        if (HP) acc_hn[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st][rt], b[st][2], acc_hn[rt], 0, 0, 0);
        else acc_in[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[st][rt], b[st][2], acc_in[rt], 0, 0, 0);
      }
    }
    if (HP && t == ht) {
      for (int f = tid; f < T16_ROWS * 16; f += THREADS) Hs[f >> 4][f & 15] = As[buf][f >> 4][hc + (f & 15)];
    }
    store_tile(buf ^ 1, t + 1, stv);
    __syncthreads();
  };
  using HP0 = std::integral_constant<bool, false>;
  using HP1 = std::integral_constant<bool, true>;
  Stage sa, sb;
  load_tile(0, sa);
  load_tile(1, sb);
  store_tile(0, 0, sa);
  __syncthreads();
  int t = 0;
  for (; t + 2 <= nkx; t += 2) {
    step(HP0{}, 0, t, sa, sb);
    step(HP0{}, 1, t + 1, sb, sa);
  }
  if (t < nkx) {  // odd number of message tiles: the memory tiles start in LDS[1]
    step(HP0{}, 0, t, sa, sb);
    for (++t; t + 2 <= nkt; t += 2) {
      step(HP1{}, 1, t, sb, sa);
      step(HP1{}, 0, t + 1, sa, sb);
    }
    if (t < nkt) step(HP1{}, 1, t, sb, sa);
  } else {
    for (; t + 2 <= nkt; t += 2) {
      step(HP1{}, 0, t, sa, sb);
      step(HP1{}, 1, t + 1, sb, sa);
    }
    if (t < nkt) step(HP1{}, 0, t, sa, sb);
  }
  // fold the four k-groups (as in k_gru): groups [half, 2 half) write, groups [0, half) add
#pragma unroll
  for (int half = 2; half >= 1; half /= 2) {
    if (ks >= half && ks < 2 * half) {
#pragma unroll
      for (int rt = 0; rt < T16_RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          red[ks - half][0][rg][rt * 4 + r][lane] = acc_r[rt][r];
          red[ks - half][1][rg][rt * 4 + r][lane] = acc_z[rt][r];
          red[ks - half][2][rg][rt * 4 + r][lane] = acc_in[rt][r];
          red[ks - half][3][rg][rt * 4 + r][lane] = acc_hn[rt][r];
        }
    }
    __syncthreads();
    if (ks < half) {
#pragma unroll
      for (int rt = 0; rt < T16_RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          acc_r[rt][r] += red[ks][0][rg][rt * 4 + r][lane];
          acc_z[rt][r] += red[ks][1][rg][rt * 4 + r][lane];
          acc_in[rt][r] += red[ks][2][rg][rt * 4 + r][lane];
          acc_hn[rt][r] += red[ks][3][rg][rt * 4 + r][lane];
        }
    }
    if (half > 1) __syncthreads();
  }
  if (ks != 0) return;
  const int j = j0 + li;
  if (j >= d) return;
#pragma unroll
  for (int rt = 0; rt < T16_RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lr = rg * T16_RG + rt * 16 + 4 * lk + r;
      const int64_t m = m0 + lr;
      if (m >= M) continue;
      const float rgate = fast_sigmoid(acc_r[rt][r] + br);
      const float zgate = fast_sigmoid(acc_z[rt][r] + bz);
      const float hn = acc_hn[rt][r] + bhn;
      const float ng = fast_tanh(acc_in[rt][r] + bin + rgate * hn);
      const float hv = (1.f - zgate) * ng + zgate * Hs[lr][li];
      g.out[(int64_t)orow_s[lr] * g.ldo + j] = hv;
      if (g.out2) g.out2[(g.out2_by_row ? (int64_t)orow_s[lr] : m) * (int64_t)d + j] = g.add2 ? hv + g.add2[(int64_t)orow_s[lr] * d + j] : hv;
      if (g.gates) {
        float* gp = g.gates + m * 4 * (int64_t)d + j;
        gp[0] = rgate; gp[d] = zgate; gp[2 * d] = ng; gp[3 * d] = hn;
      }
    }
}

// diagnostic only (TG_GRU_DBG & 16): per-block s_memtime stamps {entry, loop start, loop end, exit}
__device__ unsigned long long g_gru_trace[2048 * 4];

template <int NW, int KS>
__global__ void __launch_bounds__(64 * NW * KS, (NW == 4 && KS == 1) ? 2 : 1) k_gru(GruArgs g) {
  // NW wavefronts stack 32-row MFMA tiles (BM = 32 NW rows per block); with KS = 2 a second
  // group of NW wavefronts takes the other half of every tile's k-steps into its own
  // accumulators (summed through LDS at the end), which puts two independent instruction
  // streams on every SIMD: a single wave drives the f32 matrix pipe to only ~65 % here.
  constexpr int THREADS = 64 * NW * KS;
  constexpr int BM = 32 * NW;
  constexpr int RP = THREADS / 8;              // tile rows staged per pass (8 threads per 32-float row)
  constexpr int NA = BM / RP;                  // activation float4 per thread per tile
  constexpr int NBL = (96 + RP - 1) / RP;      // weight float4 per thread per tile (3 planes x 32 rows)
  constexpr int NOPS = NA + NBL;
  constexpr int PP = 8 / KS;                   // k-step pairs per wave per tile
  constexpr int SL = (NOPS + PP / 2 - 1) / (PP / 2);  // memory-op slots per k-step pair: 3 in the wide blocks, 4 in the 32-row one
  static_assert(BM % RP == 0 && SL <= 4, "at most four memory-op slots between the six MFMAs of a k-step pair");
  const unsigned long long t_entry = (g.dbg & 16) ? __builtin_amdgcn_s_memtime() : 0ull;
  // One LDS arena: the operand tiles while the loop runs, the k-group fold afterwards (the tiles are dead then).
  constexpr int A_FLOATS = 2 * BM * LDK, B_FLOATS = 2 * 3 * 32 * LDK;
  // k-group fold: either halving rounds (the upper half of the live groups writes at once), or - where the LDS allows -
  // one reduce-scatter round after which EVERY k-group finishes the rows it owns (see the epilogue)
  constexpr bool SCAT = KS > 1 && NW != 3;
  constexpr int OWN = 16 / KS;  // accumulator registers (row quads) a k-group owns in the scattered epilogue
  constexpr int RED_FLOATS = KS == 1 ? 0 : SCAT ? NW * KS * (KS - 1) * 4 * OWN * 64 : (KS / 2) * 4 * NW * 16 * 64;
  constexpr int ARENA0 = (A_FLOATS + B_FLOATS) > RED_FLOATS ? (A_FLOATS + B_FLOATS) : RED_FLOATS;
  constexpr bool TAIL = NW == 3 && KS == 4;  // this instance also serves the 16-column tail blocks (gru_tail16)
  constexpr int ARENA = TAIL && (T16_A + T16_B) > ARENA0 ? (T16_A + T16_B) : ARENA0;
  __shared__ float arena[ARENA];
  float (*As)[BM][LDK] = reinterpret_cast<float (*)[BM][LDK]>(arena);
  float (*Bs)[3][32][LDK] = reinterpret_cast<float (*)[3][32][LDK]>(arena + A_FLOATS);
  float (*red)[4][NW][16][64] = reinterpret_cast<float (*)[4][NW][16][64]>(arena);  // [k-group slot][plane][row wave]
  // epilogue operands staged while the loop runs (no global load is left for the epilogue, where its
  // latency would be exposed): the old-memory tile h[m, j0..j0+32) is one of the A tiles the loop
  // streams anyway, the output rows are fetched at block start
  // (128-row blocks: a lane captures the old-memory values of ITS accumulator rows in registers when that tile passes -
  // 17 KB of LDS less, which is what lets two k_gru<4, 1> blocks share a CU)
  constexpr bool HREG = NW == 4;
  constexpr int NHOLD = KS == 1 ? 16 : OWN;
  constexpr int HS_FLOATS = HREG ? 4 : TAIL && T16_ROWS * 17 > BM * LDK ? T16_ROWS * 17 : BM * LDK;
  __shared__ float hs_raw[HS_FLOATS];
  float hold_r[HREG ? NHOLD : 1];
  __shared__ int orow_s[TAIL ? T16_ROWS : BM];
  float (*Hs)[LDK] = reinterpret_cast<float (*)[LDK]>(hs_raw);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rw = wave % NW, ks = wave / NW;
  const int d = g.d, xw = g.xw;
  // column tiles of 32 handled here; with a tail (tail_blocks > 0) the last, partial one belongs to gru_tail16,
  // whose blocks come FIRST in the grid so that they start with everybody else
  const int NT = (d + 31) / 32 - (g.tail_blocks > 0 ? 1 : 0);
  int64_t M = g.cap;
  if (g.n_dev) M = min(M, (int64_t)*g.n_dev);
  const int xcd = blockIdx.x & 7;
  int s = blockIdx.x >> 3;
  if (TAIL && g.tail_blocks > 0) {
    // With the tail the launch is sized to fit the chip in ONE round (every CU at most one block), so the live
    // blocks must also be dealt evenly over the eight XCDs (blockIdx % 8): XCD x works through the row tiles
    // mt = x (mod 8), all their column tiles, then its share of the tail blocks - the XCDs that own one row
    // tile less take NT tail blocks each first, the rest is dealt round robin.  All from the live row count.
    const int MT = (int)((M + BM - 1) / BM), TT = (int)((M + T16_ROWS - 1) / T16_ROWS);
    const int r = MT & 7, n_main = (MT / 8 + (xcd < r ? 1 : 0)) * NT;
    if (s >= n_main) {
      const int ti = s - n_main, light = r ? 8 - r : 0, first = light * NT;
      int tb;
      if (r && xcd >= r) tb = ti < NT ? (xcd - r) * NT + ti : first + xcd + 8 * (ti - NT);
      else tb = first + xcd + 8 * ti;
      if (tb < TT) gru_tail16(g, tb, NT * 32, arena, hs_raw, orow_s);
      return;
    }
  }
  const int64_t mt = (int64_t)(s / NT) * 8 + xcd;
  const int nt = s % NT;
  const int64_t m0 = mt * BM;
  if (m0 >= M) return;
  const int j0 = nt * 32;
  if (tid < BM) {
    const int64_t m = min(m0 + tid, M - 1);
    orow_s[tid] = g.out_rows ? g.out_rows[m] : (int)m;
  }
  // gate biases, requested before the loop
  const int jb = min(j0 + (lane & 31), d - 1);
  const float br = g.b_ih[jb] + g.b_hh[jb];
  const float bz = g.b_ih[d + jb] + g.b_hh[d + jb];
  const float bin = g.b_ih[2 * d + jb], bhn = g.b_hh[2 * d + jb];
  const int ar = tid >> 3, ac4 = (tid & 7) * 4;
  // branch-free staging (see k_gemm): clamped addresses, zeros only for k past the segment
  const float* xrow[NA];
  const float* hrow[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int64_t m = min(m0 + ar + i * RP, M - 1);
    xrow[i] = g.x.p + (g.x.idx ? g.x.idx[m] : m) * g.x.ld;
    hrow[i] = g.h.p + (g.h.idx ? g.h.idx[m] : m) * g.h.ld;
  }
  const int nkx = (xw + BK - 1) / BK - g.x_skip_n, nkh = (d + BK - 1) / BK;  // message tiles that are processed
  const int nkt = nkx + nkh;
  // processed message tile t holds k-tile t, or t + x_skip_n past the skipped run: a column shift on the ADDRESSES of
  // those tiles (xs_sh), the k arithmetic itself runs on the compacted width xwe
  const int xs_at = g.x_skip_at, xs_sh = g.x_skip_n * BK, xwe = xw - xs_sh;
  float4 ra0[NA], rb0[NBL], ra1[NA], rb1[NBL];
  const int fr = lane & 31, fk = lane >> 5;
  f32x16 acc_r, acc_z, acc_in, acc_hn;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc_r[i] = acc_z[i] = acc_in[i] = acc_hn[i] = 0.f;
  const int dbg = g.dbg;  // bit 16: record s_memtime stamps (diagnostic knob, 0 in production)
  // ---- hand-scheduled tile step ------------------------------------------------------
  // A CU pulls only ~10 B/clk through its vector-memory path, and a wave issues in order: a
  // burst of global loads (or ds_writes) in front of the MFMAs stalls the matrix pipe until
  // the memory queue drains (measured: loop = MFMA + loads + stores, nothing hidden).  So the
  // memory work of the OTHER tiles is threaded between the MFMAs of this tile and the order
  // is pinned with sched_barrier: during the first half of a wave's k-step pairs the global
  // loads of tile t+2, during the second half the ds_writes of tile t+1 into the other LDS
  // buffer, while the operand fragments of the next pair are read one pair ahead.
  struct Frag {
    float a0, a1, b00, b01, b10, b11, b20, b21;
  };
  auto read_pair = [&](int buf, int p, Frag& f) {  // k-steps 2p and 2p+1 of the tile in LDS[buf]
    const float* ap = &As[buf][rw * 32 + fr][fk + 4 * p];
    const float* b0 = &Bs[buf][0][fr][fk + 4 * p];
    const float* b1 = &Bs[buf][1][fr][fk + 4 * p];
    const float* b2 = &Bs[buf][2][fr][fk + 4 * p];
    f.a0 = ap[0]; f.a1 = ap[2];
    f.b00 = b0[0]; f.b01 = b0[2];
    f.b10 = b1[0]; f.b11 = b1[2];
    f.b20 = b2[0]; f.b21 = b2[2];
  };
  auto load_one = [&](int t, int i, float4* ra, float4* rb) {  // i-th staged float4 of tile t
    const bool hp = t >= nkx;
    const int k = (hp ? t - nkx : t) * BK + ac4;
    const int width = hp ? d : xw;  // row stride of the weight operand
    const int kc = (k < (hp ? d : xwe) ? k : 0) + ((!hp && t >= xs_at) ? xs_sh : 0);
    // raw load from a clamped address; columns past the segment are zeroed when the tile is
    // written to LDS (store_one), so nothing consumes the load result here
    if (i < NA) {
      ra[i] = ldg4((hp ? hrow[i] : xrow[i]) + kc);
    } else {
      const int L = min(ar + (i - NA) * RP, 95);  // row of the [3 planes x 32] weight tile
      const int jc = min(j0 + (L & 31), d - 1);
      rb[i - NA] = ldg4((hp ? g.w_hh : g.w_ih) + ((int64_t)(L >> 5) * d + jc) * width + kc);
    }
  };
  auto store_one = [&](int buf, int t, int i, const float4* ra, const float4* rb) {  // tile t's i-th float4
    const bool hp = t >= nkx;
    const bool kin = (hp ? t - nkx : t) * BK + ac4 < (hp ? d : xwe);
    if (i < NA) {
      sts4(As[buf][ar + i * RP], ac4, kin ? ra[i] : zero4());
    } else {
      const int L = ar + (i - NA) * RP;
      if (L < 96) sts4(Bs[buf][L >> 5][L & 31], ac4, kin ? rb[i - NA] : zero4());
    }
  };
#define TG_SB() __builtin_amdgcn_sched_barrier(0)
  auto tile = [&](auto hp_tag, int buf, int t, float4* la, float4* lb, const float4* sa, const float4* sb) {
    constexpr bool HP = decltype(hp_tag)::value;
    const int tl = min(t + 2, nkt - 1);  // past the end: a redundant reload keeps the block branch-free
    const int p0 = ks * PP;              // this wave's share of the tile's k-step pairs
    Frag cur, nxt;
    read_pair(buf, p0, cur);
#pragma unroll
    for (int q = 0; q < PP; ++q) {
      const int op0 = (q % (PP / 2)) * SL;  // SL memory-op slots per pair; NOPS of them are used
      auto memop = [&](int i) {
        if (i < NOPS) {
          if (q < PP / 2) load_one(tl, i, la, lb);
          else store_one(buf ^ 1, t + 1, i, sa, sb);
        }
      };
      acc_r = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a0, cur.b00, acc_r, 0, 0, 0);
      if (q < PP - 1) read_pair(buf, p0 + q + 1, nxt);
      TG_SB();
      acc_z = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a0, cur.b10, acc_z, 0, 0, 0);
      memop(op0);
      TG_SB();
      if (HP) acc_hn = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a0, cur.b20, acc_hn, 0, 0, 0);
      else acc_in = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a0, cur.b20, acc_in, 0, 0, 0);
      if (SL > 3) memop(op0 + 3);
      TG_SB();
      acc_r = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a1, cur.b01, acc_r, 0, 0, 0);
      memop(op0 + 1);
      TG_SB();
      acc_z = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a1, cur.b11, acc_z, 0, 0, 0);
      TG_SB();
      if (HP) acc_hn = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a1, cur.b21, acc_hn, 0, 0, 0);
      else acc_in = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a1, cur.b21, acc_in, 0, 0, 0);
      memop(op0 + 2);
      TG_SB();
      cur = nxt;
    }
    if (HP && t == nkx + nt) {  // this A tile is h[m0.., j0..j0+32): keep it for the epilogue
      if constexpr (HREG) {
#pragma unroll
        for (int q = 0; q < NHOLD; ++q) {
          const int r = KS == 1 ? q : ks * OWN + q;
          hold_r[q] = As[buf][rw * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk][fr];
        }
      } else {
        for (int f = tid; f < BM * 32; f += THREADS) Hs[f >> 5][f & 31] = As[buf][f >> 5][f & 31];
      }
    }
    __syncthreads();
  };
#undef TG_SB
  using HP0 = std::integral_constant<bool, false>;
  using HP1 = std::integral_constant<bool, true>;
  // prologue: tile 0 -> LDS[0]; tile 1 -> registers R1
#pragma unroll
  for (int i = 0; i < NOPS; ++i) load_one(0, i, ra0, rb0);
#pragma unroll
  for (int i = 0; i < NOPS; ++i) load_one(min(1, nkt - 1), i, ra1, rb1);
#pragma unroll
  for (int i = 0; i < NOPS; ++i) store_one(0, 0, i, ra0, rb0);
  __syncthreads();
  const unsigned long long t_loop0 = (dbg & 16) ? __builtin_amdgcn_s_memtime() : 0ull;
  // Message tiles (i_n plane) first, then memory tiles (h_n plane), each as its own straight-line loop
  // over tile pairs, with the memory loops written out for both LDS-buffer parities.  A single loop with a
  // per-tile phase test moved the accumulators between registers on every path (64 v_mov_b64 per pair)
  // and its joins made the compiler wait for prefetched tiles half a tile early.
  // even tile: multiply LDS[0]; load tile t+2 -> R0; store tile t+1 (R1) -> LDS[1]; odd tile: mirrored
  int t = 0;
  for (; t + 2 <= nkx; t += 2) {
    tile(HP0{}, 0, t, ra0, rb0, ra1, rb1);
    tile(HP0{}, 1, t + 1, ra1, rb1, ra0, rb0);
  }
  if (t < nkx) {  // odd number of message tiles: the memory tiles start in LDS[1]
    tile(HP0{}, 0, t, ra0, rb0, ra1, rb1);
    for (++t; t + 2 <= nkt; t += 2) {
      tile(HP1{}, 1, t, ra1, rb1, ra0, rb0);
      tile(HP1{}, 0, t + 1, ra0, rb0, ra1, rb1);
    }
    if (t < nkt) tile(HP1{}, 1, t, ra1, rb1, ra0, rb0);
  } else {
    for (; t + 2 <= nkt; t += 2) {
      tile(HP1{}, 0, t, ra0, rb0, ra1, rb1);
      tile(HP1{}, 1, t + 1, ra1, rb1, ra0, rb0);
    }
    if (t < nkt) tile(HP1{}, 0, t, ra0, rb0, ra1, rb1);
  }
  const unsigned long long t_loop1 = (dbg & 16) ? __builtin_amdgcn_s_memtime() : 0ull;
  const int j = min(j0 + fr, d - 1);
  const bool jok = j0 + fr < d;
  auto finish = [&](int r, int hq, float ar_, float az_, float ain_, float ahn_) {  // gates + blend of accumulator row r (hq: its slot in hold_r)
    const int lr = rw * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
    const int64_t m = m0 + lr;
    const float hold = HREG ? hold_r[HREG ? hq : 0] : Hs[lr][fr];
    const int64_t orow = orow_s[lr];
    const float rg = fast_sigmoid(ar_ + br);
    const float zg = fast_sigmoid(az_ + bz);
    const float hn = ahn_ + bhn;
    const float ng = fast_tanh(ain_ + bin + rg * hn);
    if (jok && m < M) {
      const float hv = (1.f - zg) * ng + zg * hold;
      g.out[orow * g.ldo + j] = hv;
      if (g.out2) g.out2[(g.out2_by_row ? orow : m) * (int64_t)d + j] = g.add2 ? hv + g.add2[orow * d + j] : hv;
      if (g.gates) {
        float* gp = g.gates + m * 4 * (int64_t)d + j;
        gp[0] = rg; gp[d] = zg; gp[2 * d] = ng; gp[3 * d] = hn;
      }
    }
  };
  if constexpr (SCAT) {
    // Reduce-scatter over the k-groups of a row wave: group v owns accumulator registers [v OWN, (v+1) OWN) (a quarter
    // of the tile's rows with four groups).  Every group parks the registers the others own in LDS - one round, one
    // barrier - then sums its own share and runs the gate arithmetic and the stores for it, so the epilogue's
    // transcendental work is spread over all the block's wavefronts instead of the first k-group's.
    float (*sc)[KS][KS - 1][4][OWN][64] = reinterpret_cast<float (*)[KS][KS - 1][4][OWN][64]>(arena);
#pragma unroll
    for (int v = 0; v < KS; ++v) {
      if (v != ks) {  // wave-uniform
        const int slot = (ks - v - 1 + KS) % KS;
#pragma unroll
        for (int q = 0; q < OWN; ++q) {
          sc[rw][v][slot][0][q][lane] = acc_r[v * OWN + q];
          sc[rw][v][slot][1][q][lane] = acc_z[v * OWN + q];
          sc[rw][v][slot][2][q][lane] = acc_in[v * OWN + q];
          sc[rw][v][slot][3][q][lane] = acc_hn[v * OWN + q];
        }
      }
    }
    __syncthreads();
    // The partial sums of a row are added in k-group order 0, 1, .., KS - 1 WHICHEVER group owns the row: a row's result
    // must not depend on its place in the tile (the eager updater's row order comes from an atomic compaction and
    // differs from run to run; summed owner-first the step was reproducible only to the last bit or two).
    float o_r[OWN], o_z[OWN], o_in[OWN], o_hn[OWN];
#pragma unroll
    for (int gsrc = 0; gsrc < KS; ++gsrc) {
      float t_r[OWN], t_z[OWN], t_in[OWN], t_hn[OWN];
      if (gsrc == ks) {  // wave-uniform
#pragma unroll
        for (int v = 0; v < KS; ++v)
          if (v == ks) {
#pragma unroll
            for (int q = 0; q < OWN; ++q) {
              t_r[q] = acc_r[v * OWN + q]; t_z[q] = acc_z[v * OWN + q];
              t_in[q] = acc_in[v * OWN + q]; t_hn[q] = acc_hn[v * OWN + q];
            }
          }
      } else {
        const int sl = (gsrc - ks - 1 + KS) % KS;
#pragma unroll
        for (int q = 0; q < OWN; ++q) {
          t_r[q] = sc[rw][ks][sl][0][q][lane]; t_z[q] = sc[rw][ks][sl][1][q][lane];
          t_in[q] = sc[rw][ks][sl][2][q][lane]; t_hn[q] = sc[rw][ks][sl][3][q][lane];
        }
      }
#pragma unroll
      for (int q = 0; q < OWN; ++q) {
        o_r[q] = gsrc == 0 ? t_r[q] : o_r[q] + t_r[q];
        o_z[q] = gsrc == 0 ? t_z[q] : o_z[q] + t_z[q];
        o_in[q] = gsrc == 0 ? t_in[q] : o_in[q] + t_in[q];
        o_hn[q] = gsrc == 0 ? t_hn[q] : o_hn[q] + t_hn[q];
      }
    }
#pragma unroll
    for (int q = 0; q < OWN; ++q) finish(ks * OWN + q, q, o_r[q], o_z[q], o_in[q], o_hn[q]);
  } else {
  // fold the k-groups' partial sums into group 0, halving the number of live groups per round: groups
  // [half, 2 half) write, groups [0, half) add (the last tile's barrier has retired every read of the tiles)
#pragma unroll
  for (int half = KS / 2; half >= 1; half /= 2) {
    if (ks >= half && ks < 2 * half) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        red[ks - half][0][rw][r][lane] = acc_r[r];
        red[ks - half][1][rw][r][lane] = acc_z[r];
        red[ks - half][2][rw][r][lane] = acc_in[r];
        red[ks - half][3][rw][r][lane] = acc_hn[r];
      }
    }
    __syncthreads();
    if (ks < half) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc_r[r] += red[ks][0][rw][r][lane];
        acc_z[r] += red[ks][1][rw][r][lane];
        acc_in[r] += red[ks][2][rw][r][lane];
        acc_hn[r] += red[ks][3][rw][r][lane];
      }
    }
    if (half > 1) __syncthreads();  // the next round overwrites the slots
  }
  if (ks == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) finish(r, r, acc_r[r], acc_z[r], acc_in[r], acc_hn[r]);
  }
  }
  if ((dbg & 16) && tid == 0 && blockIdx.x < 2048) {
    g_gru_trace[blockIdx.x * 4 + 0] = t_entry;
    g_gru_trace[blockIdx.x * 4 + 1] = t_loop0;
    g_gru_trace[blockIdx.x * 4 + 2] = t_loop1;
    g_gru_trace[blockIdx.x * 4 + 3] = __builtin_amdgcn_s_memtime();
  }
}

// ---------------------------------------------------------------------------------
// The GRU cell for FEW rows (the eager updater of a C2-sized batch: ~1 000 rows): 32 rows x 32 hidden columns
// per block, four wavefronts, and NO LDS in the k-loop.
// In a 32-row block the four wavefronts share nothing: with one row wave, LDS staging only re-shapes global
// rows into MFMA fragments, and that costs more than the MFMAs (s_memtime ablations of k_gru<1, 4>: 44.9 k
// cycles per block loop, 27.2 k without the LDS stores, 25.1 k for the MFMAs alone - the store path moves
// 64-79 B/clk per CU and every ds_write holds the issuing wave).  The sum over k does not care which k values
// share an MFMA step, so a lane can feed the matrix unit straight from what it loads: lane (row r, half kh)
// reads the 64 contiguous bytes A[r][k0 + 16 kh .. + 15] of its row as four float4, the same slice of its weight
// row in each of the three planes, and MFMA step (q, j) multiplies element j of float4 q - k = k0 + 16 kh + 4 q + j
// on both operands.  The k-tiles are dealt to the wavefronts (wave w takes tiles w, w + 4, ...), each into its own
// accumulators: no barrier and no LDS until the fold, a tile is 16 loads and 48 MFMAs of one wavefront, the next
// tile's loads are in flight meanwhile.  Fold and epilogue as k_gru's scattered form: every wavefront finishes
// a quarter of the rows; the old-memory values and output rows of those are requested at kernel start.
// ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_gru_direct(GruArgs g) {
  constexpr int KS = 4, OWN = 4;
  __shared__ float sc_raw[KS * (KS - 1) * 4 * OWN * 64];
  float (*sc)[KS - 1][4][OWN][64] = reinterpret_cast<float (*)[KS - 1][4][OWN][64]>(sc_raw);
  const unsigned long long t_entry = (g.dbg & 16) ? __builtin_amdgcn_s_memtime() : 0ull;
  const int tid = threadIdx.x, lane = tid & 63, ks = tid >> 6;
  const int fr = lane & 31, fk = lane >> 5;
  const int d = g.d, xw = g.xw;
  const int NT = (d + 31) / 32;
  int64_t M = g.cap;
  if (g.n_dev) M = min(M, (int64_t)*g.n_dev);
  const int xcd = blockIdx.x & 7, s = blockIdx.x >> 3;
  const int64_t mt = (int64_t)(s / NT) * 8 + xcd;
  const int nt = s % NT;
  const int64_t m0 = mt * 32;
  if (m0 >= M) return;
  const int j0 = nt * 32;
  const int jc = min(j0 + fr, d - 1);
  const bool jok = j0 + fr < d;
  // this lane's operand rows: activation row m0 + fr, weight row jc of every plane
  const int64_t mrow = min(m0 + fr, M - 1);
  const float* xrow = g.x.p + (g.x.idx ? g.x.idx[mrow] : mrow) * g.x.ld;
  const float* hrow = g.h.p + (g.h.idx ? g.h.idx[mrow] : mrow) * g.h.ld;
  const float* wi = g.w_ih + (int64_t)jc * xw;
  const float* wh = g.w_hh + (int64_t)jc * d;
  const int64_t wi_ps = (int64_t)d * xw, wh_ps = (int64_t)d * d;  // plane strides
  // epilogue operands of the rows this wavefront finishes (accumulator registers [4 ks, 4 ks + 4))
  float hold[OWN], addv[OWN];  // (addv: GruArgs.add2 of the row's node, requested with the old memory value - same depth)
  int64_t orow[OWN];
#pragma unroll
  for (int q = 0; q < OWN; ++q) {
    const int64_t mm = min(m0 + 8 * ks + q + 4 * fk, M - 1);
    const int64_t node = g.h.idx ? g.h.idx[mm] : mm;
    hold[q] = g.h.p[node * g.h.ld + jc];
    orow[q] = g.out_rows ? (int64_t)g.out_rows[mm] : mm;
    addv[q] = (g.out2 && g.add2) ? g.add2[orow[q] * d + jc] : 0.f;  // by the OUTPUT row, as every other body (GruArgs.add2)
  }
  const float br = g.b_ih[jc] + g.b_hh[jc];
  const float bz = g.b_ih[d + jc] + g.b_hh[d + jc];
  const float bin = g.b_ih[2 * d + jc], bhn = g.b_hh[2 * d + jc];
  const int nkx = (xw + BK - 1) / BK - g.x_skip_n, nkh = (d + BK - 1) / BK;
  const int nkt = nkx + nkh;
  const int xs_at = g.x_skip_at, xs_sh = g.x_skip_n * BK, xwe = xw - xs_sh;  // zero k-tiles skipped (see k_gru)
  // this wavefront's tiles: message tiles ks, ks + 4, ... < nkx, then memory tiles th0, th0 + 4, ... < nkt
  const int nx = ks < nkx ? (nkx - ks + 3) / 4 : 0;
  const int th0 = nkx + ((ks - nkx) % 4 + 4) % 4;
  const int nh = th0 < nkt ? (nkt - th0 + 3) / 4 : 0;
  const int n_my = nx + nh;
  auto tile_of = [&](int i) { return i < nx ? ks + 4 * i : th0 + 4 * (i - nx); };
  struct Tile {
    float4 a[4], w0[4], w1[4], w2[4];
  };
  // raw loads from clamped addresses; `live` bit q: float4 q of the activation slice lies inside the operand (the
  // others are taken as zero when they are used - the weight slice then multiplies zeros, whatever it holds)
  auto load_tile = [&](int i, Tile& T, unsigned& live) {
    // past the end: a redundant reload keeps the code branch-free; a wavefront without tiles (fewer than four k-tiles
    // in all) reads tile th0 >= nkt, whose every k is out of range: clamped addresses, nothing live
    const int t = tile_of(max(0, min(i, n_my - 1)));
    const bool hp = t >= nkx;
    const int kb = (hp ? t - nkx : t) * BK + 16 * fk;
    const int sh = (!hp && t >= xs_at) ? xs_sh : 0;
    const int wid = hp ? d : xwe;
    const float* ar = hp ? hrow : xrow;
    const float* wr = hp ? wh : wi;
    const int64_t ps = hp ? wh_ps : wi_ps;
    live = 0u;
    int kc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = kb + 4 * q;
      if (k < wid) live |= 1u << q;
      kc[q] = (k < wid ? k : 0) + sh;
    }
    // the four float4 of one row slice are requested back to back (one cache line each row)
#pragma unroll
    for (int q = 0; q < 4; ++q) T.a[q] = ldg4(ar + kc[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) T.w0[q] = ldg4(wr + kc[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) T.w1[q] = ldg4(wr + ps + kc[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) T.w2[q] = ldg4(wr + 2 * ps + kc[q]);
  };
  f32x16 acc_r, acc_z, acc_in, acc_hn;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc_r[i] = acc_z[i] = acc_in[i] = acc_hn[i] = 0.f;
  auto mma_tile = [&](auto hp_tag, const Tile& T, unsigned live) {
    constexpr bool HP = decltype(hp_tag)::value;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 a = ((live >> q) & 1u) ? T.a[q] : zero4();
      const float av[4] = {a.x, a.y, a.z, a.w};
      const float b0[4] = {T.w0[q].x, T.w0[q].y, T.w0[q].z, T.w0[q].w};
      const float b1[4] = {T.w1[q].x, T.w1[q].y, T.w1[q].z, T.w1[q].w};
      const float b2[4] = {T.w2[q].x, T.w2[q].y, T.w2[q].z, T.w2[q].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc_r = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b0[j], acc_r, 0, 0, 0);
        acc_z = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b1[j], acc_z, 0, 0, 0);
        if (HP) acc_hn = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b2[j], acc_hn, 0, 0, 0);
        else acc_in = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b2[j], acc_in, 0, 0, 0);
      }
    }
  };
  using HP0 = std::integral_constant<bool, false>;
  using HP1 = std::integral_constant<bool, true>;
  Tile T0, T1;
  unsigned l0 = 0u, l1 = 0u;
  load_tile(0, T0, l0);
  const unsigned long long t_loop0 = (g.dbg & 16) ? __builtin_amdgcn_s_memtime() : 0ull;
  // One step: request tile i + 1 into the idle register set, THEN multiply tile i (the order is pinned: left to
  // itself the scheduler sinks the loads to the end of the MFMA stream, where the next tile waits for them in full).
  // Message tiles (i_n plane) first, then memory tiles (h_n plane), each as straight-line pairs, written out for both
  // register parities of the phase change.
#define TG_STEP(HPT, CUR, LCUR, NXT, LNXT, INEXT)     \
  do {                                                \
    load_tile(INEXT, NXT, LNXT);                      \
    __builtin_amdgcn_sched_barrier(0);                \
    mma_tile(HPT{}, CUR, LCUR);                       \
    __builtin_amdgcn_sched_barrier(0);                \
  } while (0)
  int i = 0;
  for (; i + 2 <= nx; i += 2) {
    TG_STEP(HP0, T0, l0, T1, l1, i + 1);
    TG_STEP(HP0, T1, l1, T0, l0, i + 2);
  }
  if (i < nx) {  // odd number of message tiles: the memory tiles start in the other register set
    TG_STEP(HP0, T0, l0, T1, l1, i + 1);
    for (++i; i + 2 <= n_my; i += 2) {
      TG_STEP(HP1, T1, l1, T0, l0, i + 1);
      TG_STEP(HP1, T0, l0, T1, l1, i + 2);
    }
    if (i < n_my) mma_tile(HP1{}, T1, l1);
  } else {
    for (; i + 2 <= n_my; i += 2) {
      TG_STEP(HP1, T0, l0, T1, l1, i + 1);
      TG_STEP(HP1, T1, l1, T0, l0, i + 2);
    }
    if (i < n_my) mma_tile(HP1{}, T0, l0);
  }
#undef TG_STEP
  const unsigned long long t_loop1 = (g.dbg & 16) ? __builtin_amdgcn_s_memtime() : 0ull;
  // reduce-scatter over the four wavefronts (as k_gru's scattered epilogue): park what the others own, sum one's own
#pragma unroll
  for (int v = 0; v < KS; ++v) {
    if (v != ks) {
      const int slot = (ks - v - 1 + KS) % KS;
#pragma unroll
      for (int q = 0; q < OWN; ++q) {
        sc[v][slot][0][q][lane] = acc_r[v * OWN + q];
        sc[v][slot][1][q][lane] = acc_z[v * OWN + q];
        sc[v][slot][2][q][lane] = acc_in[v * OWN + q];
        sc[v][slot][3][q][lane] = acc_hn[v * OWN + q];
      }
    }
  }
  __syncthreads();
  // in wavefront order 0..3 whichever wavefront owns the row (see k_gru: the result must not depend on the row's place)
  float o_r[OWN], o_z[OWN], o_in[OWN], o_hn[OWN];
#pragma unroll
  for (int gsrc = 0; gsrc < KS; ++gsrc) {
    float t_r[OWN], t_z[OWN], t_in[OWN], t_hn[OWN];
    if (gsrc == ks) {  // wave-uniform
#pragma unroll
      for (int v = 0; v < KS; ++v)
        if (v == ks) {
#pragma unroll
          for (int q = 0; q < OWN; ++q) {
            t_r[q] = acc_r[v * OWN + q]; t_z[q] = acc_z[v * OWN + q];
            t_in[q] = acc_in[v * OWN + q]; t_hn[q] = acc_hn[v * OWN + q];
          }
        }
    } else {
      const int sl = (gsrc - ks - 1 + KS) % KS;
#pragma unroll
      for (int q = 0; q < OWN; ++q) {
        t_r[q] = sc[ks][sl][0][q][lane]; t_z[q] = sc[ks][sl][1][q][lane];
        t_in[q] = sc[ks][sl][2][q][lane]; t_hn[q] = sc[ks][sl][3][q][lane];
      }
    }
#pragma unroll
    for (int q = 0; q < OWN; ++q) {
      o_r[q] = gsrc == 0 ? t_r[q] : o_r[q] + t_r[q];
      o_z[q] = gsrc == 0 ? t_z[q] : o_z[q] + t_z[q];
      o_in[q] = gsrc == 0 ? t_in[q] : o_in[q] + t_in[q];
      o_hn[q] = gsrc == 0 ? t_hn[q] : o_hn[q] + t_hn[q];
    }
  }
#pragma unroll
  for (int q = 0; q < OWN; ++q) {
    const int64_t m = m0 + 8 * ks + q + 4 * fk;
    const float rg = fast_sigmoid(o_r[q] + br);
    const float zg = fast_sigmoid(o_z[q] + bz);
    const float hn = o_hn[q] + bhn;
    const float ng = fast_tanh(o_in[q] + bin + rg * hn);
    if (jok && m < M) {
      const float hv = (1.f - zg) * ng + zg * hold[q];
      g.out[orow[q] * g.ldo + j0 + fr] = hv;
      if (g.out2) g.out2[(g.out2_by_row ? orow[q] : m) * (int64_t)d + j0 + fr] = hv + addv[q];
      if (g.gates) {
        float* gp = g.gates + m * 4 * (int64_t)d + j0 + fr;
        gp[0] = rg; gp[d] = zg; gp[2 * d] = ng; gp[3 * d] = hn;
      }
    }
  }
  if ((g.dbg & 16) && tid == 0 && blockIdx.x < 2048) {
    g_gru_trace[blockIdx.x * 4 + 0] = t_entry;
    g_gru_trace[blockIdx.x * 4 + 1] = t_loop0;
    g_gru_trace[blockIdx.x * 4 + 2] = t_loop1;
    g_gru_trace[blockIdx.x * 4 + 3] = __builtin_amdgcn_s_memtime();
  }
}

// ---- LDS-free updater blocks on 16 x 16 MFMA tiles: 16 RT rows x 16 hidden columns ------------------------------------
// k_gru_direct's 32 x 32 blocks leave CUs idle whenever (row tiles x column tiles) is not close to 256: C2's ~1 060 rows at
// d = 172 are 34 x 6 = 204 blocks, and the launch lasts as long as ONE block.  On v_mfma_f32_16x16x4_f32 (same flops per
// cycle) the hidden width is cut into 16-column tiles (172 -> 11 tiles, 2 % padding instead of 10 %) and a block owns 16,
// 32 or 48 rows: the kernel picks, from the LIVE row count, the smallest of the three whose blocks all fit the chip at
// once (least work per block; C2: 23 x 11 = 253 blocks of 48 rows, three quarters of the work of a 32 x 32 block each;
// the batch-of-200 workload: 32-row blocks).  Same scheme otherwise: no LDS in the k-loop, a lane feeds the matrix unit
// from what it loads (lane (row i, quarter kq) reads the 32 contiguous bytes A[i][k0 + 8 kq ..] of each of its RT rows
// and of its weight row in each plane; MFMA step (q, j) multiplies element j of float4 q on both operands - the sum over
// k does not care which k values share a step), the k-tiles are dealt to the four wavefronts, whose accumulators meet
// in a reduce-scatter through LDS (k-group order: bit-reproducible).  Blocks are dealt to the XCDs in contiguous chunks of
// the (row tile, column tile) sequence - balanced to within one block, and a row tile's gathered rows are fetched by one
// XCD's L2, two at a chunk border.
// BL: the blend form (GruArgs.w_blend): a fifth plane w_blend[j, :] . t over the memory-side k-tiles gives the old memory
// value of the blend term instead of a load; everything else - tiles, k order, fold order - is the present form's.
template <int RT, bool BL = false>
__device__ __forceinline__ void gru_direct16_body(const GruArgs& g, int64_t M, int64_t mt, int nt, float* sc_raw) {
  constexpr int KS = 4, NP = BL ? 5 : 4;
  TG_PT(const unsigned long long pt_entry = (g.dbg & 16) ? __builtin_amdgcn_s_memtime() : 0ull;)  // (diagnostic, as in gemm_ks16_tile)
  float (*sc)[KS - 1][NP][RT][64] = reinterpret_cast<float (*)[KS - 1][NP][RT][64]>(sc_raw);  // [owner][slot][plane][row tile]
  const int tid = threadIdx.x, lane = tid & 63, ks = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int d = g.d, xw = g.xw;
  const int64_t m0 = mt * (16 * RT);
  const int j0 = nt * 16;
  const int jc = min(j0 + li, d - 1);
  const bool jok = j0 + li < d;
  const float* xrow[RT];
  const float* hrow[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int64_t mrow = min(m0 + 16 * rt + li, M - 1);
    xrow[rt] = g.x.p + (g.x.idx ? g.x.idx[mrow] : mrow) * g.x.ld;
    hrow[rt] = g.h.p + (g.h.idx ? g.h.idx[mrow] : mrow) * g.h.ld;
  }
  const float* wi = g.w_ih + (int64_t)jc * xw;
  const float* wh = g.w_hh + (int64_t)jc * d;
  const float* wb = BL ? g.w_blend + (int64_t)jc * d : nullptr;
  const int64_t wi_ps = (int64_t)d * xw, wh_ps = (int64_t)d * d;  // plane strides
  // epilogue operands of the rows this wavefront finishes: accumulator register ks of every row tile (row 4 lk + ks)
  float hold[RT], addv[RT];
  int64_t orow[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int64_t mm = min(m0 + 16 * rt + 4 * lk + ks, M - 1);
    orow[rt] = g.out_rows ? (int64_t)g.out_rows[mm] : mm;
    hold[rt] = BL ? 0.f : g.h.p[(g.h.idx ? g.h.idx[mm] : mm) * g.h.ld + jc];
    addv[rt] = (g.out2 && g.add2) ? g.add2[orow[rt] * d + jc] : 0.f;  // by the OUTPUT row, as every other body (GruArgs.add2)
  }
  const float bb = BL ? g.b_blend[jc] : 0.f;
  const float br = g.b_ih[jc] + g.b_hh[jc];
  const float bz = g.b_ih[d + jc] + g.b_hh[d + jc];
  const float bin = g.b_ih[2 * d + jc], bhn = g.b_hh[2 * d + jc];
  const int nkx = (xw + BK - 1) / BK - g.x_skip_n, nkh = (d + BK - 1) / BK;
  const int nkt = nkx + nkh;
  const int xs_at = g.x_skip_at, xs_sh = g.x_skip_n * BK, xwe = xw - xs_sh;  // zero k-tiles skipped (see k_gru)
  // this wavefront's tiles: message tiles ks, ks + 4, ... < nkx, then memory tiles th0, th0 + 4, ... < nkt
  const int nx = ks < nkx ? (nkx - ks + 3) / 4 : 0;
  const int th0 = nkx + ((ks - nkx) % 4 + 4) % 4;
  const int nh = th0 < nkt ? (nkt - th0 + 3) / 4 : 0;
  const int n_my = nx + nh;
  auto tile_of = [&](int i) { return i < nx ? ks + 4 * i : th0 + 4 * (i - nx); };
  struct Tile {
    float4 a[RT][2], w0[2], w1[2], w2[2], w3[BL ? 2 : 1];
  };
  auto load_tile = [&](int i, Tile& T, unsigned& live) {  // raw loads from clamped addresses (see k_gru_direct)
    const int t = tile_of(max(0, min(i, n_my - 1)));
    const bool hp = t >= nkx;
    const int kb = (hp ? t - nkx : t) * BK + 8 * lk;
    const int sh = (!hp && t >= xs_at) ? xs_sh : 0;
    const int wid = hp ? d : xwe;
    const float* wr = hp ? wh : wi;
    const int64_t ps = hp ? wh_ps : wi_ps;
    live = 0u;
    int kc[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int k = kb + 4 * q;
      if (k < wid) live |= 1u << q;
      kc[q] = (k < wid ? k : 0) + sh;
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int q = 0; q < 2; ++q) T.a[rt][q] = ldg4((hp ? hrow[rt] : xrow[rt]) + kc[q]);
#pragma unroll
    for (int q = 0; q < 2; ++q) T.w0[q] = ldg4(wr + kc[q]);
#pragma unroll
    for (int q = 0; q < 2; ++q) T.w1[q] = ldg4(wr + ps + kc[q]);
#pragma unroll
    for (int q = 0; q < 2; ++q) T.w2[q] = ldg4(wr + 2 * ps + kc[q]);
    if constexpr (BL) {  // (message tiles: a valid address, the values are not used)
#pragma unroll
      for (int q = 0; q < 2; ++q) T.w3[q] = ldg4(wb + (hp ? kc[q] : 0));
    }
  };
  f32x4m acc_r[RT], acc_z[RT], acc_in[RT], acc_hn[RT], acc_hb[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) acc_r[rt] = acc_z[rt] = acc_in[rt] = acc_hn[rt] = acc_hb[rt] = f32x4m{0.f, 0.f, 0.f, 0.f};
  auto mma_tile = [&](auto hp_tag, const Tile& T, unsigned live) {
    constexpr bool HP = decltype(hp_tag)::value;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      float av[RT][4];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const float4 a = ((live >> q) & 1u) ? T.a[rt][q] : zero4();
        av[rt][0] = a.x; av[rt][1] = a.y; av[rt][2] = a.z; av[rt][3] = a.w;
      }
      const float b0[4] = {T.w0[q].x, T.w0[q].y, T.w0[q].z, T.w0[q].w};
      const float b1[4] = {T.w1[q].x, T.w1[q].y, T.w1[q].z, T.w1[q].w};
      const float b2[4] = {T.w2[q].x, T.w2[q].y, T.w2[q].z, T.w2[q].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc_r[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][j], b0[j], acc_r[rt], 0, 0, 0);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc_z[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][j], b1[j], acc_z[rt], 0, 0, 0);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          if (HP) acc_hn[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][j], b2[j], acc_hn[rt], 0, 0, 0);
          else acc_in[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][j], b2[j], acc_in[rt], 0, 0, 0);
        }
        if constexpr (BL && HP) {
          const float b3[4] = {T.w3[q].x, T.w3[q].y, T.w3[q].z, T.w3[q].w};
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) acc_hb[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][j], b3[j], acc_hb[rt], 0, 0, 0);
        }
      }
    }
  };
  using HP0 = std::integral_constant<bool, false>;
  using HP1 = std::integral_constant<bool, true>;
  Tile T0, T1;
  unsigned l0 = 0u, l1 = 0u;
  load_tile(0, T0, l0);
#define TG_STEP(HPT, CUR, LCUR, NXT, LNXT, INEXT)     \
  do {                                                \
    load_tile(INEXT, NXT, LNXT);                      \
    __builtin_amdgcn_sched_barrier(0);                \
    mma_tile(HPT{}, CUR, LCUR);                       \
    __builtin_amdgcn_sched_barrier(0);                \
  } while (0)
  TG_PT(const unsigned long long pt_loop0 = (g.dbg & 16) ? __builtin_amdgcn_s_memtime() : 0ull;)
  int i = 0;
  for (; i + 2 <= nx; i += 2) {
    TG_STEP(HP0, T0, l0, T1, l1, i + 1);
    TG_STEP(HP0, T1, l1, T0, l0, i + 2);
  }
  if (i < nx) {  // odd number of message tiles: the memory tiles start in the other register set
    TG_STEP(HP0, T0, l0, T1, l1, i + 1);
    for (++i; i + 2 <= n_my; i += 2) {
      TG_STEP(HP1, T1, l1, T0, l0, i + 1);
      TG_STEP(HP1, T0, l0, T1, l1, i + 2);
    }
    if (i < n_my) mma_tile(HP1{}, T1, l1);
  } else {
    for (; i + 2 <= n_my; i += 2) {
      TG_STEP(HP1, T0, l0, T1, l1, i + 1);
      TG_STEP(HP1, T1, l1, T0, l0, i + 2);
    }
    if (i < n_my) mma_tile(HP1{}, T0, l0);
  }
#undef TG_STEP
  TG_PT(unsigned long long pt_loop1 = 0ull; if (g.dbg & 16) {
    asm volatile("s_nop 0" ::"v"(acc_r[0][0]));
    pt_loop1 = __builtin_amdgcn_s_memtime();
  })
  // reduce-scatter over the four wavefronts: wavefront v finishes accumulator register v of every row tile; the others'
  // registers are parked in LDS (one round, one barrier)
#pragma unroll
  for (int v = 0; v < KS; ++v) {
    if (v != ks) {  // wave-uniform
      const int slot = (ks - v - 1 + KS) % KS;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        sc[v][slot][0][rt][lane] = acc_r[rt][v];
        sc[v][slot][1][rt][lane] = acc_z[rt][v];
        sc[v][slot][2][rt][lane] = acc_in[rt][v];
        sc[v][slot][3][rt][lane] = acc_hn[rt][v];
        if constexpr (BL) sc[v][slot][NP - 1][rt][lane] = acc_hb[rt][v];
      }
    }
  }
  __syncthreads();
  // partial sums are added in wavefront order 0..3 whichever wavefront owns the row (k_gru: a row's result must not
  // depend on its place in the tile)
  float o_r[RT], o_z[RT], o_in[RT], o_hn[RT], o_hb[RT];
#pragma unroll
  for (int gsrc = 0; gsrc < KS; ++gsrc) {
    float t_r[RT], t_z[RT], t_in[RT], t_hn[RT], t_hb[RT];
    if (gsrc == ks) {  // wave-uniform
#pragma unroll
      for (int v = 0; v < KS; ++v)
        if (v == ks) {
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) {
            t_r[rt] = acc_r[rt][v]; t_z[rt] = acc_z[rt][v]; t_in[rt] = acc_in[rt][v]; t_hn[rt] = acc_hn[rt][v];
            t_hb[rt] = acc_hb[rt][v];
          }
        }
    } else {
      const int sl = (gsrc - ks - 1 + KS) % KS;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        t_r[rt] = sc[ks][sl][0][rt][lane]; t_z[rt] = sc[ks][sl][1][rt][lane];
        t_in[rt] = sc[ks][sl][2][rt][lane]; t_hn[rt] = sc[ks][sl][3][rt][lane];
        t_hb[rt] = BL ? sc[ks][sl][NP - 1][rt][lane] : 0.f;
      }
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      o_r[rt] = gsrc == 0 ? t_r[rt] : o_r[rt] + t_r[rt];
      o_z[rt] = gsrc == 0 ? t_z[rt] : o_z[rt] + t_z[rt];
      o_in[rt] = gsrc == 0 ? t_in[rt] : o_in[rt] + t_in[rt];
      o_hn[rt] = gsrc == 0 ? t_hn[rt] : o_hn[rt] + t_hn[rt];
      o_hb[rt] = gsrc == 0 ? t_hb[rt] : o_hb[rt] + t_hb[rt];
    }
  }
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    if constexpr (BL) hold[rt] = o_hb[rt] + bb;
    const int64_t m = m0 + 16 * rt + 4 * lk + ks;
    const float rg = fast_sigmoid(o_r[rt] + br);
    const float zg = fast_sigmoid(o_z[rt] + bz);
    const float hn = o_hn[rt] + bhn;
    const float ng = fast_tanh(o_in[rt] + bin + rg * hn);
    if (jok && m < M) {
      const float hv = (1.f - zg) * ng + zg * hold[rt];
      g.out[orow[rt] * g.ldo + j0 + li] = hv;
      if (g.out2) g.out2[(g.out2_by_row ? orow[rt] : m) * (int64_t)d + j0 + li] = hv + addv[rt];
      if (g.gates) {
        float* gp = g.gates + m * 4 * (int64_t)d + j0 + li;
        gp[0] = rg; gp[d] = zg; gp[2 * d] = ng; gp[3 * d] = hn;
      }
    }
  }
  TG_PT(if ((g.dbg & 16) && tid == 0 && blockIdx.x < 2048) {
    g_gru_trace[blockIdx.x * 4 + 0] = pt_entry;
    g_gru_trace[blockIdx.x * 4 + 1] = pt_loop0;
    g_gru_trace[blockIdx.x * 4 + 2] = pt_loop1;
    g_gru_trace[blockIdx.x * 4 + 3] = __builtin_amdgcn_s_memtime();
  })
}

constexpr int GRU16_RT_MAX = 6;
// RTM: the most rows / 16 this instance offers (3: 16 / 32 / 48 rows, 176 + 72 registers; 6: also 64 / 96, 254 + 144 - the
// bigger register file costs the 48-row blocks 5 %, so launches whose bound fits 48-row blocks take the small instance)
template <int RTM, bool BL = false>
__global__ void __launch_bounds__(256) k_gru_direct16(GruArgs g) {
  __shared__ float sc_raw[4 * 3 * (BL ? 5 : 4) * RTM * 64];
  int64_t M = g.cap;
  if (g.n_dev) M = min(M, (int64_t)*g.n_dev);
  if (M <= 0) return;
  const int NT = (g.d + 15) / 16;
  // rows per block from the LIVE row count: the smallest of 16 / 32 / 48 (/ 64 / 96) whose blocks fit the 256 CUs at once
  int rt = RTM;
  if (((M + 15) / 16) * NT <= 256) rt = 1;
  else if (((M + 31) / 32) * NT <= 256) rt = 2;
  else if (RTM > 3 && ((M + 47) / 48) * NT <= 256) rt = 3;
  else if (RTM > 3 && ((M + 63) / 64) * NT <= 256) rt = 4;
  const int64_t total = ((M + 16 * rt - 1) / (16 * rt)) * NT;
  // XCD x (blockIdx % 8) works through the chunk [x per, (x + 1) per) of the tile sequence.  The grid is 256 blocks whatever
  // the capacity (no tail of dead blocks: the row CAPACITY of the eager updater is twice its live rows and more); a row
  // count beyond the largest blocks' single round makes blocks take a second tile
  const int64_t per = (total + 7) / 8;
  for (int64_t jx = blockIdx.x >> 3; jx < per; jx += gridDim.x >> 3) {
    const int64_t b = (int64_t)(blockIdx.x & 7) * per + jx;
    if (b >= total) break;
    const int64_t mt = b / NT;
    const int nt = (int)(b - mt * NT);
    if (rt == 1) gru_direct16_body<1, BL>(g, M, mt, nt, sc_raw);
    else if (rt == 2) gru_direct16_body<2, BL>(g, M, mt, nt, sc_raw);
    else if (RTM == 3 || rt == 3) gru_direct16_body<3, BL>(g, M, mt, nt, sc_raw);
    else if (rt == 4) gru_direct16_body<(RTM > 3 ? 4 : 3), BL>(g, M, mt, nt, sc_raw);
    else gru_direct16_body<RTM, BL>(g, M, mt, nt, sc_raw);
    __syncthreads();  // the fold's LDS is re-used by the next tile
  }
}

extern "C" int tg_debug_gru_trace(unsigned long long* out_host, int n_blocks) {
  return hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_gru_trace), sizeof(unsigned long long) * 4 * n_blocks) == hipSuccess ? 0 : -4;
}

// the condition under which gru_launch takes k_gru_direct16 (below), for callers that must know before they launch
static bool gru_d16_fits(int64_t cap, int64_t rows_hint, int d) {
  const int64_t rows_b = rows_hint > 0 ? std::min<int64_t>(rows_hint, cap) : cap;
  return cdiv(rows_b, 16 * GRU16_RT_MAX) * ((d + 15) / 16) <= 256;
}
bool gru_blend_ok(int64_t cap, int64_t rows_hint, int d) {
  static const int force_nw = env_int("TG_GRU_NW", 0), d16_knob = env_int("TG_GRU_D16", 1);
  return cap > 0 && force_nw == 0 && d16_knob && (d16_knob == 3 || gru_d16_fits(cap, rows_hint, d));
}

int gru_launch(const GruArgs& g, hipStream_t st) {
  if (g.cap <= 0) return TG_OK;
  if (g.d <= 0 || (g.d % 4) || g.xw <= 0 || (g.xw % 4)) return TG_EINVAL;
  // the blend form exists in the 16 x 16 kernel only, without gate outputs (gru_blend_ok; a missing kernel is an error)
  if (g.w_blend && (!g.b_blend || g.gates || !gru_blend_ok(g.cap, g.rows_hint, g.d))) return TG_EUNSUPPORTED;
  static const int dbg = env_int("TG_GRU_DBG", 0);  // bit 16: trace stamps
  static const int force_nw = env_int("TG_GRU_NW", 0);  // tuning knob
  GruArgs a = g;
  a.dbg = dbg;
  const int NT = (g.d + 31) / 32;
  // small problems (at most ~64k live rows): 64-row blocks double the block count so that two
  // blocks share a CU and cover each other's stalls; large ones keep 128 rows (half the weight traffic)
  static const int ks_knob = env_int("TG_GRU_KS", 0);  // tuning knob: 0 = by the grid (below)
  // 96-row blocks (four k-groups of three row waves: 12 wavefronts, three per SIMD) with the partial column tile
  // as 16-column blocks: a quarter less work per block and no padded columns, which pays exactly when the whole
  // launch fits the chip in ONE round - every CU runs at most one block, so the duration is one block's duration
  // (C2 shapes, 4174 rows: 61.9 -> 51.8 us).  One block more than CUs and it costs a second round (4400 rows:
  // 83 us), so the choice needs a guaranteed bound on the live rows: rows_hint (the caller's bound, e.g. the node
  // count), not the capacity.  At C2's steady state (4350-4550 involved nodes of 9228) it does not apply.
  // Smaller still when it fits: 64-row blocks (k_gru<2, 4>, 8 wavefronts; 1588 rows at d = 172: 36 us against
  // 47 us with 96 rows and 58 us with 128).  Its blocks follow the plain XCD map, so every XCD must hold its
  // share: ceil(row tiles / 8) x column tiles <= 32 CUs.
  bool small = false, tiny = false, micro = false;
  {
    const int tail = g.d % 32;
    const bool use_tail = tail > 0 && tail <= 16;
    const int64_t rows = g.rows_hint > 0 ? std::min<int64_t>(g.rows_hint, g.cap) : g.cap;
    const int64_t blocks96 = cdiv(rows, 96) * (NT - (use_tail ? 1 : 0)) + (use_tail ? cdiv(rows, T16_ROWS) : 0);
    small = blocks96 + 8 <= 256;  // (+8: the per-XCD dealing can leave one XCD a block short of full)
    tiny = cdiv(cdiv(rows, 64), 8) * NT <= 32;
    // fewer rows still: 32-row blocks (k_gru<1, 4>, four wavefronts) double the block count once more - the updater of the
    // eager step runs on ~1000 rows at C2: 17 x 6 = 102 blocks of 64 rows leave 154 CUs idle, 34 x 6 = 204 do not.  An XCD
    // that ends up with a few more blocks than its 32 CUs co-hosts two of these small blocks on a CU (no second round)
    micro = cdiv(cdiv(rows, 32), 8) * NT <= 40;
  }
  static const int micro_knob = env_int("TG_GRU_MICRO", 1);  // tuning knob: 0 = off
  {
    // LDS-free blocks of 16 hidden columns x 16 .. 96 rows (k_gru_direct16 picks the rows per block from the live row
    // count): whenever the caller's bound on the rows says that the 96-row blocks fit the chip at once.  Measured against
    // the kernels below (d = 172): 380 rows 18.5 -> 11.3 us, 1 060 rows 19.9 -> 16.1 us; d = 100, 1 060 rows 14.7 -> 9.3 us
    static const int d16_knob = env_int("TG_GRU_D16", 1);  // tuning knob: 0 = off, 3 = always
    const int64_t rows_b = g.rows_hint > 0 ? std::min<int64_t>(g.rows_hint, g.cap) : g.cap;
    const int NT16 = (g.d + 15) / 16;
    if (force_nw == 0 && d16_knob && (d16_knob == 3 || gru_d16_fits(g.cap, g.rows_hint, g.d))) {
      a.tail_blocks = 0;
      // (the sampler riders of the collate prefetch were tried here too - the sampler reads the graph only - and cost the
      // updater more than they saved the query-row launch: C2 updater +4.6 us, launch behind it -0.7 us; C4 +22 us)
      const dim3 grid16((unsigned)std::min<int64_t>(256, 8 * cdiv(cdiv(g.cap, 16) * NT16, 8)));
      const bool rt3 = cdiv(rows_b, 48) * NT16 <= 256;
      if (g.w_blend && rt3) TG_KLAUNCH((k_gru_direct16<3, true>), grid16, dim3(256), 0, st, a);
      else if (g.w_blend) TG_KLAUNCH((k_gru_direct16<GRU16_RT_MAX, true>), grid16, dim3(256), 0, st, a);
      else if (rt3) TG_KLAUNCH(k_gru_direct16<3>, grid16, dim3(256), 0, st, a);
      else TG_KLAUNCH(k_gru_direct16<GRU16_RT_MAX>, grid16, dim3(256), 0, st, a);
      static_assert(GRU16_RT_MAX == 6, "the form names below spell the instance out");
      TG_GRU_FORM(g.w_blend ? (rt3 ? "direct16<3,blend>" : "direct16<6,blend>") : (rt3 ? "direct16<3>" : "direct16<6>"));
      return check_launch("gru(16 x 16)");
    }
  }
  if (force_nw == 1 || (force_nw == 0 && micro && micro_knob)) {
    a.tail_blocks = 0;
    static const int direct_knob = env_int("TG_GRU_DIRECT", 1);  // tuning knob: 0 = LDS-staged
    const dim3 grid32((unsigned)(8 * cdiv(cdiv(g.cap, 32), 8) * NT));
    if (direct_knob) TG_KLAUNCH(k_gru_direct, grid32, dim3(256), 0, st, a);
    else TG_KLAUNCH((k_gru<1, 4>), grid32, dim3(256), 0, st, a);
    TG_GRU_FORM(direct_knob ? "direct" : "gru<1,4>");
    return check_launch("gru(32)");
  }
  if (force_nw == 2 || (force_nw == 0 && tiny)) {
    a.tail_blocks = 0;
    TG_KLAUNCH((k_gru<2, 4>), dim3((unsigned)(8 * cdiv(cdiv(g.cap, 64), 8) * NT)), dim3(512), 0, st, a);
    TG_GRU_FORM("gru<2,4>");
    return check_launch("gru(64)");
  }
  if (force_nw == 3 || (force_nw == 0 && small)) {
    const int tail = g.d % 32;
    const bool use_tail = tail > 0 && tail <= 16;  // the partial column tile as 16-column blocks of T16_ROWS rows
    a.tail_blocks = use_tail ? (int)cdiv(g.cap, T16_ROWS) : 0;
    const int ntm = NT - (use_tail ? 1 : 0);
    // per XCD: its row tiles x column tiles, then at most NT + ceil(tails / 8) + 1 tail slots (see the kernel's map)
    const int64_t per_xcd = cdiv(cdiv(g.cap, 96), 8) * ntm + (use_tail ? ntm + cdiv(a.tail_blocks, 8) + 1 : 0);
    TG_KLAUNCH((k_gru<3, 4>), dim3((unsigned)(8 * per_xcd)), dim3(768), 0, st, a);
    TG_GRU_FORM(use_tail ? "gru<3,4,tail16>" : "gru<3,4>");
    return check_launch("gru(96)");
  }
  // 128-row blocks.  More blocks than CUs: four wavefronts per block and TWO blocks per CU (k_gru<4, 1>: 58 KB of LDS - the
  // old-memory tile of the epilogue lives in registers - and at most 256 registers), so that one block's prologue (first
  // tiles exposed) and epilogue (gates, scattered stores) run under the other's k-loop, and there is no k-group fold.
  // Measured against the eight-wavefront blocks (k_gru<4, 2>, one per CU), rows x message width -> d:
  // 65 536 x 1 024 -> 256 1 200 -> 1 073 us (120 TF/s); 49 152 x 688 -> 172 485 -> 435 us; 8 192 x 1 024 -> 256 152 -> 140 us;
  // a launch of at most one block per CU keeps the eight wavefronts (4 096 x 1 024 -> 256: 77 against 81 us).
  const int64_t grid = 8 * cdiv(cdiv(g.cap, 128), 8) * NT;
  const int64_t live = g.rows_hint > 0 ? cdiv(std::min<int64_t>(g.rows_hint, g.cap), 128) * NT : grid;
  // (the caller's row bound carries a margin - 1.5 x the rows seen: between one and 1.25 blocks per CU by that bound the launch
  // usually fits one round, where the eight wavefronts are ahead: 5 000 x 688 -> 172 61.6 against 64.2 us)
  if (ks_knob == 2 || (ks_knob == 0 && live <= (g.rows_hint > 0 ? 320 : 256))) {
    TG_KLAUNCH((k_gru<4, 2>), dim3((unsigned)grid), dim3(512), 0, st, a);
    TG_GRU_FORM("gru<4,2>");
  } else {
    TG_KLAUNCH((k_gru<4, 1>), dim3((unsigned)grid), dim3(256), 0, st, a);
    TG_GRU_FORM("gru<4,1>");
  }
  return check_launch("gru");
}

}  // namespace tg

// diagnostic: one cell straight through gru_launch with every GruArgs field a caller can set, and which kernel it picked.
// Every argument check runs before anything touches the GPU.
extern "C" int tg_debug_gru(const tg_gru_probe* p, const char** form_out, void* stream) {
  using namespace tg;
  if (form_out) *form_out = nullptr;
  if (!p || !p->x || !p->h || !p->w_ih || !p->w_hh || !p->b_ih || !p->b_hh || !p->out) return TG_EINVAL;
  if (p->cap < 0 || p->rows_hint < 0) return TG_EINVAL;
  if (p->d <= 0 || (p->d % 4) || p->xw <= 0 || (p->xw % 4)) return TG_EINVAL;
  if (p->x_w != p->xw || p->h_w != p->d) return TG_EINVAL;
  if (p->x_ld < p->xw || (p->x_ld % 4) || p->h_ld < p->d || (p->h_ld % 4) || p->ldo < p->d) return TG_EINVAL;
  // the skipped run lies inside the whole k-tiles of the message and leaves a message column to multiply
  if (p->x_skip_at < 0 || p->x_skip_n < 0) return TG_EINVAL;
  if (p->x_skip_n > 0 && ((int64_t)(p->x_skip_at + p->x_skip_n) * BK > p->xw || (int64_t)p->x_skip_n * BK >= p->xw)) return TG_EINVAL;
  if ((p->out2_by_row || p->add2) && !p->out2) return TG_EINVAL;
  GruArgs g{};
  g.cap = p->cap; g.n_dev = p->n_dev; g.d = p->d; g.xw = p->xw;
  g.x = ASeg{p->x, p->x_ld, p->x_w, p->x_idx};
  g.h = ASeg{p->h, p->h_ld, p->h_w, p->h_idx};
  g.w_ih = p->w_ih; g.w_hh = p->w_hh; g.b_ih = p->b_ih; g.b_hh = p->b_hh;
  g.out = p->out; g.ldo = p->ldo; g.out_rows = p->out_rows; g.gates = p->gates;
  g.out2 = p->out2; g.add2 = p->add2; g.out2_by_row = p->out2_by_row ? 1 : 0;
  g.rows_hint = p->rows_hint; g.x_skip_at = p->x_skip_at; g.x_skip_n = p->x_skip_n;
  g.w_blend = p->w_blend; g.b_blend = p->b_blend;
  t_gru_form = nullptr;
  const int rc = gru_launch(g, as_stream(stream));
  if (form_out) *form_out = t_gru_form;
  return rc;
}
