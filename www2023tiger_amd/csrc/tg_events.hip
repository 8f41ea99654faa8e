// Event keys: external 64-bit event keys -> rows of the edge-feature table (idempotent ingestion, retraction by key;
// tiger_hip.h: tg_events_*; DESIGN 7.24.  The reference names an event by its row in the data set and has no counterpart).
// The persistent table IS a tg_idmap (tg_idmap.h: slot_key / slot_id / key_of, dense id = edge row); it is written by
// tg_idmap_assign (commit) and tg_idmap_rebuild / _rebuild_free (growth, loading, after a release) alone.
//
// screen: what of a batch is new, without touching the map.  Equivalent to
//     d = the map; kept = []
//     for i, k in enumerate(keys):
//         if k not in d: d[k] = rows + len(kept); kept.append(i)
//         eid_out[i] = d[k]
// with d thrown away.  A key the persistent table holds is answered by a read-only probe (im_find; plain loads, no atomics).
// The others meet in a SCRATCH open-addressing table of this call - scap = the power of two >= max(2 n, 16) slots, the same
// home slot idmap_mix(key) & (scap - 1) and linear probing: skey (INT64_MIN = empty) is claimed by a 64-bit compare-and-swap
// and spos takes atomicMin(position), so after the pass a slot names the SMALLEST position that holds its key (the idiom of
// k_idmap_claim).  Then, as in tg_idmap.hip: the flag "position i is the first occurrence of an unknown key" leaves as
// ballot words over tiles of 2048, the tiles' counts are scanned (256 tiles per workgroup, block_sum_front for the chunks
// in front), and a position's row is rows + base[tile of w] + popcount of the flags in front of w, w its key's winner; a
// winner also writes its position to keep_out[rank] - ascending, because the rank is.
// Launches (n > TG_EVENTS_ONE_MAX), each reading what the previous one wrote - no kernel waits for another workgroup:
//   find   clears the scratch table (in the workspace) and probes the persistent table: eid_out of a known key, states
//   claim  the unknown keys claim their scratch slots
//   flags, bases, write   as above; the owner of base[n_tile] writes out2 = {kept, error bits}: the call's ONE read-back
// n <= TG_EVENTS_ONE_MAX: one workgroup, one launch, the scratch table in LDS, the phases separated by barriers; position i
// belongs to thread i % 256 in every phase, so slot[i] / wpos[i] are written and read by the same thread.
// Every probe loop ends after the table's capacity (TG_IDMAP_ERR_PROBE); 2 n <= scap, so the scratch bound is never met.
// A slot_id becomes a row only if it lies in [1, rows), a scratch slot and a winner position index only after their range
// checks (TG_IDMAP_ERR_TABLE).  INT64_MIN in keys[] is no key: TG_EVENTS_ERR_KEY, eid_out = -1, never probed.
// Workspace: 4 B n (slots) + 4 B n (winners) + 8 B * 32 n_tile (flag words) + 3 * 4 B n_tile (counts, error bits, bases),
// and for n > TG_EVENTS_ONE_MAX 12 B * scap (scratch), each part rounded up to 16 bytes.
//
// repack: follows a release of edge rows (tg_edge_rows.hip: remap, monotone).  One launch, one thread per OLD row:
// key_of_new[remap[r]] = key_of_old[r] - a wavefront's stores ascend.  The keyless bitmap (bit r set <=> row r holds no
// key: a row the model was built with) is rebuilt a word at a time by ballot-style assembly over the NEW rows: the
// wavefront that holds the old row of new row 64 w owns word w; it walks the old rows from there, 64 at a time, until the
// word's 64 new rows are passed, ORs the bits (shifted to their new place) and stores the word.  A range of <= 64 new rows
// holds at most one multiple of 64, so every word has one owner: no atomics, nothing read back.  The walk is as long as
// the released run it crosses (rows_before / 64 steps at most).
#include <algorithm>
#include <vector>

#include "tg_tcsr.h"
#include "tg_step.h"
#include "tg_idmap.h"

namespace tg {

// Batches up to here run in one workgroup of one launch.  NOT MEASURED: 256 is TG_IDMAP_ONE_MAX's measured value
// (profiles/idmap_one_max_v1.json), taken over for a kernel with the same structure; tools/events_bench.py is the
// measurement to run.  (Diagnostic builds: make EXTRA=-DTG_EVENTS_ONE_MAX=N, 0 <= N <= 2048.)
#ifndef TG_EVENTS_ONE_MAX
#define TG_EVENTS_ONE_MAX 256
#endif
constexpr int EV_ONE_MAX = TG_EVENTS_ONE_MAX;
static_assert(EV_ONE_MAX >= 0 && EV_ONE_MAX <= IM_TILE, "the one-workgroup form covers one tile");
constexpr int64_t ev_pow2_at_least(int64_t x) {
  int64_t c = 16;
  while (c < x) c <<= 1;
  return c;
}
constexpr int EV_ONE_CAP = (int)ev_pow2_at_least(2 * (int64_t)EV_ONE_MAX);  // LDS scratch slots: 12 B each, <= 48 KiB
constexpr int32_t EV_NOPOS = INT32_MAX;                                     // spos of a slot nobody claimed
// wpos[i] of a position that waits for no rank: done, or why it failed
constexpr int32_t EV_DONE = -1, EV_BAD_PROBE = -2, EV_BAD_TABLE = -3, EV_BAD_KEY = -4;

struct EventsArgs {
  tg_idmap m;
  int64_t rows, n, n_tile;
  const int64_t* keys;
  int32_t* eid_out;
  int64_t* keep_out;
  int64_t* out2;
  uint32_t* slot;   // [n] the scratch slot of a position that waits for its rank
  int32_t* wpos;    // [n] the smallest position with the same key, or EV_DONE / EV_BAD_*
  uint64_t* words;  // [n_tile * IM_WORDS]
  uint32_t *cnt, *errs, *base;  // [n_tile], [n_tile], [n_tile + 1]
};

__device__ __forceinline__ void ev_clear(int64_t* skey, int32_t* spos, int64_t scap, int64_t first, int64_t step) {
  for (int64_t s = first; s < scap; s += step) {
    skey[s] = IM_EMPTY;
    spos[s] = EV_NOPOS;
  }
}

// positions first, first + step, ... < a.n: the persistent table, read-only
__device__ __forceinline__ void ev_find_pass(const EventsArgs& a, int64_t first, int64_t step) {
  for (int64_t i = first; i < a.n; i += step) {
    const int64_t key = a.keys[i];
    int32_t state = 0, eid = -1;  // (pending: the claim pass goes on)
    if (key == IM_EMPTY) {
      state = EV_BAD_KEY;
    } else {
      const int64_t s = im_find(a.m, key);
      if (s == -2) state = EV_BAD_PROBE;
      if (s >= 0) {
        const int32_t v = a.m.slot_id[s];  // >= 1: the key's row; below: a slot that holds no row - the key is unknown
        if (v >= 1) {
          state = v < a.rows ? EV_DONE : EV_BAD_TABLE;
          if (v < a.rows) eid = v;
        }
      }
    }
    a.wpos[i] = state;
    if (state < 0) a.eid_out[i] = eid;
  }
}

// the scratch slot that holds `key` once this returns - found, or claimed from the empty slots -, or -2
__device__ __forceinline__ int64_t ev_claim(int64_t* skey, int64_t scap, int64_t key) {
  const uint64_t mask = (uint64_t)scap - 1;
  uint64_t s = idmap_mix(key) & mask;
  for (int64_t j = 0; j < scap; ++j, s = (s + 1) & mask) {
    int64_t k = im_ld(skey + s);
    if (k == IM_EMPTY) {  // (a slot never becomes empty again inside a call)
      k = (int64_t)atomicCAS(reinterpret_cast<unsigned long long*>(skey + s), (unsigned long long)IM_EMPTY,
                             (unsigned long long)key);
      if (k == IM_EMPTY) return (int64_t)s;
    }
    if (k == key) return (int64_t)s;
  }
  return -2;
}

__device__ __forceinline__ void ev_claim_pass(const EventsArgs& a, int64_t* skey, int32_t* spos, int64_t scap, int64_t first,
                                              int64_t step) {
  for (int64_t i = first; i < a.n; i += step) {
    if (a.wpos[i] != 0) continue;
    const int64_t s = ev_claim(skey, scap, a.keys[i]);
    if (s < 0) {
      a.wpos[i] = EV_BAD_PROBE;
      a.eid_out[i] = -1;
    } else {
      atomicMin(spos + s, (int32_t)i);
      a.slot[i] = (uint32_t)s;
    }
  }
}

// one workgroup: tile `tile`
__device__ __forceinline__ void ev_flag_tile(const EventsArgs& a, const int32_t* spos, int64_t scap, int64_t tile,
                                             uint32_t* s_cnt /*[IM_WAVES + 1]*/) {
  const uint32_t t = threadIdx.x, lane = t & (TG_WAVE - 1), wv = t / TG_WAVE;
  const int64_t p0 = tile * IM_TILE;
  if (t == 0) s_cnt[IM_WAVES] = 0;
  __syncthreads();
  uint32_t firsts = 0, err = 0;  // (firsts: the same value on every lane of a wavefront)
#pragma unroll
  for (int i = 0; i < IM_ITEMS; ++i) {
    const int64_t p = p0 + (int64_t)i * IM_THREADS + t;
    bool first = false;
    if (p < a.n) {
      const int32_t st = a.wpos[p];
      if (st == EV_BAD_PROBE) err |= TG_IDMAP_ERR_PROBE;
      if (st == EV_BAD_TABLE) err |= TG_IDMAP_ERR_TABLE;
      if (st == EV_BAD_KEY) err |= TG_EVENTS_ERR_KEY;
      if (st >= 0) {
        const uint32_t sl = a.slot[p];
        const int64_t w = (int64_t)sl < scap ? (int64_t)im_ld(spos + sl) : -1;
        if (w < 0 || w > p) {  // (the slot names no position of this call at or in front of p)
          err |= TG_IDMAP_ERR_TABLE;
          a.wpos[p] = EV_BAD_TABLE;
          a.eid_out[p] = -1;
        } else {
          a.wpos[p] = (int32_t)w;
          first = w == p;
        }
      }
    }
    const uint64_t word = __ballot(first);  // bit l: position p0 + 256 i + 64 wv + l
    if (lane == 0) a.words[tile * IM_WORDS + i * IM_WAVES + wv] = word;
    firsts += (uint32_t)__popcll(word);
  }
  if (lane == 0) s_cnt[wv] = firsts;
  if (err) atomicOr(&s_cnt[IM_WAVES], err);
  __syncthreads();
  if (t == 0) {
    uint32_t c = 0;
#pragma unroll
    for (int w = 0; w < IM_WAVES; ++w) c += s_cnt[w];
    a.cnt[tile] = c;
    a.errs[tile] = s_cnt[IM_WAVES];
  }
}

// one workgroup: slots [256 b, 256 b + 256) of base[0 .. n_tile]; the owner of base[n_tile] also writes out2
__device__ __forceinline__ void ev_bases_chunk(const EventsArgs& a, int64_t b, uint32_t* s_w /*[IM_WAVES + 1]*/) {
  const int64_t s0 = b * IM_THREADS;
  const uint32_t front = block_sum_front(a.cnt, (uint32_t)s0, s_w);  // (s0 <= n_tile < 2^21)
  const int64_t s = s0 + threadIdx.x;
  uint32_t total;
  const uint32_t r = block_excl_scan(s < a.n_tile ? a.cnt[s] : 0u, s_w, &total);
  if (s <= a.n_tile) a.base[s] = front + r;
  if (b != a.n_tile / IM_THREADS) return;  // (block-uniform)
  uint32_t err = 0;
  for (int64_t i = threadIdx.x; i < a.n_tile; i += IM_THREADS) err |= a.errs[i];
  if (threadIdx.x == 0) s_w[IM_WAVES] = 0;
  __syncthreads();
  if (err) atomicOr(&s_w[IM_WAVES], err);
  __syncthreads();
  if (s == a.n_tile) {
    a.out2[0] = (int64_t)(front + r);
    a.out2[1] = (int64_t)s_w[IM_WAVES];
  }
}

// first occurrences of unknown keys in front of position w
__device__ __forceinline__ uint32_t ev_rank(const EventsArgs& a, int64_t w) {
  const int64_t tile = w / IM_TILE;
  const uint32_t off = (uint32_t)(w % IM_TILE);
  // offset 256 i + 64 wv + l is bit l of word 4 i + wv = off / 64: the words are in position order
  const uint32_t full = off / 64, part = off % 64;
  const uint64_t* __restrict__ wd = a.words + tile * IM_WORDS;
  uint32_t r = a.base[tile];
  for (uint32_t j = 0; j < full; ++j) r += (uint32_t)__popcll(wd[j]);
  return r + (uint32_t)__popcll(wd[full] & ((1ull << part) - 1ull));
}

__device__ __forceinline__ void ev_write_pass(const EventsArgs& a, int64_t first, int64_t step) {
  for (int64_t i = first; i < a.n; i += step) {
    const int64_t w = a.wpos[i];
    if (w < 0) continue;
    const int64_t r = (int64_t)ev_rank(a, w);
    if (r >= a.n) continue;  // (the entry checked rows + n <= 2^31 - 1: a workspace that is no plan of this call)
    a.eid_out[i] = (int32_t)(a.rows + r);
    if (w == i) a.keep_out[r] = i;
  }
}

__global__ void __launch_bounds__(IM_THREADS) k_events_find(EventsArgs a, int64_t* skey, int32_t* spos, int64_t scap) {
  const int64_t first = (int64_t)blockIdx.x * IM_THREADS + threadIdx.x, step = (int64_t)gridDim.x * IM_THREADS;
  ev_clear(skey, spos, scap, first, step);
  ev_find_pass(a, first, step);
}
__global__ void __launch_bounds__(IM_THREADS) k_events_claim(EventsArgs a, int64_t* skey, int32_t* spos, int64_t scap) {
  ev_claim_pass(a, skey, spos, scap, (int64_t)blockIdx.x * IM_THREADS + threadIdx.x, (int64_t)gridDim.x * IM_THREADS);
}
__global__ void __launch_bounds__(IM_THREADS) k_events_flags(EventsArgs a, const int32_t* spos, int64_t scap) {
  __shared__ uint32_t s_cnt[IM_WAVES + 1];
  ev_flag_tile(a, spos, scap, (int64_t)blockIdx.x, s_cnt);
}
__global__ void __launch_bounds__(IM_THREADS) k_events_bases(EventsArgs a) {
  __shared__ uint32_t s_w[IM_WAVES + 1];
  ev_bases_chunk(a, (int64_t)blockIdx.x, s_w);
}
__global__ void __launch_bounds__(IM_THREADS) k_events_write(EventsArgs a) {
  ev_write_pass(a, (int64_t)blockIdx.x * IM_THREADS + threadIdx.x, (int64_t)gridDim.x * IM_THREADS);
}
// n <= EV_ONE_MAX: the phases in one workgroup, the scratch table in LDS.  What crosses threads goes through LDS (the
// scratch table: atomics and L1-bypassing loads) or through the workspace with plain stores and loads of one workgroup (the
// flag words, the count, the bases), both ordered by the barriers.
__global__ void __launch_bounds__(IM_THREADS) k_events_screen_one(EventsArgs a) {
  __shared__ int64_t s_key[EV_ONE_CAP];
  __shared__ int32_t s_pos[EV_ONE_CAP];
  __shared__ uint32_t s_w[IM_WAVES + 1];
  ev_clear(s_key, s_pos, EV_ONE_CAP, threadIdx.x, IM_THREADS);
  ev_find_pass(a, threadIdx.x, IM_THREADS);
  __syncthreads();
  ev_claim_pass(a, s_key, s_pos, EV_ONE_CAP, threadIdx.x, IM_THREADS);
  __syncthreads();
  if (a.n_tile) ev_flag_tile(a, s_pos, EV_ONE_CAP, 0, s_w);
  __syncthreads();
  ev_bases_chunk(a, 0, s_w);
  __syncthreads();
  ev_write_pass(a, threadIdx.x, IM_THREADS);
}

__device__ __forceinline__ uint64_t wave_or64(uint64_t v) {
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
  for (int d = TG_WAVE / 2; d >= 1; d >>= 1) {
    lo |= (uint32_t)__shfl_xor((int)lo, d);
    hi |= (uint32_t)__shfl_xor((int)hi, d);
  }
  return ((uint64_t)hi << 32) | lo;
}

// one thread per old row; a wavefront = 64 consecutive old rows
__global__ void __launch_bounds__(IM_THREADS) k_events_repack(const int64_t* __restrict__ key_of_old,
                                                              const uint64_t* __restrict__ keyless_old,
                                                              const int32_t* __restrict__ remap, int64_t rows_before,
                                                              int64_t* __restrict__ key_of_new, uint64_t* __restrict__ keyless_new,
                                                              int64_t rows_new) {
  const int lane = lane_id();
  const int64_t r = (int64_t)blockIdx.x * IM_THREADS + threadIdx.x;
  const int64_t v = r < rows_before ? (int64_t)remap[r] : -1;
  const bool kept = v >= 0 && v < rows_new;  // (a remap that names no new row moves nothing)
  if (kept) key_of_new[v] = key_of_old[r];
  uint64_t owners = __ballot(kept && (v & 63) == 0);  // (the same on every lane: the loops below are wave-uniform)
  while (owners) {
    const int src = __ffsll((unsigned long long)owners) - 1;
    owners &= owners - 1;
    const int64_t w0 = ((int64_t)(uint32_t)__shfl((int)v, src));  // new row 64 w: the first of the word
    uint64_t acc = 0;
    for (int64_t q = r + src; q - lane < rows_before; q += TG_WAVE) {  // q: this lane's old row; lane 0 starts at the owner's
      const int64_t vv = q < rows_before ? (int64_t)remap[q] : -1;
      if (vv >= w0 && vv < w0 + 64 && vv < rows_new && ((keyless_old[q >> 6] >> (q & 63)) & 1ull)) acc |= 1ull << (vv - w0);
      if (__ballot(vv >= w0 + 64)) break;  // (remap is monotone: nothing of the word lies beyond)
    }
    acc = wave_or64(acc);
    if (lane == 0) keyless_new[w0 >> 6] = acc;
  }
}

struct EventsLayout {
  int64_t n_tile, scap;
  size_t slot, wpos, words, cnt, errs, base, skey, spos, total;
};
static EventsLayout events_layout(int64_t n) {
  EventsLayout l{};
  l.n_tile = cdiv(n, IM_TILE);
  l.scap = n <= EV_ONE_MAX ? 0 : ev_pow2_at_least(2 * n);
  l.slot = 0;
  l.wpos = l.slot + align16((size_t)n * sizeof(uint32_t));
  l.words = l.wpos + align16((size_t)n * sizeof(int32_t));
  l.cnt = l.words + align16((size_t)l.n_tile * IM_WORDS * sizeof(uint64_t));
  l.errs = l.cnt + align16((size_t)l.n_tile * sizeof(uint32_t));
  l.base = l.errs + align16((size_t)l.n_tile * sizeof(uint32_t));
  l.skey = l.base + align16((size_t)(l.n_tile + 1) * sizeof(uint32_t));
  l.spos = l.skey + align16((size_t)l.scap * sizeof(int64_t));
  l.total = l.spos + align16((size_t)l.scap * sizeof(int32_t));
  return l;
}

static int events_screen_args(const tg_idmap* m, int64_t rows, const int64_t* keys, int64_t n, const int32_t* eid_out,
                              const int64_t* keep_out, const int64_t* out2) {
  if (int rc = idmap_struct_ok(m)) return rc;
  if (rows < 1 || n < 0 || rows > 0x7fffffffLL || n > 0x7fffffffLL - rows || rows > m->key_rows) return TG_EINVAL;
  if (!out2 || (n > 0 && (!keys || !eid_out || !keep_out))) return TG_EINVAL;
  return TG_OK;
}

static int events_repack_args(const int64_t* key_of_old, const uint64_t* keyless_old, const int32_t* remap, int64_t rows_before,
                              const int64_t* key_of_new, const uint64_t* keyless_new, int64_t rows_new) {
  if (!key_of_old || !keyless_old || !remap || !key_of_new || !keyless_new) return TG_EINVAL;
  if (rows_before < 1 || rows_before > 0x7fffffffLL || rows_new < 1 || rows_new > rows_before) return TG_EINVAL;
  return TG_OK;
}

}  // namespace tg

using namespace tg;

extern "C" size_t tg_events_screen_workspace_bytes(int64_t n) {
  if (n < 0 || n > 0x7fffffffLL) return 0;
  return events_layout(n).total;
}

extern "C" int tg_events_screen(const tg_idmap* map, int64_t rows, const int64_t* keys, int64_t n, int32_t* eid_out,
                                int64_t* keep_out, int64_t* out2, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = events_screen_args(map, rows, keys, n, eid_out, keep_out, out2)) return rc;
  const EventsLayout l = events_layout(n);
  if (int rc = ws_check(ws, ws_bytes, l.total)) return rc;  // before the first launch
  char* b = static_cast<char*>(ws);
  EventsArgs a{*map, rows, n, l.n_tile, keys, eid_out, keep_out, out2,
               reinterpret_cast<uint32_t*>(b + l.slot), reinterpret_cast<int32_t*>(b + l.wpos),
               reinterpret_cast<uint64_t*>(b + l.words), reinterpret_cast<uint32_t*>(b + l.cnt),
               reinterpret_cast<uint32_t*>(b + l.errs), reinterpret_cast<uint32_t*>(b + l.base)};
  hipStream_t st = as_stream(stream);
  if (n <= EV_ONE_MAX) {
    hipLaunchKernelGGL(k_events_screen_one, dim3(1), dim3(IM_THREADS), 0, st, a);
    return check_launch("tg_events_screen");
  }
  int64_t* skey = reinterpret_cast<int64_t*>(b + l.skey);
  int32_t* spos = reinterpret_cast<int32_t*>(b + l.spos);
  const unsigned flat = (unsigned)cdiv(n, IM_THREADS);
  hipLaunchKernelGGL(k_events_find, dim3(flat_grid(l.scap, IM_THREADS)), dim3(IM_THREADS), 0, st, a, skey, spos, l.scap);
  hipLaunchKernelGGL(k_events_claim, dim3(flat), dim3(IM_THREADS), 0, st, a, skey, spos, l.scap);
  hipLaunchKernelGGL(k_events_flags, dim3((unsigned)l.n_tile), dim3(IM_THREADS), 0, st, a, spos, l.scap);
  hipLaunchKernelGGL(k_events_bases, dim3((unsigned)cdiv(l.n_tile + 1, IM_THREADS)), dim3(IM_THREADS), 0, st, a);
  hipLaunchKernelGGL(k_events_write, dim3(flat), dim3(IM_THREADS), 0, st, a);
  return check_launch("tg_events_screen");
}

extern "C" int tg_events_repack(const int64_t* key_of_old, const uint64_t* keyless_old, const int32_t* remap,
                                int64_t rows_before, int64_t* key_of_new, uint64_t* keyless_new, int64_t rows_new,
                                void* stream) {
  if (int rc = events_repack_args(key_of_old, keyless_old, remap, rows_before, key_of_new, keyless_new, rows_new)) return rc;
  hipLaunchKernelGGL(k_events_repack, dim3((unsigned)cdiv(rows_before, IM_THREADS)), dim3(IM_THREADS), 0, as_stream(stream),
                     key_of_old, keyless_old, remap, rows_before, key_of_new, keyless_new, rows_new);
  return check_launch("tg_events_repack");
}

// The host twins: plain C++ over host pointers (those of `map` included), one key after the other.
extern "C" int tg_events_screen_host(const tg_idmap* map, int64_t rows, const int64_t* keys, int64_t n, int32_t* eid_out,
                                     int64_t* keep_out, int64_t* out2) {
  if (int rc = events_screen_args(map, rows, keys, n, eid_out, keep_out, out2)) return rc;
  const int64_t scap = ev_pow2_at_least(2 * n);
  const uint64_t mask = (uint64_t)scap - 1;
  std::vector<int64_t> skey((size_t)scap, IM_EMPTY);
  std::vector<int32_t> srow((size_t)scap, -1);
  int64_t err = 0, kept = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t key = keys[i];
    eid_out[i] = -1;
    if (key == IM_EMPTY) {
      err |= TG_EVENTS_ERR_KEY;
      continue;
    }
    bool found = false;
    const int64_t s = host_probe(map, key, &found);
    if (s < 0) {
      err |= TG_IDMAP_ERR_PROBE;
      continue;
    }
    if (found && map->slot_id[s] >= 1) {
      if (map->slot_id[s] < rows) eid_out[i] = map->slot_id[s];
      else err |= TG_IDMAP_ERR_TABLE;
      continue;
    }
    uint64_t q = idmap_mix(key) & mask;  // (2 n <= scap: an empty slot is always met)
    while (skey[q] != key && skey[q] != IM_EMPTY) q = (q + 1) & mask;
    if (skey[q] == IM_EMPTY) {
      skey[q] = key;
      srow[q] = (int32_t)(rows + kept);
      keep_out[kept++] = i;
    }
    eid_out[i] = srow[q];
  }
  out2[0] = kept;
  out2[1] = err;
  return TG_OK;
}

extern "C" int tg_events_repack_host(const int64_t* key_of_old, const uint64_t* keyless_old, const int32_t* remap,
                                     int64_t rows_before, int64_t* key_of_new, uint64_t* keyless_new, int64_t rows_new) {
  if (int rc = events_repack_args(key_of_old, keyless_old, remap, rows_before, key_of_new, keyless_new, rows_new)) return rc;
  for (int64_t w = 0; w < cdiv(rows_new, 64); ++w) keyless_new[w] = 0;
  for (int64_t r = 0; r < rows_before; ++r) {
    const int64_t v = remap[r];
    if (v < 0 || v >= rows_new) continue;
    key_of_new[v] = key_of_old[r];
    if ((keyless_old[r >> 6] >> (r & 63)) & 1ull) keyless_new[v >> 6] |= 1ull << (v & 63);
  }
  return TG_OK;
}
