// The device id map: external 64-bit keys -> dense int32 node ids (online serving behind account numbers or hashes; the
// reference numbers its nodes offline, in its preprocessing script, and has no counterpart of this).
//
// Layout (tiger_hip.h: tg_idmap).  An open-addressing table with linear probing: slot_key int64 [capacity] (TG_IDMAP_EMPTY
// = INT64_MIN marks an empty slot), slot_id int32 [capacity] (-1 in an empty slot, the key's dense id >= 1 otherwise), and
// the reverse table key_of int64 [key_rows] (dense id -> key; key_of[0] = INT64_MIN: the key of the padding id 0, which is
// never inserted - looking it up or assigning it gives id 0).  capacity is a power of two; the home slot of a key is
// idmap_mix(key) & (capacity - 1) (the splitmix64 step: tiger_hip.h).  The MAPPING never depends on the hash or on who wins
// a slot; only where a key sits in the table does.
//
// assign: a key the map does not hold gets size + r, r = the rank of its FIRST occurrence in keys[] among the first
// occurrences of all such keys - what `for x in keys: d.setdefault(x, len(d))` gives.  Dependent launches; a value another
// workgroup writes is never waited for inside a kernel, it is read by the NEXT launch:
//   claim  (one thread per position i): probe from the home slot.  An empty slot is claimed by a 64-bit compare-and-swap on
//           slot_key; a loser that reads back its own key has found the slot like the winner.  A slot with id >= 1 is a key
//           from before the call: ids_out[i] is that id, the position is done.  Otherwise the slot belongs to this call:
//           atomicMin(slot_id, INT32_MIN + i) - empty is -1, every pending value is below it, settled ids are above - so
//           after the launch the slot names the SMALLEST position that holds its key.  slot[i] goes to the workspace.
//   flags  (one workgroup per tile of 2048 positions): w = the slot's smallest position -> wpos[i]; the flag "i is the
//           first occurrence of a new key" (w == i) leaves as ballot words in position order, one count per tile, and the
//           tile's error bits.
//   bases  (one workgroup per 256 tiles): base[s] = new keys in front of tile s (block_sum_front + block scan, as
//           tg_erase.hip); the workgroup that owns base[n_tile] writes out2 = {size + total, OR of the error bits}.
//   write  (one thread per position): id = size + base[tile of w] + popcount of the flags in front of w; ids_out[i] = id;
//           the first occurrence also settles slot_id and writes key_of[id].
// n <= 256 (one key per thread): the four phases run in ONE workgroup of one launch, separated by workgroup barriers.
// Every probe loop runs at most `capacity` steps and then raises TG_IDMAP_ERR_PROBE; the C entry refuses
// 2 (size + n) > capacity, so a well-formed table is never more than half full and the bound is not met.
// Values loaded from the table become addresses only after a range check (a slot_id that is neither an id below `size`
// nor a position of this call raises TG_IDMAP_ERR_TABLE and is not used).
// Workspace: 4 B * n (slots) + 4 B * n (winning positions) + 8 B * 32 * n_tile (flag words) + 4 B * n_tile (counts) +
// 4 B * n_tile (error bits) + 4 B * (n_tile + 1) (bases), each part rounded up to 16 bytes; n_tile = ceil(n / 2048).
//
// rebuild: fills an EMPTY table from key_of[1 .. size) - growth, loading.  Launch A claims like `claim` with the ROW in
// place of the position; launch B looks every row's key up again: the slot names the smallest row with that key, and a
// row that is not that one repeats the key of an earlier row (TG_IDMAP_ERR_DUP).  The error word is folded with atomicMax
// over ((0x7fffffff - row) << 8 | class): the SMALLEST offending row and its class, whatever the launch geometry.
#include <algorithm>

#include "tg_tcsr.h"
#include "tg_step.h"

namespace tg {

constexpr int IM_THREADS = TG_SCAN_BLOCK;  // block_excl_scan: 256
constexpr int IM_ITEMS = 8;
constexpr int IM_TILE = IM_THREADS * IM_ITEMS;  // positions per workgroup
constexpr int IM_WORDS = IM_TILE / 64;          // flag words per tile
constexpr int IM_WAVES = IM_THREADS / TG_WAVE;
// Batches up to here run in one workgroup of one launch: one key per thread.  Measured (profiles/idmap_one_max_v1.json,
// DESIGN 7.18): at 256 keys the one launch is the faster form; at 2 048 - eight keys per thread, each a chain of dependent
// atomics - the four launches are.  (Diagnostic builds: make EXTRA=-DTG_IDMAP_ONE_MAX=N, 0 <= N <= 2048.)
#ifndef TG_IDMAP_ONE_MAX
#define TG_IDMAP_ONE_MAX 256
#endif
constexpr int IM_ONE_MAX = TG_IDMAP_ONE_MAX;
static_assert(IM_ONE_MAX >= 0 && IM_ONE_MAX <= IM_TILE, "the one-workgroup form covers one tile");
constexpr int64_t IM_EMPTY = TG_IDMAP_EMPTY;
constexpr int32_t IM_PENDING = INT32_MIN;  // slot_id of a slot claimed in this call: IM_PENDING + smallest position
// wpos[i] of a position that waits for no rank: done, or why it failed
constexpr int32_t IM_DONE = -1, IM_BAD_PROBE = -2, IM_BAD_TABLE = -3;

__host__ __device__ __forceinline__ uint64_t idmap_mix(int64_t key) {
  uint64_t z = (uint64_t)key + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// table words other workgroups change while this kernel runs: read past the vector L1
__device__ __forceinline__ int64_t im_ld(const int64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int32_t im_ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the slot that holds `key`, or -1 (an empty slot comes first: the map does not hold it), or -2 (capacity slots probed)
__device__ __forceinline__ int64_t im_find(const tg_idmap& m, int64_t key) {
  const uint64_t mask = (uint64_t)m.capacity - 1;
  uint64_t s = idmap_mix(key) & mask;
  for (int64_t j = 0; j < m.capacity; ++j, s = (s + 1) & mask) {
    const int64_t k = im_ld(m.slot_key + s);
    if (k == key) return (int64_t)s;
    if (k == IM_EMPTY) return -1;
  }
  return -2;
}
// the slot that holds `key` once this returns - found, or claimed from the empty slots -, or -2 (capacity slots probed)
__device__ __forceinline__ int64_t im_claim(const tg_idmap& m, int64_t key) {
  const uint64_t mask = (uint64_t)m.capacity - 1;
  uint64_t s = idmap_mix(key) & mask;
  for (int64_t j = 0; j < m.capacity; ++j, s = (s + 1) & mask) {
    int64_t k = im_ld(m.slot_key + s);
    if (k == IM_EMPTY) {  // (a slot never becomes empty again: a key read here is final, an EMPTY read here is settled by the swap)
      k = (int64_t)atomicCAS(reinterpret_cast<unsigned long long*>(m.slot_key + s), (unsigned long long)IM_EMPTY,
                             (unsigned long long)key);
      if (k == IM_EMPTY) return (int64_t)s;
    }
    if (k == key) return (int64_t)s;
  }
  return -2;
}

__global__ void __launch_bounds__(IM_THREADS) k_idmap_lookup(tg_idmap m, const int64_t* __restrict__ keys, int64_t n,
                                                             int32_t* __restrict__ ids_out) {
  const int64_t nth = (int64_t)gridDim.x * IM_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * IM_THREADS + threadIdx.x; i < n; i += nth) {
    const int64_t key = keys[i];
    int32_t id = 0;
    if (key != IM_EMPTY) {
      const int64_t s = im_find(m, key);
      id = s >= 0 ? m.slot_id[s] : -1;
      if (id < 1) id = -1;  // (a slot that was claimed and never settled: no table of this library's)
    }
    ids_out[i] = id;
  }
}

struct IdmapAssignArgs {
  tg_idmap m;
  int64_t size, n, n_tile;
  const int64_t* keys;
  int32_t* ids_out;
  int64_t* out2;
  uint32_t* slot;   // [n] the slot of a position that waits for its rank
  int32_t* wpos;    // [n] the smallest position with the same key, or IM_DONE / IM_BAD_*
  uint64_t* words;  // [n_tile * IM_WORDS]
  uint32_t *cnt, *errs, *base;  // [n_tile], [n_tile], [n_tile + 1]
};

// positions first, first + step, ... < a.n
__device__ __forceinline__ void im_claim_pass(const IdmapAssignArgs& a, int64_t first, int64_t step) {
  for (int64_t i = first; i < a.n; i += step) {
    const int64_t key = a.keys[i];
    int32_t state = IM_DONE;
    if (key == IM_EMPTY) {
      a.ids_out[i] = 0;
    } else {
      const int64_t s = im_claim(a.m, key);
      if (s < 0) {
        a.ids_out[i] = -1;
        state = IM_BAD_PROBE;
      } else {
        const int32_t v = im_ld(a.m.slot_id + s);  // >= 1: settled before this call and not written by it; else < 0
        if (v >= 1) {
          a.ids_out[i] = v < a.size ? v : -1;
          if (v >= a.size) state = IM_BAD_TABLE;
        } else {
          atomicMin(a.m.slot_id + s, IM_PENDING + (int32_t)i);
          a.slot[i] = (uint32_t)s;
          state = 0;  // pending: the flags pass names the winner
        }
      }
    }
    a.wpos[i] = state;
  }
}

// one workgroup: tile `tile`
__device__ __forceinline__ void im_flag_tile(const IdmapAssignArgs& a, int64_t tile, uint32_t* s_cnt /*[IM_WAVES + 1]*/) {
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
      if (st == IM_BAD_PROBE) err |= TG_IDMAP_ERR_PROBE;
      if (st == IM_BAD_TABLE) err |= TG_IDMAP_ERR_TABLE;
      if (st >= 0) {
        const int64_t w = (int64_t)im_ld(a.m.slot_id + a.slot[p]) - (int64_t)IM_PENDING;
        if (w < 0 || w > p) {  // (the slot names no position of this call at or in front of p)
          err |= TG_IDMAP_ERR_TABLE;
          a.wpos[p] = IM_BAD_TABLE;
          a.ids_out[p] = -1;
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
__device__ __forceinline__ void im_bases_chunk(const IdmapAssignArgs& a, int64_t b, uint32_t* s_w /*[IM_WAVES + 1]*/) {
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
    a.out2[0] = a.size + (int64_t)(front + r);
    a.out2[1] = (int64_t)s_w[IM_WAVES];
  }
}

__device__ __forceinline__ void im_write_pass(const IdmapAssignArgs& a, int64_t first, int64_t step) {
  for (int64_t i = first; i < a.n; i += step) {
    const int64_t w = a.wpos[i];
    if (w < 0) continue;
    const int64_t tile = w / IM_TILE;
    const uint32_t off = (uint32_t)(w % IM_TILE);
    // offset 256 i + 64 wv + l is bit l of word 4 i + wv = off / 64: the words are in position order
    const uint32_t full = off / 64, part = off % 64;
    const uint64_t* __restrict__ wd = a.words + tile * IM_WORDS;
    uint32_t r = a.base[tile];  // new keys in front of the tile, then in front of w inside it
    for (uint32_t j = 0; j < full; ++j) r += (uint32_t)__popcll(wd[j]);
    r += (uint32_t)__popcll(wd[full] & ((1ull << part) - 1ull));
    const int64_t id = a.size + (int64_t)r;
    if (id >= a.m.key_rows) continue;  // (the entry checked size + n <= key_rows: a workspace that is no plan of this call)
    a.ids_out[i] = (int32_t)id;
    if (w == i) {
      a.m.slot_id[a.slot[i]] = (int32_t)id;
      a.m.key_of[id] = a.keys[i];
    }
  }
}

__global__ void __launch_bounds__(IM_THREADS) k_idmap_claim(IdmapAssignArgs a) {
  im_claim_pass(a, (int64_t)blockIdx.x * IM_THREADS + threadIdx.x, (int64_t)gridDim.x * IM_THREADS);
}
__global__ void __launch_bounds__(IM_THREADS) k_idmap_flags(IdmapAssignArgs a) {
  __shared__ uint32_t s_cnt[IM_WAVES + 1];
  im_flag_tile(a, (int64_t)blockIdx.x, s_cnt);
}
__global__ void __launch_bounds__(IM_THREADS) k_idmap_bases(IdmapAssignArgs a) {
  __shared__ uint32_t s_w[IM_WAVES + 1];
  im_bases_chunk(a, (int64_t)blockIdx.x, s_w);
}
__global__ void __launch_bounds__(IM_THREADS) k_idmap_write(IdmapAssignArgs a) {
  im_write_pass(a, (int64_t)blockIdx.x * IM_THREADS + threadIdx.x, (int64_t)gridDim.x * IM_THREADS);
}
// n <= IM_ONE_MAX: the four phases in one workgroup.  Position i belongs to thread i % 256 in EVERY phase (the claim and
// write passes stride by 256 from threadIdx.x, the flags pass takes p0 + 256 item + threadIdx.x), so slot[i] and wpos[i] are
// written and read by one and the same thread; what crosses threads - the flag words, the count, the bases - goes through
// the workspace with plain stores and loads of one workgroup, ordered by the barriers, and slot_id through agent-scope
// atomics and L1-bypassing loads, which the barriers order as well.
__global__ void __launch_bounds__(IM_THREADS) k_idmap_assign_one(IdmapAssignArgs a) {
  __shared__ uint32_t s_w[IM_WAVES + 1];
  im_claim_pass(a, threadIdx.x, IM_THREADS);
  __syncthreads();
  if (a.n_tile) im_flag_tile(a, 0, s_w);
  __syncthreads();
  im_bases_chunk(a, 0, s_w);
  __syncthreads();
  im_write_pass(a, threadIdx.x, IM_THREADS);
}

__device__ __forceinline__ void im_rebuild_error(int64_t* out2, int64_t row, uint32_t cls) {
  atomicMax(reinterpret_cast<unsigned long long*>(out2 + 1), ((unsigned long long)(0x7fffffffLL - row) << 8) | cls);
}
// rows [1, size): claim a slot; the slot ends with IM_PENDING + the smallest row that holds its key
__global__ void __launch_bounds__(IM_THREADS) k_idmap_rebuild_claim(tg_idmap m, int64_t size, int64_t* __restrict__ out2) {
  const int64_t r = 1 + (int64_t)blockIdx.x * IM_THREADS + threadIdx.x;
  if (r >= size) return;
  const int64_t key = m.key_of[r];
  if (key == IM_EMPTY) return im_rebuild_error(out2, r, TG_IDMAP_ERR_EMPTY_KEY);
  const int64_t s = im_claim(m, key);
  if (s < 0) return im_rebuild_error(out2, r, TG_IDMAP_ERR_PROBE);
  atomicMin(m.slot_id + s, IM_PENDING + (int32_t)r);
}
// rows [1, size): the smallest row of a key settles the slot, every other row of that key is a duplicate.  (A reader of
// slot_id meets the pending form or the settled one: both name the same row.)
__global__ void __launch_bounds__(IM_THREADS) k_idmap_rebuild_settle(tg_idmap m, int64_t size, int64_t* __restrict__ out2) {
  const int64_t r = 1 + (int64_t)blockIdx.x * IM_THREADS + threadIdx.x;
  if (r == 1) out2[0] = size;
  if (r >= size) return;
  const int64_t key = m.key_of[r];
  if (key == IM_EMPTY) return;
  const int64_t s = im_find(m, key);
  if (s < 0) return;  // (launch A has reported the probe bound)
  const int32_t v = im_ld(m.slot_id + s);
  const int64_t w = v < 0 ? (int64_t)v - (int64_t)IM_PENDING : (int64_t)v;
  if (w == r) m.slot_id[s] = (int32_t)r;
  else im_rebuild_error(out2, r, w < r ? TG_IDMAP_ERR_DUP : TG_IDMAP_ERR_TABLE);  // (w > r: the table was not empty)
}

struct IdmapLayout {
  int64_t n_tile;
  size_t slot, wpos, words, cnt, errs, base, total;
};
static IdmapLayout idmap_layout(int64_t n) {
  IdmapLayout l{};
  l.n_tile = cdiv(n, IM_TILE);
  l.slot = 0;
  l.wpos = l.slot + align16((size_t)n * sizeof(uint32_t));
  l.words = l.wpos + align16((size_t)n * sizeof(int32_t));
  l.cnt = l.words + align16((size_t)l.n_tile * IM_WORDS * sizeof(uint64_t));
  l.errs = l.cnt + align16((size_t)l.n_tile * sizeof(uint32_t));
  l.base = l.errs + align16((size_t)l.n_tile * sizeof(uint32_t));
  l.total = l.base + align16((size_t)(l.n_tile + 1) * sizeof(uint32_t));
  return l;
}

// a table the kernels may probe, holding `size` ids and room for `n` more: the load stays <= 1/2
static int idmap_args(const tg_idmap* m, int64_t size, int64_t n) {
  if (!m || !m->slot_key || !m->slot_id || !m->key_of) return TG_EINVAL;
  if (m->capacity < 16 || m->capacity > (1LL << 32) || (m->capacity & (m->capacity - 1))) return TG_EINVAL;
  if (size < 1 || n < 0 || size > 0x7fffffffLL || n > 0x7fffffffLL - size) return TG_EINVAL;
  if (2 * (size + n) > m->capacity || size + n > m->key_rows) return TG_EINVAL;
  return TG_OK;
}

// host twins' probe: the slot of `key`, or of the first empty slot (*found = false), or -1 after capacity slots
static int64_t host_probe(const tg_idmap* m, int64_t key, bool* found) {
  const uint64_t mask = (uint64_t)m->capacity - 1;
  uint64_t s = idmap_mix(key) & mask;
  for (int64_t j = 0; j < m->capacity; ++j, s = (s + 1) & mask) {
    *found = m->slot_key[s] == key;
    if (*found || m->slot_key[s] == IM_EMPTY) return (int64_t)s;
  }
  return -1;
}

}  // namespace tg

using namespace tg;

extern "C" uint64_t tg_idmap_hash(int64_t key) { return idmap_mix(key); }

extern "C" size_t tg_idmap_assign_workspace_bytes(int64_t n) {
  if (n < 0 || n > 0x7fffffffLL) return 0;
  return idmap_layout(n).total;
}

extern "C" int tg_idmap_lookup(const tg_idmap* map, const int64_t* keys, int64_t n, int32_t* ids_out, void* stream) {
  if (int rc = idmap_args(map, 1, 0)) return rc;
  if (n < 0 || (n > 0 && (!keys || !ids_out))) return TG_EINVAL;
  if (n == 0) return TG_OK;
  hipLaunchKernelGGL(k_idmap_lookup, dim3(flat_grid(n, IM_THREADS)), dim3(IM_THREADS), 0, as_stream(stream), *map, keys, n,
                     ids_out);
  return check_launch("tg_idmap_lookup");
}

extern "C" int tg_idmap_assign(const tg_idmap* map, int64_t size, const int64_t* keys, int64_t n, int32_t* ids_out,
                               int64_t* out2, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = idmap_args(map, size, n)) return rc;
  if (!out2 || (n > 0 && (!keys || !ids_out))) return TG_EINVAL;
  const IdmapLayout l = idmap_layout(n);
  if (int rc = ws_check(ws, ws_bytes, l.total)) return rc;  // before the first launch
  char* b = static_cast<char*>(ws);
  IdmapAssignArgs a{*map, size, n, l.n_tile, keys, ids_out, out2,
                    reinterpret_cast<uint32_t*>(b + l.slot), reinterpret_cast<int32_t*>(b + l.wpos),
                    reinterpret_cast<uint64_t*>(b + l.words), reinterpret_cast<uint32_t*>(b + l.cnt),
                    reinterpret_cast<uint32_t*>(b + l.errs), reinterpret_cast<uint32_t*>(b + l.base)};
  hipStream_t st = as_stream(stream);
  if (n <= IM_ONE_MAX) {
    hipLaunchKernelGGL(k_idmap_assign_one, dim3(1), dim3(IM_THREADS), 0, st, a);
    return check_launch("tg_idmap_assign");
  }
  const unsigned flat = (unsigned)cdiv(n, IM_THREADS);
  hipLaunchKernelGGL(k_idmap_claim, dim3(flat), dim3(IM_THREADS), 0, st, a);
  hipLaunchKernelGGL(k_idmap_flags, dim3((unsigned)l.n_tile), dim3(IM_THREADS), 0, st, a);
  hipLaunchKernelGGL(k_idmap_bases, dim3((unsigned)cdiv(l.n_tile + 1, IM_THREADS)), dim3(IM_THREADS), 0, st, a);
  hipLaunchKernelGGL(k_idmap_write, dim3(flat), dim3(IM_THREADS), 0, st, a);
  return check_launch("tg_idmap_assign");
}

extern "C" int tg_idmap_rebuild(const tg_idmap* map, int64_t size, int64_t* out2, void* stream) {
  if (int rc = idmap_args(map, size, 0)) return rc;
  if (!out2) return TG_EINVAL;
  hipStream_t st = as_stream(stream);
  if (hipError_t e = hipMemsetAsync(out2, 0, 2 * sizeof(int64_t), st)) {
    set_hip_error(e, "tg_idmap_rebuild");
    return TG_EHIP;
  }
  const unsigned grid = (unsigned)std::max<int64_t>(cdiv(size - 1, IM_THREADS), 1);
  hipLaunchKernelGGL(k_idmap_rebuild_claim, dim3(grid), dim3(IM_THREADS), 0, st, *map, size, out2);
  hipLaunchKernelGGL(k_idmap_rebuild_settle, dim3(grid), dim3(IM_THREADS), 0, st, *map, size, out2);
  return check_launch("tg_idmap_rebuild");
}

// The host twins: plain C++ over host pointers (those of `map` included), one key after the other.
extern "C" int tg_idmap_lookup_host(const tg_idmap* map, const int64_t* keys, int64_t n, int32_t* ids_out) {
  if (int rc = idmap_args(map, 1, 0)) return rc;
  if (n < 0 || (n > 0 && (!keys || !ids_out))) return TG_EINVAL;
  for (int64_t i = 0; i < n; ++i) {
    int32_t id = 0;
    if (keys[i] != IM_EMPTY) {
      bool found = false;
      const int64_t s = host_probe(map, keys[i], &found);
      id = (s >= 0 && found) ? map->slot_id[s] : -1;
      if (id < 1) id = -1;
    }
    ids_out[i] = id;
  }
  return TG_OK;
}

extern "C" int tg_idmap_assign_host(const tg_idmap* map, int64_t size, const int64_t* keys, int64_t n, int32_t* ids_out,
                                    int64_t* out2) {
  if (int rc = idmap_args(map, size, n)) return rc;
  if (!out2 || (n > 0 && (!keys || !ids_out))) return TG_EINVAL;
  int64_t err = 0, next = size;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t key = keys[i];
    if (key == IM_EMPTY) {
      ids_out[i] = 0;
      continue;
    }
    bool found = false;
    const int64_t s = host_probe(map, key, &found);
    if (s < 0) {
      ids_out[i] = -1;
      err |= TG_IDMAP_ERR_PROBE;
    } else if (found) {
      const int32_t v = map->slot_id[s];
      ids_out[i] = (v >= 1 && v < next) ? v : -1;
      if (ids_out[i] < 0) err |= TG_IDMAP_ERR_TABLE;
    } else {
      map->slot_key[s] = key;
      map->slot_id[s] = (int32_t)next;
      map->key_of[next] = key;
      ids_out[i] = (int32_t)next++;
    }
  }
  out2[0] = next;
  out2[1] = err;
  return TG_OK;
}

extern "C" int tg_idmap_rebuild_host(const tg_idmap* map, int64_t size, int64_t* out2) {
  if (int rc = idmap_args(map, size, 0)) return rc;
  if (!out2) return TG_EINVAL;
  int64_t err = 0;  // the first offending row in row order is the smallest
  for (int64_t r = 1; r < size; ++r) {
    const int64_t key = map->key_of[r];
    uint32_t cls = 0;
    if (key == IM_EMPTY) {
      cls = TG_IDMAP_ERR_EMPTY_KEY;
    } else {
      bool found = false;
      const int64_t s = host_probe(map, key, &found);
      if (s < 0) cls = TG_IDMAP_ERR_PROBE;
      else if (found) cls = TG_IDMAP_ERR_DUP;
      else {
        map->slot_key[s] = key;
        map->slot_id[s] = (int32_t)r;
      }
    }
    if (cls && !err) err = (int64_t)(((uint64_t)(0x7fffffffLL - r) << 8) | cls);
  }
  out2[0] = size;
  out2[1] = err;
  return TG_OK;
}
