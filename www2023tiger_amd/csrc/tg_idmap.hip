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
//
// Removing keys and recycling ids.  free_bits: uint64 words over the dense ids, bit i set <=> id i was
// released and not handed out again <=> key_of[i] == INT64_MIN (1 <= i < size; size is the high-water mark now).
// remove: a removed slot KEEPS its slot_key and gets slot_id = -1, so probe chains stay intact and a slot still never
// becomes empty again; lookup answers -1 for it and claim sends it down its pending path - a key that comes back is a new
// key.  Two phases: find (one thread per position; stores nothing to the table, so every copy of a key reads the same
// settled id) and apply (slot_id = -1, key_of[id] = INT64_MIN, 64-bit atomicOr on the bit; the thread whose atomicOr flips
// the bit counts the id and names it in released[] - one thread per distinct id, whatever the race; counts are summed per
// workgroup, then with one atomic add).  n <= 256: one workgroup, the phases separated by a barrier; else two launches.
// assign_recycle (n_free > 0): claim, flags and bases are those of assign.  The new key of rank r gets the r-th SMALLEST
// free id while r < n_free and size + (r - n_free) after that - the sequential loop that pops a heap of free ids.  A select
// over the bitmap writes the sorted list free_list[L], L = min(n_free, n): tiles of 2048 words (131 072 ids) per
// workgroup; launch 1 counts the set bits per tile, launch 2 sums the counts of the tiles in front (block_sum_front), scans
// the popcounts of its own words and writes the set bits of ranks < L (a wavefront at a time: the words of one lane are
// broadcast, lane l writes bit l); a tile whose base is >= L writes nothing.  The write
// pass takes free_list[r] or the tail id; the first occurrence also clears the taken bit with atomicAnd.  The select runs
// in its own two launches in front of the others in both forms (it depends on nothing they write); n <= 256 then runs claim,
// flags, bases and write in one workgroup.  A bitmap that does not hold n_free set bits raises TG_IDMAP_ERR_FREE, and a
// free id outside [1, size) TG_IDMAP_ERR_TABLE; neither becomes an address.
#include <algorithm>
#include <vector>

#include "tg_tcsr.h"
#include "tg_step.h"
#include "tg_idmap.h"

namespace tg {

// Batches up to here run in one workgroup of one launch: one key per thread.  Measured (profiles/idmap_one_max_v1.json,
// DESIGN 7.18): at 256 keys the one launch is the faster form; at 2 048 - eight keys per thread, each a chain of dependent
// atomics - the four launches are.  (Diagnostic builds: make EXTRA=-DTG_IDMAP_ONE_MAX=N, 0 <= N <= 2048.)
#ifndef TG_IDMAP_ONE_MAX
#define TG_IDMAP_ONE_MAX 256
#endif
constexpr int IM_ONE_MAX = TG_IDMAP_ONE_MAX;
static_assert(IM_ONE_MAX >= 0 && IM_ONE_MAX <= IM_TILE, "the one-workgroup form covers one tile");
constexpr int32_t IM_PENDING = INT32_MIN;  // slot_id of a slot claimed in this call: IM_PENDING + smallest position
// wpos[i] of a position that waits for no rank: done, or why it failed
constexpr int32_t IM_DONE = -1, IM_BAD_PROBE = -2, IM_BAD_TABLE = -3;

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

// first occurrences of new keys in front of position w
__device__ __forceinline__ uint32_t im_rank(const IdmapAssignArgs& a, int64_t w) {
  const int64_t tile = w / IM_TILE;
  const uint32_t off = (uint32_t)(w % IM_TILE);
  // offset 256 i + 64 wv + l is bit l of word 4 i + wv = off / 64: the words are in position order
  const uint32_t full = off / 64, part = off % 64;
  const uint64_t* __restrict__ wd = a.words + tile * IM_WORDS;
  uint32_t r = a.base[tile];  // new keys in front of the tile, then in front of w inside it
  for (uint32_t j = 0; j < full; ++j) r += (uint32_t)__popcll(wd[j]);
  return r + (uint32_t)__popcll(wd[full] & ((1ull << part) - 1ull));
}

__device__ __forceinline__ void im_write_pass(const IdmapAssignArgs& a, int64_t first, int64_t step) {
  for (int64_t i = first; i < a.n; i += step) {
    const int64_t w = a.wpos[i];
    if (w < 0) continue;
    const int64_t id = a.size + (int64_t)im_rank(a, w);
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
// rows [1, size): claim a slot; the slot ends with IM_PENDING + the smallest row that holds its key.  FREE: a row whose
// bit is set holds no key and is skipped; INT64_MIN under a clear bit and a key under a set bit are reported
template <bool FREE>
__global__ void __launch_bounds__(IM_THREADS) k_idmap_rebuild_claim(tg_idmap m, int64_t size, const uint64_t* __restrict__ bits,
                                                                     int64_t* __restrict__ out2) {
  const int64_t r = 1 + (int64_t)blockIdx.x * IM_THREADS + threadIdx.x;
  if (r >= size) return;
  const int64_t key = m.key_of[r];
  const bool gone = FREE && ((bits[r >> 6] >> (r & 63)) & 1ull);
  if (key == IM_EMPTY) {
    if (!gone) im_rebuild_error(out2, r, TG_IDMAP_ERR_EMPTY_KEY);
    return;
  }
  if (gone) return im_rebuild_error(out2, r, TG_IDMAP_ERR_FREE);
  const int64_t s = im_claim(m, key);
  if (s < 0) return im_rebuild_error(out2, r, TG_IDMAP_ERR_PROBE);
  atomicMin(m.slot_id + s, IM_PENDING + (int32_t)r);
}
// rows [1, size): the smallest row of a key settles the slot, every other row of that key is a duplicate.  (A reader of
// slot_id meets the pending form or the settled one: both name the same row.)
template <bool FREE>
__global__ void __launch_bounds__(IM_THREADS) k_idmap_rebuild_settle(tg_idmap m, int64_t size, const uint64_t* __restrict__ bits,
                                                                      int64_t* __restrict__ out2) {
  const int64_t r = 1 + (int64_t)blockIdx.x * IM_THREADS + threadIdx.x;
  if (r == 1) out2[0] = size;
  if (r >= size) return;
  const int64_t key = m.key_of[r];
  if (key == IM_EMPTY) return;
  if (FREE && ((bits[r >> 6] >> (r & 63)) & 1ull)) return;  // (launch A has reported it)
  const int64_t s = im_find(m, key);
  if (s < 0) return;  // (launch A has reported the probe bound)
  const int32_t v = im_ld(m.slot_id + s);
  const int64_t w = v < 0 ? (int64_t)v - (int64_t)IM_PENDING : (int64_t)v;
  if (w == r) m.slot_id[s] = (int32_t)r;
  else im_rebuild_error(out2, r, w < r ? TG_IDMAP_ERR_DUP : TG_IDMAP_ERR_TABLE);  // (w > r: the table was not empty)
}

// ---- removing keys ---------------------------------------------------------------------------------------------------
struct IdmapRemoveArgs {
  tg_idmap m;
  int64_t size, n, bit_words;
  const int64_t* keys;
  int32_t* ids_out;
  int32_t* released;  // [n] the id at the position that released it, INT32_MAX elsewhere
  uint64_t* bits;
  int64_t* out2;   // {ids released, error bits}: zeroed before the first launch
  uint32_t* slot;  // [n] the slot of a position whose key the map holds
};
// phase 1: nothing is stored to the table
__device__ __forceinline__ void im_remove_find(const IdmapRemoveArgs& a, int64_t first, int64_t step) {
  uint32_t err = 0;
  for (int64_t i = first; i < a.n; i += step) {
    const int64_t key = a.keys[i];
    int32_t id = 0;
    if (key != IM_EMPTY) {
      id = -1;
      const int64_t s = im_find(a.m, key);
      if (s == -2) err |= TG_IDMAP_ERR_PROBE;
      if (s >= 0) {
        const int32_t v = im_ld(a.m.slot_id + s);  // < 1: removed before this call
        if (v >= 1) {
          if (v < a.size && v < a.m.key_rows && (v >> 6) < a.bit_words) {
            id = v;
            a.slot[i] = (uint32_t)s;
          } else {
            err |= TG_IDMAP_ERR_TABLE;
          }
        }
      }
    }
    a.ids_out[i] = id;
    a.released[i] = INT32_MAX;
  }
  if (err) atomicOr(reinterpret_cast<unsigned long long*>(a.out2 + 1), (unsigned long long)err);
}
// phase 2: every thread of the workgroup arrives here (the count is summed over the workgroup)
__device__ __forceinline__ void im_remove_apply(const IdmapRemoveArgs& a, int64_t first, int64_t step, uint32_t* s_w) {
  uint32_t mine = 0;
  for (int64_t i = first; i < a.n; i += step) {
    const int32_t id = a.ids_out[i];
    if (id < 1 || id >= a.size || id >= a.m.key_rows || (id >> 6) >= a.bit_words) continue;
    const uint32_t s = a.slot[i];
    if ((int64_t)s >= a.m.capacity) continue;  // (a workspace that is not phase 1's)
    a.m.slot_id[s] = -1;
    a.m.key_of[id] = IM_EMPTY;
    const unsigned long long bit = 1ull << (id & 63);
    const unsigned long long old = atomicOr(reinterpret_cast<unsigned long long*>(a.bits + (id >> 6)), bit);
    if (!(old & bit)) {
      ++mine;
      a.released[i] = id;
    }
  }
  uint32_t total;
  block_excl_scan(mine, s_w, &total);
  if (threadIdx.x == 0 && total) atomicAdd(reinterpret_cast<unsigned long long*>(a.out2), (unsigned long long)total);
}
__global__ void __launch_bounds__(IM_THREADS) k_idmap_remove_find(IdmapRemoveArgs a) {
  im_remove_find(a, (int64_t)blockIdx.x * IM_THREADS + threadIdx.x, (int64_t)gridDim.x * IM_THREADS);
}
__global__ void __launch_bounds__(IM_THREADS) k_idmap_remove_apply(IdmapRemoveArgs a) {
  __shared__ uint32_t s_w[IM_WAVES];
  im_remove_apply(a, (int64_t)blockIdx.x * IM_THREADS + threadIdx.x, (int64_t)gridDim.x * IM_THREADS, s_w);
}
// n <= IM_ONE_MAX: position i belongs to thread i in both phases; the barrier orders the table loads of phase 1 in front
// of the stores of phase 2
__global__ void __launch_bounds__(IM_THREADS) k_idmap_remove_one(IdmapRemoveArgs a) {
  __shared__ uint32_t s_w[IM_WAVES];
  im_remove_find(a, threadIdx.x, IM_THREADS);
  __syncthreads();
  im_remove_apply(a, threadIdx.x, IM_THREADS, s_w);
}

// ---- assigning with free ids: the select over the bitmap and the write pass --------------------------------------------
constexpr int IM_SEL_ITEMS = 8;
constexpr int IM_SEL_TILE = IM_THREADS * IM_SEL_ITEMS;  // bitmap words per workgroup: 131 072 ids
struct IdmapFreeArgs {
  uint64_t* bits;
  int64_t sel_words;  // ceil(size / 64): the words the select reads
  int64_t n_sel;      // tiles of the select
  int64_t n_free, L;  // L = min(n_free, n)
  int32_t* free_list;  // [L] the L smallest free ids, ascending
  uint32_t* tcnt;      // [n_sel] set bits per tile
  uint32_t* ftotal;    // [1] set bits in all
};
// thread t of tile `tile` owns the 8 consecutive words from tile * 2048 + 8 t: thread order is id order
__device__ __forceinline__ uint32_t im_sel_load(const IdmapFreeArgs& f, int64_t tile, uint64_t (&w)[IM_SEL_ITEMS]) {
  const int64_t w0 = tile * IM_SEL_TILE + (int64_t)threadIdx.x * IM_SEL_ITEMS;
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < IM_SEL_ITEMS; ++j) {
    w[j] = w0 + j < f.sel_words ? f.bits[w0 + j] : 0ull;
    c += (uint32_t)__popcll(w[j]);
  }
  return c;
}
__global__ void __launch_bounds__(IM_THREADS) k_idmap_select_count(IdmapFreeArgs f) {
  __shared__ uint32_t s_w[IM_WAVES];
  uint64_t w[IM_SEL_ITEMS];
  uint32_t total;
  block_excl_scan(im_sel_load(f, (int64_t)blockIdx.x, w), s_w, &total);
  if (threadIdx.x == 0) f.tcnt[blockIdx.x] = total;
}
__global__ void __launch_bounds__(IM_THREADS) k_idmap_select_write(IdmapFreeArgs f) {
  __shared__ uint32_t s_w[IM_WAVES];
  const int64_t tile = (int64_t)blockIdx.x;
  const uint32_t front = block_sum_front(f.tcnt, (uint32_t)tile, s_w);  // (tile < 2^14)
  if (tile != f.n_sel - 1 && (int64_t)front >= f.L) return;           // (block-uniform: nothing of this tile is taken)
  uint64_t w[IM_SEL_ITEMS];
  uint32_t total;
  const uint32_t mine = im_sel_load(f, tile, w);
  const uint32_t r = front + block_excl_scan(mine, s_w, &total);  // the rank of this thread's first set bit (< 2^31)
  if (tile == f.n_sel - 1 && threadIdx.x == 0) f.ftotal[0] = front + total;
  // The wavefront writes together: for every lane that owns set bits of a rank below L, its eight words are broadcast and
  // lane l writes bit l of each - 64 consecutive ids per store instruction, however dense the bitmap is.  (One thread
  // writing its own up to 512 bits one after the other made a tile of a nearly all-free bitmap the call's longest kernel.)
  const int lane = lane_id();
  const uint64_t below = (1ull << lane) - 1ull;
  const int64_t id_wave = (tile * IM_SEL_TILE + (int64_t)(threadIdx.x - lane) * IM_SEL_ITEMS) * 64;
  uint64_t todo = __ballot(mine != 0 && (int64_t)r < f.L);  // (the same on every lane: the loop is wave-uniform)
  while (todo) {
    const int src = __ffsll((unsigned long long)todo) - 1;
    todo &= todo - 1;
    int64_t rr = (int64_t)(uint32_t)__shfl((int)r, src);
    const int64_t id0 = id_wave + (int64_t)src * IM_SEL_ITEMS * 64 + lane;
#pragma unroll
    for (int j = 0; j < IM_SEL_ITEMS; ++j) {
      const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)w[j], src), hi = (uint32_t)__shfl((int)(uint32_t)(w[j] >> 32), src);
      const uint64_t word = ((uint64_t)hi << 32) | lo;
      const int64_t rank = rr + __popcll(word & below);
      if (((word >> lane) & 1ull) && rank < f.L) f.free_list[rank] = (int32_t)(id0 + j * 64);
      rr += __popcll(word);
    }
  }
}

__device__ __forceinline__ void im_write_recycle(const IdmapAssignArgs& a, const IdmapFreeArgs& f, int64_t first, int64_t step) {
  const int64_t have = (int64_t)f.ftotal[0];
  if (first == 0 && have != f.n_free)
    atomicOr(reinterpret_cast<unsigned long long*>(a.out2 + 1), (unsigned long long)TG_IDMAP_ERR_FREE);
  for (int64_t i = first; i < a.n; i += step) {
    const int64_t w = a.wpos[i];
    if (w < 0) continue;
    const int64_t r = (int64_t)im_rank(a, w);
    const bool recycled = r < f.n_free;
    int64_t id = -1;
    if (!recycled) id = a.size + (r - f.n_free);
    else if (r < f.L && r < have) id = (int64_t)f.free_list[r];
    if (id < 1 || id >= a.m.key_rows || (recycled && id >= a.size)) {  // (no id of this map: it is no address)
      a.ids_out[i] = -1;
      if (recycled && r < have) atomicOr(reinterpret_cast<unsigned long long*>(a.out2 + 1), (unsigned long long)TG_IDMAP_ERR_TABLE);
      continue;
    }
    a.ids_out[i] = (int32_t)id;
    if (w == i) {
      a.m.slot_id[a.slot[i]] = (int32_t)id;
      a.m.key_of[id] = a.keys[i];
      if (recycled) atomicAnd(reinterpret_cast<unsigned long long*>(f.bits + (id >> 6)), ~(1ull << (id & 63)));
    }
  }
}
__global__ void __launch_bounds__(IM_THREADS) k_idmap_write_recycle(IdmapAssignArgs a, IdmapFreeArgs f) {
  im_write_recycle(a, f, (int64_t)blockIdx.x * IM_THREADS + threadIdx.x, (int64_t)gridDim.x * IM_THREADS);
}
// n <= IM_ONE_MAX, behind the two select launches: as k_idmap_assign_one, with the recycling write pass
__global__ void __launch_bounds__(IM_THREADS) k_idmap_assign_recycle_one(IdmapAssignArgs a, IdmapFreeArgs f) {
  __shared__ uint32_t s_w[IM_WAVES + 1];
  im_claim_pass(a, threadIdx.x, IM_THREADS);
  __syncthreads();
  if (a.n_tile) im_flag_tile(a, 0, s_w);
  __syncthreads();
  im_bases_chunk(a, 0, s_w);
  __syncthreads();
  im_write_recycle(a, f, threadIdx.x, IM_THREADS);
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

struct IdmapFreeLayout {
  IdmapLayout a;
  int64_t n_sel;
  size_t tcnt, ftotal, total;
};
static IdmapFreeLayout idmap_free_layout(int64_t n, int64_t size) {
  IdmapFreeLayout l{};
  l.a = idmap_layout(n);
  l.n_sel = std::max<int64_t>(cdiv(cdiv(size, 64), IM_SEL_TILE), 1);
  l.tcnt = l.a.total;
  l.ftotal = l.tcnt + align16((size_t)l.n_sel * sizeof(uint32_t));
  l.total = l.ftotal + 16;
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

// the entries that know of free ids: `size` is the high-water mark, `occupied` bounds the slots in use (gone ones
// included) and decides the load; the bitmap covers [0, size)
static int idmap_free_args(const tg_idmap* m, int64_t size, int64_t occupied, int64_t n, int64_t n_free, const uint64_t* bits,
                           int64_t bit_words) {
  if (!m || !m->slot_key || !m->slot_id || !m->key_of || !bits) return TG_EINVAL;
  if (m->capacity < 16 || m->capacity > (1LL << 32) || (m->capacity & (m->capacity - 1))) return TG_EINVAL;
  if (size < 1 || n < 0 || size > 0x7fffffffLL || n > 0x7fffffffLL || occupied < 0 || occupied > 0x7fffffffLL) return TG_EINVAL;
  if (n_free < 0 || n_free >= size || bit_words < cdiv(size, 64)) return TG_EINVAL;
  const int64_t grown = size + std::max<int64_t>(0, n - n_free);
  if (grown > 0x7fffffffLL || grown > m->key_rows || 2 * (occupied + n) > m->capacity) return TG_EINVAL;
  return TG_OK;
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
  hipLaunchKernelGGL(k_idmap_rebuild_claim<false>, dim3(grid), dim3(IM_THREADS), 0, st, *map, size, nullptr, out2);
  hipLaunchKernelGGL(k_idmap_rebuild_settle<false>, dim3(grid), dim3(IM_THREADS), 0, st, *map, size, nullptr, out2);
  return check_launch("tg_idmap_rebuild");
}

extern "C" int tg_idmap_rebuild_free(const tg_idmap* map, int64_t size, int64_t live, const uint64_t* free_bits,
                                     int64_t free_words, int64_t* out2, void* stream) {
  if (live < 1 || live > size) return TG_EINVAL;
  if (int rc = idmap_free_args(map, size, live, 0, 0, free_bits, free_words)) return rc;
  if (!out2) return TG_EINVAL;
  hipStream_t st = as_stream(stream);
  if (hipError_t e = hipMemsetAsync(out2, 0, 2 * sizeof(int64_t), st)) {
    set_hip_error(e, "tg_idmap_rebuild_free");
    return TG_EHIP;
  }
  const unsigned grid = (unsigned)std::max<int64_t>(cdiv(size - 1, IM_THREADS), 1);
  hipLaunchKernelGGL(k_idmap_rebuild_claim<true>, dim3(grid), dim3(IM_THREADS), 0, st, *map, size, free_bits, out2);
  hipLaunchKernelGGL(k_idmap_rebuild_settle<true>, dim3(grid), dim3(IM_THREADS), 0, st, *map, size, free_bits, out2);
  return check_launch("tg_idmap_rebuild_free");
}

extern "C" size_t tg_idmap_remove_workspace_bytes(int64_t n) {
  if (n < 0 || n > 0x7fffffffLL) return 0;
  return align16((size_t)n * sizeof(uint32_t));
}

extern "C" int tg_idmap_remove(const tg_idmap* map, int64_t size, uint64_t* free_bits, int64_t free_words, const int64_t* keys,
                               int64_t n, int32_t* ids_out, int32_t* released_out, int64_t* out2, void* ws, size_t ws_bytes,
                               void* stream) {
  if (int rc = idmap_free_args(map, size, 0, 0, 0, free_bits, free_words)) return rc;
  if (n < 0 || n > 0x7fffffffLL || !out2 || (n > 0 && (!keys || !ids_out || !released_out))) return TG_EINVAL;
  if (int rc = ws_check(ws, ws_bytes, tg_idmap_remove_workspace_bytes(n))) return rc;  // before the first launch
  hipStream_t st = as_stream(stream);
  if (hipError_t e = hipMemsetAsync(out2, 0, 2 * sizeof(int64_t), st)) {
    set_hip_error(e, "tg_idmap_remove");
    return TG_EHIP;
  }
  if (n == 0) return TG_OK;
  IdmapRemoveArgs a{*map, size, n, free_words, keys, ids_out, released_out, free_bits, out2, static_cast<uint32_t*>(ws)};
  if (n <= IM_ONE_MAX) {
    hipLaunchKernelGGL(k_idmap_remove_one, dim3(1), dim3(IM_THREADS), 0, st, a);
    return check_launch("tg_idmap_remove");
  }
  const unsigned grid = flat_grid(n, IM_THREADS);
  hipLaunchKernelGGL(k_idmap_remove_find, dim3(grid), dim3(IM_THREADS), 0, st, a);
  hipLaunchKernelGGL(k_idmap_remove_apply, dim3(grid), dim3(IM_THREADS), 0, st, a);
  return check_launch("tg_idmap_remove");
}

extern "C" size_t tg_idmap_assign_recycle_workspace_bytes(int64_t n, int64_t size) {
  if (n < 0 || n > 0x7fffffffLL || size < 1 || size > 0x7fffffffLL) return 0;
  return idmap_free_layout(n, size).total;
}

extern "C" int tg_idmap_assign_recycle(const tg_idmap* map, int64_t size, int64_t occupied, uint64_t* free_bits,
                                       int64_t free_words, int64_t n_free, const int64_t* keys, int64_t n, int32_t* ids_out,
                                       int32_t* free_list_out, int64_t* out2, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = idmap_free_args(map, size, occupied, n, n_free, free_bits, free_words)) return rc;
  if (!out2 || (n > 0 && (!keys || !ids_out))) return TG_EINVAL;
  const int64_t L = std::min(n_free, n);
  if (L > 0 && !free_list_out) return TG_EINVAL;
  const IdmapFreeLayout l = idmap_free_layout(n, size);
  if (int rc = ws_check(ws, ws_bytes, l.total)) return rc;  // before the first launch
  char* b = static_cast<char*>(ws);
  IdmapAssignArgs a{*map, size, n, l.a.n_tile, keys, ids_out, out2,
                    reinterpret_cast<uint32_t*>(b + l.a.slot), reinterpret_cast<int32_t*>(b + l.a.wpos),
                    reinterpret_cast<uint64_t*>(b + l.a.words), reinterpret_cast<uint32_t*>(b + l.a.cnt),
                    reinterpret_cast<uint32_t*>(b + l.a.errs), reinterpret_cast<uint32_t*>(b + l.a.base)};
  IdmapFreeArgs f{free_bits, cdiv(size, 64), l.n_sel, n_free, L, free_list_out,
                  reinterpret_cast<uint32_t*>(b + l.tcnt), reinterpret_cast<uint32_t*>(b + l.ftotal)};
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(k_idmap_select_count, dim3((unsigned)l.n_sel), dim3(IM_THREADS), 0, st, f);
  hipLaunchKernelGGL(k_idmap_select_write, dim3((unsigned)l.n_sel), dim3(IM_THREADS), 0, st, f);
  if (n <= IM_ONE_MAX) {
    hipLaunchKernelGGL(k_idmap_assign_recycle_one, dim3(1), dim3(IM_THREADS), 0, st, a, f);
    return check_launch("tg_idmap_assign_recycle");
  }
  const unsigned flat = (unsigned)cdiv(n, IM_THREADS);
  hipLaunchKernelGGL(k_idmap_claim, dim3(flat), dim3(IM_THREADS), 0, st, a);
  hipLaunchKernelGGL(k_idmap_flags, dim3((unsigned)l.a.n_tile), dim3(IM_THREADS), 0, st, a);
  hipLaunchKernelGGL(k_idmap_bases, dim3((unsigned)cdiv(l.a.n_tile + 1, IM_THREADS)), dim3(IM_THREADS), 0, st, a);
  hipLaunchKernelGGL(k_idmap_write_recycle, dim3(flat), dim3(IM_THREADS), 0, st, a, f);
  return check_launch("tg_idmap_assign_recycle");
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

extern "C" int tg_idmap_rebuild_free_host(const tg_idmap* map, int64_t size, int64_t live, const uint64_t* free_bits,
                                          int64_t free_words, int64_t* out2) {
  if (live < 1 || live > size) return TG_EINVAL;
  if (int rc = idmap_free_args(map, size, live, 0, 0, free_bits, free_words)) return rc;
  if (!out2) return TG_EINVAL;
  int64_t err = 0;
  for (int64_t r = 1; r < size; ++r) {
    const int64_t key = map->key_of[r];
    const bool gone = (free_bits[r >> 6] >> (r & 63)) & 1ull;
    uint32_t cls = 0;
    if (key == IM_EMPTY) {
      if (!gone) cls = TG_IDMAP_ERR_EMPTY_KEY;
    } else if (gone) {
      cls = TG_IDMAP_ERR_FREE;
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

extern "C" int tg_idmap_remove_host(const tg_idmap* map, int64_t size, uint64_t* free_bits, int64_t free_words,
                                    const int64_t* keys, int64_t n, int32_t* ids_out, int32_t* released_out, int64_t* out2) {
  if (int rc = idmap_free_args(map, size, 0, 0, 0, free_bits, free_words)) return rc;
  if (n < 0 || n > 0x7fffffffLL || !out2 || (n > 0 && (!keys || !ids_out || !released_out))) return TG_EINVAL;
  int64_t err = 0, released = 0;
  // phase 1 in full before phase 2, as on the device: every copy of a key reads the id it had before the call
  std::vector<int64_t> slot((size_t)n, -1);
  for (int64_t i = 0; i < n; ++i) {
    int32_t id = 0;
    if (keys[i] != IM_EMPTY) {
      id = -1;
      bool found = false;
      const int64_t s = host_probe(map, keys[i], &found);
      if (s < 0) err |= TG_IDMAP_ERR_PROBE;
      else if (found && map->slot_id[s] >= 1) {
        if (map->slot_id[s] < size) {
          id = map->slot_id[s];
          slot[(size_t)i] = s;
        } else {
          err |= TG_IDMAP_ERR_TABLE;
        }
      }
    }
    ids_out[i] = id;
    released_out[i] = INT32_MAX;
  }
  for (int64_t i = 0; i < n; ++i) {
    const int32_t id = ids_out[i];
    if (id < 1) continue;
    map->slot_id[slot[(size_t)i]] = -1;
    map->key_of[id] = IM_EMPTY;
    const uint64_t bit = 1ull << (id & 63);
    if (!(free_bits[id >> 6] & bit)) {
      free_bits[id >> 6] |= bit;
      released_out[i] = id;
      ++released;
    }
  }
  out2[0] = released;
  out2[1] = err;
  return TG_OK;
}

extern "C" int tg_idmap_assign_recycle_host(const tg_idmap* map, int64_t size, int64_t occupied, uint64_t* free_bits,
                                            int64_t free_words, int64_t n_free, const int64_t* keys, int64_t n,
                                            int32_t* ids_out, int32_t* free_list_out, int64_t* out2) {
  if (int rc = idmap_free_args(map, size, occupied, n, n_free, free_bits, free_words)) return rc;
  if (!out2 || (n > 0 && (!keys || !ids_out))) return TG_EINVAL;
  const int64_t L = std::min(n_free, n);
  if (L > 0 && !free_list_out) return TG_EINVAL;
  int64_t err = 0, n_new = 0, have = 0;
  const int64_t words = cdiv(size, 64);
  for (int64_t w = 0; w < words; ++w) {  // the select: the L smallest free ids, and the number of set bits
    uint64_t word = free_bits[w];
    for (; word; word &= word - 1, ++have)
      if (have < L) free_list_out[have] = (int32_t)(w * 64 + __builtin_ctzll(word));
  }
  if (have != n_free) err |= TG_IDMAP_ERR_FREE;
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
    } else if (found && map->slot_id[s] >= 1) {
      const int32_t v = map->slot_id[s];
      ids_out[i] = v < size + std::max<int64_t>(0, n_new - n_free) ? v : -1;
      if (ids_out[i] < 0) err |= TG_IDMAP_ERR_TABLE;
    } else {  // an empty slot, or the slot of a key that was removed: a new key
      const bool recycled = n_new < n_free;
      int64_t id = -1;
      if (!recycled) id = size + (n_new - n_free);
      else if (n_new < have) id = free_list_out[n_new];
      ++n_new;
      if (id < 1 || id >= map->key_rows || (recycled && id >= size)) {
        ids_out[i] = -1;
        if (recycled && n_new <= have) err |= TG_IDMAP_ERR_TABLE;
        continue;
      }
      map->slot_key[s] = key;
      map->slot_id[s] = (int32_t)id;
      map->key_of[id] = key;
      if (recycled) free_bits[id >> 6] &= ~(1ull << (id & 63));
      ids_out[i] = (int32_t)id;
    }
  }
  out2[0] = size + n_new;
  out2[1] = err;
  return TG_OK;
}
