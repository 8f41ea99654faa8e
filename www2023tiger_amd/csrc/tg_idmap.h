// What the key tables share (tg_idmap.hip: node keys -> dense ids; tg_events.hip: event keys -> edge-table rows): the
// geometry of the tiled passes, the home slot, the L1-bypassing loads and the read-only probe.  The algorithms stay in
// their own files.
#pragma once
#include "tg_common.h"

namespace tg {

constexpr int IM_THREADS = TG_SCAN_BLOCK;  // block_excl_scan: 256
constexpr int IM_ITEMS = 8;
constexpr int IM_TILE = IM_THREADS * IM_ITEMS;  // positions per workgroup
constexpr int IM_WORDS = IM_TILE / 64;          // flag words per tile
constexpr int IM_WAVES = IM_THREADS / TG_WAVE;
constexpr int64_t IM_EMPTY = TG_IDMAP_EMPTY;

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

// host twins' probe: the slot of `key`, or of the first empty slot (*found = false), or -1 after capacity slots
static inline int64_t host_probe(const tg_idmap* m, int64_t key, bool* found) {
  const uint64_t mask = (uint64_t)m->capacity - 1;
  uint64_t s = idmap_mix(key) & mask;
  for (int64_t j = 0; j < m->capacity; ++j, s = (s + 1) & mask) {
    *found = m->slot_key[s] == key;
    if (*found || m->slot_key[s] == IM_EMPTY) return (int64_t)s;
  }
  return -1;
}

// a table the kernels may probe: every array present, a capacity that is a power of two in [16, 2^32]
static inline int idmap_struct_ok(const tg_idmap* m) {
  if (!m || !m->slot_key || !m->slot_id || !m->key_of) return TG_EINVAL;
  if (m->capacity < 16 || m->capacity > (1LL << 32) || (m->capacity & (m->capacity - 1))) return TG_EINVAL;
  return TG_OK;
}

}  // namespace tg
