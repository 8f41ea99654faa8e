// A stand-alone host program for a sanitizer run of the event-key host twins: tg_events_screen_host and
// tg_events_repack_host at the wavefront, one-workgroup-bound and tile edges (0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048,
// 2049, 4097 keys; 1, 64, 65, 2049 rows) - every buffer allocated EXACTLY as tiger_hip.h sizes it, every result checked
// against a plain recomputation (std::map / a scatter loop).  The persistent table is filled by tg_idmap_rebuild_host and
// extended by tg_idmap_assign_host, as EventKeys does.  No GPU is touched.  Build and run:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude -Iwww2023tiger_amd/csrc \
//         tools/events_sanitize.cpp www2023tiger_amd/csrc/tg_events.hip www2023tiger_amd/csrc/tg_idmap.hip -o events_sanitize
//   ./events_sanitize            (exit status 0 and "ok": clean)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include <hip/hip_runtime.h>

#include "tiger_hip.h"

namespace tg {
void set_hip_error(hipError_t, const char*) {}  // (tg_graph.hip's, which the twins never reach)
}

static int failures = 0;
#define EXPECT(cond)                                               \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                  \
    }                                                              \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// a table over `rows` rows (row r holds key 1000 r + 7) with room for `extra` more: capacity and key_rows the smallest legal
struct Table {
  std::vector<int64_t> slot_key, key_of;
  std::vector<int32_t> slot_id;
  tg_idmap m;
  int64_t rows;
  Table(int64_t rows_, int64_t extra) : rows(rows_) {
    int64_t cap = 16;
    while (cap < 2 * (rows + extra)) cap <<= 1;
    slot_key.assign((size_t)cap, TG_IDMAP_EMPTY);
    slot_id.assign((size_t)cap, -1);
    key_of.assign((size_t)(rows + extra), TG_IDMAP_EMPTY);
    for (int64_t r = 1; r < rows; ++r) key_of[(size_t)r] = 1000 * r + 7;
    m = tg_idmap{cap, rows + extra, slot_key.data(), slot_id.data(), key_of.data()};
    int64_t out2[2];
    EXPECT(tg_idmap_rebuild_host(&m, rows, out2) == TG_OK && out2[1] == 0);
  }
};

static void screen_case(int64_t n, int mix) {
  Table t(301, n);
  std::vector<int64_t> keys((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t known = 1000 * (1 + (int64_t)(rnd() % 300)) + 7, fresh = 5000000 + 3 * i;
    switch (mix) {
      case 0: keys[(size_t)i] = fresh; break;                                   // all new and distinct
      case 1: keys[(size_t)i] = known; break;                                   // all known
      case 2: keys[(size_t)i] = 424242; break;                                  // all one key
      case 3: keys[(size_t)i] = 5000000 + 3 * (i % ((n + 1) / 2)); break;       // every key twice
      case 4: keys[(size_t)i] = i % 2 ? fresh : known; break;                   // interleaved
      default: keys[(size_t)i] = i % 7 == 3 ? TG_IDMAP_EMPTY : (i % 3 ? fresh : known);  // INT64_MIN among them
    }
  }
  const std::vector<int64_t> sk = t.slot_key, ko = t.key_of;
  const std::vector<int32_t> si = t.slot_id;
  std::vector<int32_t> eid((size_t)n);
  std::vector<int64_t> keep((size_t)n), out2(2);
  EXPECT(tg_events_screen_host(&t.m, t.rows, keys.data(), n, eid.data(), keep.data(), out2.data()) == TG_OK);
  EXPECT(sk == t.slot_key && si == t.slot_id && ko == t.key_of);  // read-only on the map
  std::map<int64_t, int32_t> d;
  for (int64_t r = 1; r < t.rows; ++r) d[1000 * r + 7] = (int32_t)r;
  int64_t kept = 0, err = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (keys[(size_t)i] == TG_IDMAP_EMPTY) {
      err = TG_EVENTS_ERR_KEY;
      EXPECT(eid[(size_t)i] == -1);
      continue;
    }
    auto it = d.find(keys[(size_t)i]);
    if (it == d.end()) {
      it = d.emplace(keys[(size_t)i], (int32_t)(t.rows + kept)).first;
      EXPECT(kept < n && keep[(size_t)kept] == i);
      ++kept;
    }
    EXPECT(eid[(size_t)i] == it->second);
  }
  EXPECT(out2[0] == kept && out2[1] == err);
  if (err) return;
  // commit what was kept, as EventKeys does, and screen again: nothing is kept, the rows are the committed ones
  std::vector<int64_t> kk((size_t)kept);
  for (int64_t j = 0; j < kept; ++j) kk[(size_t)j] = keys[(size_t)keep[(size_t)j]];
  std::vector<int32_t> ids((size_t)kept), eid2((size_t)n);
  EXPECT(tg_idmap_assign_host(&t.m, t.rows, kk.data(), kept, ids.data(), out2.data()) == TG_OK);
  EXPECT(out2[0] == t.rows + kept && out2[1] == 0);
  EXPECT(tg_events_screen_host(&t.m, t.rows + kept, keys.data(), n, eid2.data(), keep.data(), out2.data()) == TG_OK);
  EXPECT(out2[0] == 0 && out2[1] == 0 && eid2 == eid);
}

static void repack_case(int64_t rows_before, int kind) {
  std::vector<int64_t> key_of((size_t)rows_before);
  std::vector<uint64_t> keyless((size_t)((rows_before + 63) / 64), 0);
  std::vector<int32_t> remap((size_t)rows_before);
  int64_t rows_new = 0;
  for (int64_t r = 0; r < rows_before; ++r) {
    const bool bare = r == 0 || rnd() % 5 < 2;
    key_of[(size_t)r] = bare ? TG_IDMAP_EMPTY : (int64_t)(rnd() >> 2) + 1;
    if (bare && r) keyless[(size_t)(r >> 6)] |= 1ull << (r & 63);
    bool live = true;
    if (kind == 1) live = false;                  // everything but row 0 released
    if (kind == 2) live = r % 2 == 0;             // alternating
    if (kind == 3) live = !(r >= 60 && r < 130);  // a released block at a word edge
    if (r == 0) live = true;
    remap[(size_t)r] = live ? (int32_t)rows_new++ : -1;
  }
  std::vector<int64_t> got((size_t)rows_new, 77), want((size_t)rows_new);
  std::vector<uint64_t> bits((size_t)((rows_new + 63) / 64), ~0ull), wbits(bits.size(), 0);
  for (int64_t r = 0; r < rows_before; ++r) {
    const int64_t v = remap[(size_t)r];
    if (v < 0) continue;
    want[(size_t)v] = key_of[(size_t)r];
    if ((keyless[(size_t)(r >> 6)] >> (r & 63)) & 1ull) wbits[(size_t)(v >> 6)] |= 1ull << (v & 63);
  }
  EXPECT(tg_events_repack_host(key_of.data(), keyless.data(), remap.data(), rows_before, got.data(), bits.data(), rows_new) ==
         TG_OK);
  EXPECT(got == want && bits == wbits);
}

int main() {
  static const int64_t counts[] = {0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097};
  static const int64_t rows[] = {1, 64, 65, 2049};
  int cases = 0;
  for (int64_t n : counts)
    for (int mix = 0; mix < 6; ++mix, ++cases) screen_case(n, mix);
  for (int64_t r : rows)
    for (int kind = 0; kind < 4; ++kind, ++cases) repack_case(r, kind);
  // refusals: before anything is read
  Table t(10, 4);
  int64_t k[2] = {1, 2}, keep[2], out2[2];
  int32_t eid[2];
  EXPECT(tg_events_screen_host(&t.m, 0, k, 2, eid, keep, out2) == TG_EINVAL);
  EXPECT(tg_events_screen_host(&t.m, 15, k, 2, eid, keep, out2) == TG_EINVAL);  // rows > key_rows
  EXPECT(tg_events_screen_host(&t.m, 10, nullptr, 2, eid, keep, out2) == TG_EINVAL);
  EXPECT(tg_events_screen_host(&t.m, 10, k, 2, eid, keep, nullptr) == TG_EINVAL);
  EXPECT(tg_events_screen_host(nullptr, 10, k, 2, eid, keep, out2) == TG_EINVAL);
  EXPECT(tg_events_repack_host(nullptr, nullptr, nullptr, 1, nullptr, nullptr, 1) == TG_EINVAL);
  std::printf("%d cases, %d failures: %s\n", cases, failures, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
