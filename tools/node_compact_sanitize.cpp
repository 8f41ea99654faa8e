// A stand-alone host program for a sanitizer run of the node-compaction host twins: tg_node_compact_plan_host,
// tg_node_rows_compact_host and tg_bitmap_compact_host on the word, wavefront and tile edges, every buffer allocated EXACTLY
// as tiger_hip.h sizes it, every result checked against a plain recomputation.  No GPU is touched.  Build and run:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude -Iwww2023tiger_amd/csrc \
//         tools/node_compact_sanitize.cpp www2023tiger_amd/csrc/tg_node_compact.hip -o node_compact_sanitize
//   ./node_compact_sanitize            (exit status 0 and "ok": clean)
#include <cstdint>
#include <cstdio>
#include <cstring>
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

// drop pattern `mode` over [0, N): 0 none, 1 one id, 2 the last id, 3 everything but 0, 4 alternating, 5 one word, 6 the ids
// each side of every edge
static std::vector<uint8_t> drops(int64_t N, int mode) {
  std::vector<uint8_t> d((size_t)N, 0);
  static const int64_t edges[] = {64, 128, 512, 2048, 32768, 131072};
  switch (mode) {
    case 1: if (N > 1) d[(size_t)(N / 2 > 0 ? N / 2 : 1)] = 1; break;
    case 2: if (N > 1) d[(size_t)N - 1] = 1; break;
    case 3: for (int64_t i = 1; i < N; ++i) d[(size_t)i] = 1; break;
    case 4: for (int64_t i = 1; i < N; i += 2) d[(size_t)i] = 1; break;
    case 5: for (int64_t i = 64; i < 128 && i < N; ++i) d[(size_t)i] = 1; break;
    case 6:
      for (int64_t e : edges)
        for (int64_t i = e - 1; i <= e + 1; ++i)
          if (i >= 1 && i < N) d[(size_t)i] = 1;
      break;
    default: break;
  }
  return d;
}

static void one_case(int64_t N, int64_t num_node, int mode) {
  const std::vector<uint8_t> drop = drops(N, mode);
  const int64_t W = (N + 63) / 64;
  std::vector<uint64_t> bits((size_t)W, 0);
  std::vector<int32_t> want_remap((size_t)N), want_old;
  for (int64_t i = 0; i < N; ++i) {
    if (drop[(size_t)i]) bits[(size_t)(i >> 6)] |= 1ull << (i & 63);
    want_remap[(size_t)i] = drop[(size_t)i] ? -1 : (int32_t)want_old.size();
    if (!drop[(size_t)i]) want_old.push_back((int32_t)i);
  }
  // a T-CSR over the kept ids below num_node: a hub row, sparse rows, long runs of empty rows
  std::vector<int32_t> alive;
  for (int64_t i = 1; i < num_node; ++i)
    if (!drop[(size_t)i]) alive.push_back((int32_t)i);
  std::vector<int64_t> indptr((size_t)num_node + 1, 0);
  std::vector<int32_t> nbr;
  if (!alive.empty()) {
    std::vector<int64_t> deg((size_t)num_node, 0);
    deg[(size_t)alive[0]] = 700;
    for (int k = 0; k < 300; ++k) deg[(size_t)alive[rnd() % alive.size()]] += 1 + rnd() % 3;
    for (int64_t i = 0; i < num_node; ++i) indptr[(size_t)i + 1] = indptr[(size_t)i] + deg[(size_t)i];
    nbr.resize((size_t)indptr[(size_t)num_node]);
    for (auto& v : nbr) v = alive[rnd() % alive.size()];
  }
  const int64_t P = (int64_t)nbr.size();
  std::vector<double> ts((size_t)P, 0.0);
  std::vector<int32_t> eid((size_t)P, 0);
  tg_tcsr g{num_node, P, indptr.data(), ts.data(), nbr.data(), eid.data()};
  std::vector<int32_t> remap((size_t)N), old_of((size_t)N), nbr_out((size_t)P);
  std::vector<int64_t> indptr_out((size_t)num_node + 1), out4(4);
  const int rc = tg_node_compact_plan_host(&g, bits.data(), W, N, remap.data(), old_of.data(), indptr_out.data(), nbr_out.data(),
                                           out4.data());
  EXPECT(rc == TG_OK);
  EXPECT(out4[0] == (int64_t)want_old.size() && out4[2] == 0 && out4[3] == -1);
  EXPECT(std::memcmp(remap.data(), want_remap.data(), (size_t)N * 4) == 0);
  EXPECT(std::memcmp(old_of.data(), want_old.data(), want_old.size() * 4) == 0);
  int64_t n_graph = 0;
  for (int64_t i = 0; i < num_node; ++i) {
    if (drop[(size_t)i]) continue;
    EXPECT(indptr_out[(size_t)n_graph] == indptr[(size_t)i]);
    ++n_graph;
  }
  EXPECT(out4[1] == n_graph && indptr_out[(size_t)n_graph] == P);
  for (int64_t p = 0; p < P; ++p) EXPECT(nbr_out[(size_t)p] == want_remap[(size_t)nbr[(size_t)p]]);

  // rows: the widths of the model's tables, every table with its own row count, eight in one call
  const int64_t n_new = out4[0];
  static const int64_t full[TG_NODE_ROWS_MAX] = {1, 4, 8, 16, 32, 688, 1024, 64}, slim[TG_NODE_ROWS_MAX] = {1, 4, 8, 16, 32, 48, 16, 64};
  const int64_t* widths = N > 40000 ? slim : full;  // (the long tables stay narrow: the run takes seconds)
  std::vector<std::vector<uint8_t>> src(TG_NODE_ROWS_MAX), dst(TG_NODE_ROWS_MAX);
  tg_node_rows tabs[TG_NODE_ROWS_MAX];
  for (int t = 0; t < TG_NODE_ROWS_MAX; ++t) {
    const int64_t rows_src = N - t < 1 ? 1 : N - t;  // tables of fewer rows keep a prefix of old_of
    int64_t rows_out = 0;
    while (rows_out < n_new && old_of[(size_t)rows_out] < rows_src) ++rows_out;
    src[t].resize((size_t)(rows_src * widths[t]));
    dst[t].assign((size_t)(rows_out * widths[t]), 0xEE);
    for (size_t i = 0; i < src[t].size(); ++i) src[t][i] = (uint8_t)(i * 131 + (i >> 8) + t);
    tabs[t] = tg_node_rows{src[t].data(), dst[t].data(), widths[t], rows_out, rows_src};
  }
  EXPECT(tg_node_rows_compact_host(tabs, TG_NODE_ROWS_MAX, old_of.data(), n_new) == TG_OK);
  for (int t = 0; t < TG_NODE_ROWS_MAX; ++t)
    for (int64_t j = 0; j < tabs[t].n_rows_out; ++j)
      EXPECT(std::memcmp(dst[t].data() + j * widths[t], src[t].data() + (int64_t)old_of[(size_t)j] * widths[t], (size_t)widths[t]) == 0);
  tg_node_rows nine[TG_NODE_ROWS_MAX + 1];
  for (int t = 0; t <= TG_NODE_ROWS_MAX; ++t) nine[t] = tabs[0];
  EXPECT(tg_node_rows_compact_host(nine, TG_NODE_ROWS_MAX + 1, old_of.data(), n_new) == TG_EINVAL);

  // bitmap: random bits over the old ids; the spare bits of the last output word are zero
  std::vector<uint64_t> in((size_t)W), out((size_t)((n_new + 63) / 64), ~0ull);
  for (auto& w : in) w = rnd();
  EXPECT(tg_bitmap_compact_host(in.data(), N, old_of.data(), n_new, out.data()) == TG_OK);
  for (int64_t j = 0; j < 64 * (int64_t)out.size(); ++j) {
    const bool got = (out[(size_t)(j >> 6)] >> (j & 63)) & 1ull;
    const int64_t o = j < n_new ? old_of[(size_t)j] : -1;
    EXPECT(got == (o >= 0 && ((in[(size_t)(o >> 6)] >> (o & 63)) & 1ull)));
  }
}

static void error_cases() {
  const int64_t N = 300, W = 5;
  std::vector<int64_t> indptr((size_t)N + 1, 0);
  for (int64_t i = 10; i <= N; ++i) indptr[(size_t)i] = i >= 200 ? 6 : (i >= 11 ? 3 : 0);  // rows 10 and 199 own 3 entries each
  std::vector<int32_t> nbr = {199, 150, 7, 10, 150, 8};
  std::vector<double> ts(6, 0.0);
  std::vector<int32_t> eid(6, 0), remap((size_t)N), old_of((size_t)N), nbr_out(6);
  std::vector<int64_t> indptr_out((size_t)N + 1), out4(4);
  tg_tcsr g{N, 6, indptr.data(), ts.data(), nbr.data(), eid.data()};
  auto run = [&](std::vector<int64_t> ids) {
    std::vector<uint64_t> bits((size_t)W, 0);
    for (int64_t i : ids) bits[(size_t)(i >> 6)] |= 1ull << (i & 63);
    EXPECT(tg_node_compact_plan_host(&g, bits.data(), W, N, remap.data(), old_of.data(), indptr_out.data(), nbr_out.data(),
                                     out4.data()) == TG_OK);
  };
  run({0, 5});
  EXPECT(out4[2] == TG_NODE_COMPACT_ID0 && out4[3] == 0);
  run({310, 305});
  EXPECT(out4[2] == TG_NODE_COMPACT_SPARE && out4[3] == 305);
  run({199, 10});
  EXPECT(out4[2] == TG_NODE_COMPACT_ROW && out4[3] == 10);
  run({150, 8});
  EXPECT(out4[2] == TG_NODE_COMPACT_NBR && out4[3] == 1);
  EXPECT(tg_node_compact_plan_host(&g, nullptr, W, N, remap.data(), old_of.data(), indptr_out.data(), nbr_out.data(), out4.data()) ==
         TG_EINVAL);
  std::vector<uint64_t> bits((size_t)W, 0);
  EXPECT(tg_node_compact_plan_host(&g, bits.data(), W, N - 1, remap.data(), old_of.data(), indptr_out.data(), nbr_out.data(),
                                   out4.data()) == TG_EINVAL);
  EXPECT(tg_node_compact_plan_host(&g, bits.data(), W - 1, N, remap.data(), old_of.data(), indptr_out.data(), nbr_out.data(),
                                   out4.data()) == TG_EINVAL);
}

int main() {
  static const int64_t sizes[] = {1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 2047, 2048, 2049, 32767, 32768, 32769,
                                  131071, 131072, 131073, 140000};
  int cases = 0;
  for (int64_t N : sizes)
    for (int mode = 0; mode <= 6; ++mode) {
      one_case(N, N, mode);
      if (N > 70) one_case(N, N - 70, mode);  // ids beyond the graph: assigned, never admitted
      cases += N > 70 ? 2 : 1;
    }
  error_cases();
  std::printf("%d cases, %d failures: %s\n", cases, failures, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
