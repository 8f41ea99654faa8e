// A stand-alone host program for a sanitizer run of the nearest-neighbour host twin: tg_knn_rows_host at the
// edge shapes of tests/_knn_ref.py (Q 0, 1, 31..33, tile +- 1, two tiles + 1; C 0, 1, 31..33, tile - 1 .. tile + 1, two
// tiles + 1, 4097; d 4 .. 512; k 1, 10, 64) - every buffer allocated EXACTLY as tiger_hip.h sizes it (q: (Q - 1) ldq + d
// floats, c likewise, outputs [Q, k], the full matrix [Q, C]), optional pointers present and NULL, every list checked
// against a plain recomputation (double loop + std::sort on (score desc, column asc)).  No GPU is touched.  Build and run:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Iinclude \
//         -Iwww2023tiger_amd/csrc tools/knn_sanitize.cpp www2023tiger_amd/csrc/tg_knn.hip -o knn_sanitize
//   ./knn_sanitize            (exit status 0 and "ok": clean)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "tiger_hip.h"

namespace tg {
void set_hip_error(hipError_t, const char*) {}  // (tg_graph.hip's, which the twin never reaches)
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
static float small_float() {  // multiples of 1/8 in [-2, 2], a few non-finite
  const uint64_t r = rnd() % 400;
  if (r == 0) return NAN;
  if (r == 1) return INFINITY;
  if (r == 2) return -INFINITY;
  return (float)((int)(rnd() % 33) - 16) / 8.0f;
}

static void knn_case(int64_t Q, int64_t C, int32_t d, int32_t k, int64_t pad, bool with_opt) {
  const int64_t ldq = d + pad, ldc = d + 2 * pad;
  std::vector<float> q((size_t)(Q ? (Q - 1) * ldq + d : 0)), c((size_t)(C ? (C - 1) * ldc + d : 0));
  for (auto& x : q) x = small_float();
  for (auto& x : c) x = small_float();
  std::vector<int64_t> ids((size_t)C), excl((size_t)Q);
  std::vector<float> qs((size_t)Q), cs((size_t)C);
  std::vector<uint8_t> mask((size_t)C);
  for (int64_t j = 0; j < C; ++j) {
    ids[(size_t)j] = rnd() % 17 == 0 ? 0 : (int64_t)(rnd() % 50) + 1;  // few distinct ids: duplicates, and the padding id
    cs[(size_t)j] = (float)(1 << (rnd() % 4)) * (rnd() % 9 == 0 ? -0.5f : 0.25f);
    mask[(size_t)j] = rnd() % 6 != 0;
  }
  for (int64_t i = 0; i < Q; ++i) {
    excl[(size_t)i] = (int64_t)(rnd() % 60);
    qs[(size_t)i] = (float)(1 << (rnd() % 3));
  }
  std::vector<int64_t> out_ids((size_t)(Q * k), -7);
  std::vector<float> out_s((size_t)(Q * k), -7.f), S((size_t)(Q * C), -7.f);
  std::vector<int32_t> out_c((size_t)(Q * k), -7), nv((size_t)Q, -7);
  int64_t bad = 0;
  const int rc = tg_knn_rows_host(Q, C, d, k, q.data(), ldq, c.data(), ldc, with_opt ? ids.data() : nullptr,
                                  with_opt ? qs.data() : nullptr, with_opt ? cs.data() : nullptr,
                                  with_opt ? excl.data() : nullptr, with_opt ? mask.data() : nullptr, (int32_t)(rnd() % 5),
                                  out_ids.data(), out_s.data(), out_c.data(), nv.data(), &bad, with_opt ? S.data() : nullptr);
  EXPECT(rc == TG_OK);
  int64_t want_bad = 0;
  std::vector<std::pair<float, int32_t>> left;
  for (int64_t i = 0; i < Q; ++i) {
    left.clear();
    for (int64_t j = 0; j < C; ++j) {
      float s = 0.0f;
      for (int32_t kk = 0; kk < d; ++kk) s = fmaf(q[(size_t)(i * ldq + kk)], c[(size_t)(j * ldc + kk)], s);
      if (with_opt) {
        s = s * qs[(size_t)i];
        s = s * cs[(size_t)j];
        EXPECT(std::memcmp(&s, &S[(size_t)(i * C + j)], 4) == 0 || (s != s && S[(size_t)(i * C + j)] != S[(size_t)(i * C + j)]));
      }
      const int64_t id = with_opt ? ids[(size_t)j] : j + 1;
      if (id == 0 || (with_opt && (!mask[(size_t)j] || id == excl[(size_t)i]))) continue;
      if (!std::isfinite(s)) {
        ++want_bad;
        continue;
      }
      left.emplace_back(s, (int32_t)j);
    }
    std::sort(left.begin(), left.end(), [](const std::pair<float, int32_t>& x, const std::pair<float, int32_t>& y) {
      return x.first > y.first || (x.first == y.first && x.second < y.second);
    });
    EXPECT(nv[(size_t)i] == (int32_t)left.size());
    for (int32_t p = 0; p < k; ++p) {
      const size_t o = (size_t)(i * k + p);
      if ((size_t)p < left.size()) {
        const int32_t col = left[(size_t)p].second;
        EXPECT(out_c[o] == col && out_ids[o] == (with_opt ? ids[(size_t)col] : (int64_t)col + 1));
        EXPECT(std::memcmp(&out_s[o], &left[(size_t)p].first, 4) == 0);
      } else {
        EXPECT(out_c[o] == -1 && out_ids[o] == 0 && out_s[o] == -INFINITY);
      }
    }
  }
  EXPECT(bad == want_bad);
}

int main() {
  static const int64_t Qs[] = {0, 1, 31, 32, 33, TG_KNN_Q_TILE - 1, TG_KNN_Q_TILE + 1, 2 * TG_KNN_Q_TILE + 1};
  static const int64_t Cs[] = {0, 1, 31, 32, 33, TG_KNN_C_TILE - 1, TG_KNN_C_TILE, TG_KNN_C_TILE + 1, 2 * TG_KNN_C_TILE + 1, 4097};
  static const int32_t ds[] = {4, 8, 28, 32, 36, 172, 256, 512};
  static const int32_t ks[] = {1, 10, 64};
  int cases = 0;
  // a thinned cross product: every Q with every C, the widths and k cycling (each meets each Q and each C at least once
  // over the 80 pairs), wide rows only against few pairs' worth of work
  for (size_t a = 0; a < sizeof(Qs) / sizeof(*Qs); ++a)
    for (size_t b = 0; b < sizeof(Cs) / sizeof(*Cs); ++b, ++cases) {
      int32_t d = ds[(a + 3 * b) % 8];
      if (Qs[a] * Cs[b] > 300000 && d > 36) d = ds[(a + b) % 5];
      knn_case(Qs[a], Cs[b], d, ks[(a + b) % 3], (int64_t)((a + b) % 3), (a + b) % 4 != 0);
    }
  // refusals: before anything is read or written
  float x[8] = {0};
  int64_t oi[4] = {-7, -7, -7, -7}, bad = 0;
  float os[4];
  int32_t oc[4], nv[1] = {-7};
  auto call = [&](int64_t Q, int64_t C, int32_t d, int32_t k, const float* q, int64_t ldq, const float* c, int64_t ldc,
                  int32_t ns, int64_t* ids_out) {
    return tg_knn_rows_host(Q, C, d, k, q, ldq, c, ldc, nullptr, nullptr, nullptr, nullptr, nullptr, ns, ids_out, os, oc, nv,
                            &bad, nullptr);
  };
  EXPECT(call(-1, 1, 4, 4, x, 4, x, 4, 0, oi) == TG_EINVAL);
  EXPECT(call(1, -1, 4, 4, x, 4, x, 4, 0, oi) == TG_EINVAL);
  EXPECT(call(1, (int64_t)1 << 31, 4, 4, x, 4, x, 4, 0, oi) == TG_EINVAL);
  EXPECT(call(1, 1, 4, 4, x, 3, x, 4, 0, oi) == TG_EINVAL);
  EXPECT(call(1, 1, 4, 4, x, 4, x, 3, 0, oi) == TG_EINVAL);
  EXPECT(call(1, 1, 4, 0, x, 4, x, 4, 0, oi) == TG_EINVAL);
  EXPECT(call(1, 1, 4, TG_TOPK_MAX_K + 1, x, 4, x, 4, 0, oi) == TG_EINVAL);
  EXPECT(call(1, 1, 4, 4, x, 4, x, 4, -1, oi) == TG_EINVAL);
  EXPECT(call(1, 1, 4, 4, nullptr, 4, x, 4, 0, oi) == TG_EINVAL);
  EXPECT(call(1, 1, 4, 4, x, 4, nullptr, 4, 0, oi) == TG_EINVAL);
  EXPECT(call(1, 1, 4, 4, x, 4, x, 4, 0, nullptr) == TG_EINVAL);
  EXPECT(call(1, 1, 6, 4, x, 8, x, 8, 0, oi) == TG_EUNSUPPORTED);
  EXPECT(call(1, 1, 516, 4, x, 516, x, 516, 0, oi) == TG_EUNSUPPORTED);
  EXPECT(call(0, 1, 4, 4, nullptr, 4, nullptr, 4, 0, nullptr) == TG_OK);
  EXPECT(oi[0] == -7 && nv[0] == -7 && bad == 0);
  EXPECT(tg_knn_rows_workspace_bytes(1024, (int64_t)1 << 20, 64, 8) == (size_t)1024 * 8 * (64 * 8 + 8));
  std::printf("%d cases, %d failures: %s\n", cases, failures, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
