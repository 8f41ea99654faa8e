// A stand-alone host program for a sanitizer run of the late-event host twin: tg_tcsr_merge_host over empty and
// full parents, empty batches, growth, equal times, signed zeros and infinities, every buffer allocated EXACTLY as
// tiger_hip.h sizes it, every result checked against a plain recomputation (per row: old row, then the owner's new entries in
// entry order, std::stable_sort on the times).  No GPU is touched.  Build and run:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude -Iwww2023tiger_amd/csrc \
//         tools/tcsr_merge_sanitize.cpp www2023tiger_amd/csrc/tg_append.hip www2023tiger_amd/csrc/tg_build.hip \
//         -o tcsr_merge_sanitize
//   ./tcsr_merge_sanitize            (exit status 0 and "ok": clean)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
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

// time of kind `mode`: 0 small integers (many ties), 1 one value, 2 signed zeros and +-1, 3 infinities and huge values
static double a_time(int mode) {
  static const double zeros[] = {-0.0, 0.0, -1.0, 1.0}, wide[] = {-INFINITY, INFINITY, 0.0, 1e300, -1e300, 3.0};
  switch (mode) {
    case 1: return 5.0;
    case 2: return zeros[rnd() % 4];
    case 3: return wide[rnd() % 6];
    default: return (double)(rnd() % 40) - 8.0;
  }
}

struct Tcsr {
  std::vector<int64_t> indptr;
  std::vector<double> ts;
  std::vector<int32_t> nbr, eid;
};

// a parent of P entries over N rows: random owners, ascending times per row
static Tcsr parent(int64_t N, int64_t P, int mode) {
  std::vector<int64_t> own((size_t)P);
  for (auto& o : own) o = (int64_t)(rnd() % (uint64_t)N);
  std::sort(own.begin(), own.end());
  Tcsr g;
  g.indptr.assign((size_t)N + 1, 0);
  for (int64_t o : own) g.indptr[(size_t)o + 1]++;
  for (int64_t v = 0; v < N; ++v) g.indptr[(size_t)v + 1] += g.indptr[(size_t)v];
  g.ts.resize((size_t)P);
  g.nbr.resize((size_t)P);
  g.eid.resize((size_t)P);
  for (int64_t p = 0; p < P; ++p) {
    g.ts[(size_t)p] = a_time(mode);
    g.nbr[(size_t)p] = (int32_t)(rnd() % (uint64_t)N);
    g.eid[(size_t)p] = (int32_t)rnd();
  }
  for (int64_t v = 0; v < N; ++v)
    std::sort(g.ts.begin() + g.indptr[(size_t)v], g.ts.begin() + g.indptr[(size_t)v + 1]);  // (-0.0 and 0.0 tie: either order)
  return g;
}

static void one_case(int64_t N0, int64_t N, int64_t P, int64_t n, int mode) {
  const Tcsr g = parent(N0, P, mode);
  std::vector<int64_t> src((size_t)n), dst((size_t)n), eid((size_t)n);
  std::vector<double> ts((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    src[(size_t)i] = (int64_t)(rnd() % (uint64_t)N);
    dst[(size_t)i] = rnd() % 8 == 0 ? src[(size_t)i] : (int64_t)(rnd() % (uint64_t)N);
    ts[(size_t)i] = a_time(mode);
    eid[(size_t)i] = (int64_t)(rnd() & 0x7fffffffu);
  }
  tg_tcsr t{N0, P, g.indptr.data(), g.ts.data(), g.nbr.data(), g.eid.data()};
  Tcsr out;
  out.indptr.assign((size_t)N + 1, -1);
  out.ts.resize((size_t)(P + 2 * n));
  out.nbr.resize((size_t)(P + 2 * n));
  out.eid.resize((size_t)(P + 2 * n));
  const int rc = tg_tcsr_merge_host(&t, N, n, src.data(), dst.data(), ts.data(), eid.data(), out.indptr.data(), out.ts.data(),
                                    out.nbr.data(), out.eid.data());
  EXPECT(rc == TG_OK);
  int64_t q = 0;
  for (int64_t v = 0; v < N; ++v) {  // the plain recomputation, row by row
    EXPECT(out.indptr[(size_t)v] == q);
    std::vector<double> rt;
    std::vector<int32_t> rn, re;
    if (v < N0)
      for (int64_t p = g.indptr[(size_t)v]; p < g.indptr[(size_t)v + 1]; ++p) {
        rt.push_back(g.ts[(size_t)p]);
        rn.push_back(g.nbr[(size_t)p]);
        re.push_back(g.eid[(size_t)p]);
      }
    for (int64_t j = 0; j < 2 * n; ++j) {
      const int64_t e = j >> 1, f = j & 1;
      if ((f ? dst[(size_t)e] : src[(size_t)e]) != v) continue;
      rt.push_back(ts[(size_t)e]);
      rn.push_back((int32_t)(f ? src[(size_t)e] : dst[(size_t)e]));
      re.push_back((int32_t)((uint32_t)eid[(size_t)e] | ((uint32_t)f << 31)));
    }
    std::vector<size_t> perm(rt.size());
    std::iota(perm.begin(), perm.end(), (size_t)0);
    std::stable_sort(perm.begin(), perm.end(), [&](size_t a, size_t b) { return rt[a] < rt[b]; });
    for (size_t k : perm) {
      EXPECT(std::memcmp(&out.ts[(size_t)q], &rt[k], 8) == 0 && out.nbr[(size_t)q] == rn[k] && out.eid[(size_t)q] == re[k]);
      ++q;
    }
  }
  EXPECT(out.indptr[(size_t)N] == q && q == P + 2 * n);
}

int main() {
  const int64_t shapes[][4] = {{1, 1, 0, 0},   {1, 1, 0, 3},    {5, 5, 0, 40},    {5, 5, 60, 0},     {7, 7, 1, 1},
                               {9, 9, 200, 70}, {9, 16, 200, 70}, {3, 64, 50, 300}, {300, 300, 40, 25}, {2, 2, 500, 500}};
  for (const auto& s : shapes)
    for (int mode = 0; mode < 4; ++mode) one_case(s[0], s[1], s[2], s[3], mode);
  // what the twin refuses: ids, eids, a NaN time, a shrinking node count
  {
    const Tcsr g = parent(4, 10, 0);
    tg_tcsr t{4, 10, g.indptr.data(), g.ts.data(), g.nbr.data(), g.eid.data()};
    std::vector<int64_t> ip(5);
    std::vector<double> ot(12);
    std::vector<int32_t> on(12), oe(12);
    const int64_t ok_id[1] = {1}, bad_id[1] = {4}, ok_e[1] = {7}, bad_e[1] = {(int64_t)1 << 31};
    const double ok_t[1] = {2.0}, nan_t[1] = {NAN};
    auto call = [&](const int64_t* s, const int64_t* e, const double* tt, int64_t n_out) {
      return tg_tcsr_merge_host(&t, n_out, 1, s, ok_id, tt, e, ip.data(), ot.data(), on.data(), oe.data());
    };
    EXPECT(call(ok_id, ok_e, ok_t, 4) == TG_OK);
    EXPECT(call(bad_id, ok_e, ok_t, 4) == TG_EINVAL);
    EXPECT(call(ok_id, bad_e, ok_t, 4) == TG_EINVAL);
    EXPECT(call(ok_id, ok_e, nan_t, 4) == TG_EINVAL);
    EXPECT(call(ok_id, ok_e, ok_t, 3) == TG_EINVAL);
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
