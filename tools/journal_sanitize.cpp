// A stand-alone host program for a sanitizer run of the journal's host twins: tg_tcsr_rows_pack_host,
// tg_tcsr_rows_splice_host, tg_node_rows_scatter_host and tg_bitmap_scatter_host at the tile edges (0, 1, 2, 63, 64, 65, 2047,
// 2048, 2049 listed rows), with a hub row, empty rows, growth and every refusal of the splice - every buffer allocated EXACTLY
// as tiger_hip.h sizes it, every result checked against a plain recomputation.  No GPU is touched.  Build and run:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude -Iwww2023tiger_amd/csrc \
//         tools/journal_sanitize.cpp www2023tiger_amd/csrc/tg_journal.hip -o journal_sanitize
//   ./journal_sanitize            (exit status 0 and "ok": clean)
#include <algorithm>
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

struct Csr {
  std::vector<int64_t> indptr;
  std::vector<double> ts;
  std::vector<int32_t> nbr, eid;
  tg_tcsr view() {
    return tg_tcsr{(int64_t)indptr.size() - 1, (int64_t)ts.size(), indptr.data(), ts.data(), nbr.data(), eid.data()};
  }
};

// rows of 0 to 6 entries, a third of them empty, row `hub` with 5000
static Csr make(int64_t N, int64_t hub, bool empty) {
  Csr g;
  g.indptr.assign((size_t)N + 1, 0);
  for (int64_t v = 0; v < N; ++v) {
    const int64_t deg = empty ? 0 : (v == hub ? 5000 : (rnd() % 3 == 0 ? 0 : 1 + (int64_t)(rnd() % 6)));
    g.indptr[(size_t)v + 1] = g.indptr[(size_t)v] + deg;
  }
  const size_t P = (size_t)g.indptr[(size_t)N];
  g.ts.resize(P);
  g.nbr.resize(P);
  g.eid.resize(P);
  for (size_t p = 0; p < P; ++p) {
    g.ts[p] = (double)p * 0.5;
    g.nbr[p] = (int32_t)(rnd() % (uint64_t)N);
    g.eid[p] = (int32_t)(uint32_t)rnd();
  }
  return g;
}

// D distinct ascending ids of [0, N), the first and the last id among them when D >= 2
static std::vector<int32_t> pick(int64_t N, int64_t D) {
  std::vector<uint8_t> in((size_t)N, 0);
  int64_t have = 0;
  if (D >= 1) in[0] = 1, ++have;
  if (D >= 2) in[(size_t)N - 1] = 1, ++have;
  while (have < D) {
    const size_t v = (size_t)(rnd() % (uint64_t)N);
    if (!in[v]) in[v] = 1, ++have;
  }
  std::vector<int32_t> rows;
  for (int64_t v = 0; v < N; ++v)
    if (in[(size_t)v]) rows.push_back((int32_t)v);
  return rows;
}

static void pack_splice_case(int64_t N_old, int64_t N_new, int64_t D, bool empty_old) {
  Csr old = make(N_old, N_old > 1200 ? 1000 : -1, empty_old);
  Csr fresh = make(N_new, N_new > 1200 ? 1000 : -1, false);  // the rows the listed ids take
  const std::vector<int32_t> rows = pick(N_new, D);
  tg_tcsr go = old.view(), gf = fresh.view();
  // pack the listed rows of `fresh`: outputs sized exactly
  int64_t n_pack = 0;
  for (int32_t v : rows) n_pack += fresh.indptr[(size_t)v + 1] - fresh.indptr[(size_t)v];
  std::vector<int64_t> off((size_t)D + 1);
  std::vector<double> pts((size_t)n_pack);
  std::vector<int32_t> pnbr((size_t)n_pack), peid((size_t)n_pack);
  EXPECT(tg_tcsr_rows_pack_host(&gf, rows.data(), D, off.data(), pts.data(), pnbr.data(), peid.data()) == TG_OK);
  EXPECT(off[0] == 0 && off[(size_t)D] == n_pack);
  for (int64_t j = 0; j < D; ++j) {
    const int64_t b = fresh.indptr[(size_t)rows[(size_t)j]], len = fresh.indptr[(size_t)rows[(size_t)j] + 1] - b;
    EXPECT(off[(size_t)j + 1] - off[(size_t)j] == len);
    EXPECT(len == 0 || std::memcmp(pts.data() + off[(size_t)j], fresh.ts.data() + b, (size_t)len * 8) == 0);
    EXPECT(len == 0 || std::memcmp(pnbr.data() + off[(size_t)j], fresh.nbr.data() + b, (size_t)len * 4) == 0);
    EXPECT(len == 0 || std::memcmp(peid.data() + off[(size_t)j], fresh.eid.data() + b, (size_t)len * 4) == 0);
  }
  // splice them into `old`: outputs sized as the header says (old entries + packed entries)
  const int64_t cap = go.num_entry + n_pack;
  std::vector<int64_t> indptr((size_t)N_new + 1), out3(3);
  std::vector<double> ts((size_t)cap);
  std::vector<int32_t> nbr((size_t)cap), eid((size_t)cap);
  EXPECT(tg_tcsr_rows_splice_host(&go, N_new, rows.data(), D, off.data(), n_pack, pts.data(), pnbr.data(), peid.data(),
                                  indptr.data(), ts.data(), nbr.data(), eid.data(), out3.data()) == TG_OK);
  EXPECT(out3[1] == 0 && out3[2] == -1 && out3[0] == indptr[(size_t)N_new] && indptr[0] == 0);
  size_t j = 0;
  for (int64_t v = 0; v < N_new; ++v) {
    const bool hit = j < rows.size() && rows[j] == v;
    const Csr& from = hit ? fresh : old;
    const int64_t b = hit || v < N_old ? from.indptr[(size_t)v] : 0, e = hit || v < N_old ? from.indptr[(size_t)v + 1] : 0;
    const int64_t q = indptr[(size_t)v];
    EXPECT(indptr[(size_t)v + 1] - q == e - b);
    if (indptr[(size_t)v + 1] - q != e - b) break;
    EXPECT(e == b || std::memcmp(ts.data() + q, from.ts.data() + b, (size_t)(e - b) * 8) == 0);
    EXPECT(e == b || std::memcmp(nbr.data() + q, from.nbr.data() + b, (size_t)(e - b) * 4) == 0);
    EXPECT(e == b || std::memcmp(eid.data() + q, from.eid.data() + b, (size_t)(e - b) * 4) == 0);
    j += hit;
  }
}

static void splice_refusals() {
  Csr old = make(300, -1, false), fresh = make(300, -1, false);
  tg_tcsr go = old.view(), gf = fresh.view();
  const std::vector<int32_t> rows = pick(300, 65);
  int64_t n_pack = 0;
  for (int32_t v : rows) n_pack += fresh.indptr[(size_t)v + 1] - fresh.indptr[(size_t)v];
  std::vector<int64_t> off(66);
  std::vector<double> pts((size_t)n_pack);
  std::vector<int32_t> pnbr((size_t)n_pack), peid((size_t)n_pack);
  EXPECT(tg_tcsr_rows_pack_host(&gf, rows.data(), 65, off.data(), pts.data(), pnbr.data(), peid.data()) == TG_OK);
  std::vector<int64_t> indptr(301), out3(3);
  std::vector<double> ts((size_t)(go.num_entry + n_pack));
  std::vector<int32_t> nbr(ts.size()), eid(ts.size());
  auto run = [&](const tg_tcsr& g, const std::vector<int32_t>& r, const std::vector<int64_t>& o) {
    EXPECT(tg_tcsr_rows_splice_host(&g, 300, r.data(), (int64_t)r.size(), o.data(), n_pack, pts.data(), pnbr.data(), peid.data(),
                                    indptr.data(), ts.data(), nbr.data(), eid.data(), out3.data()) == TG_OK);
  };
  std::vector<int32_t> r = rows;
  std::swap(r[20], r[40]);
  run(go, r, off);
  EXPECT(out3[1] == TG_SPLICE_ROWS && out3[2] == 21);
  r = rows;
  r[64] = 300;
  run(go, r, off);
  EXPECT(out3[1] == TG_SPLICE_ROWS && out3[2] == 64);
  std::vector<int64_t> o = off;
  o[0] = 1;
  run(go, rows, o);
  EXPECT(out3[1] == TG_SPLICE_OFF && out3[2] == 0);
  o = off;
  o[30] = o[29] - 1;
  o[50] = o[49] - 1;
  run(go, rows, o);
  EXPECT(out3[1] == TG_SPLICE_OFF && out3[2] == 30);
  o = off;
  o[65] += 1;
  run(go, rows, o);
  EXPECT(out3[1] == TG_SPLICE_OFF && out3[2] == 65);
  o = off;
  o[10] = 1ll << 40;  // offsets that are no index of anything
  o[11] = -5;
  run(go, rows, o);
  EXPECT(out3[1] == TG_SPLICE_OFF && out3[2] == 11);
  r.assign(rows.begin(), rows.end() - 1);  // a truncated off
  o.assign(off.begin(), off.end() - 1);
  if (o.back() != n_pack) {
    run(go, r, o);
    EXPECT(out3[1] == TG_SPLICE_OFF && out3[2] == 64);
  }
  Csr bad = old;
  bad.indptr[100] = bad.indptr[101] + 1;
  tg_tcsr gb = bad.view();
  run(gb, rows, off);
  EXPECT(out3[1] == TG_SPLICE_PTR && out3[2] == 100);
  EXPECT(tg_tcsr_rows_splice_host(&go, 299, rows.data(), 65, off.data(), n_pack, pts.data(), pnbr.data(), peid.data(), indptr.data(),
                                  ts.data(), nbr.data(), eid.data(), out3.data()) == TG_EINVAL);
  EXPECT(tg_tcsr_rows_splice_host(&go, 300, rows.data(), 65, nullptr, n_pack, pts.data(), pnbr.data(), peid.data(), indptr.data(),
                                  ts.data(), nbr.data(), eid.data(), out3.data()) == TG_EINVAL);
  EXPECT(tg_tcsr_rows_pack_host(&gf, rows.data(), 301, off.data(), pts.data(), pnbr.data(), peid.data()) == TG_EINVAL);
}

static void scatter_case(int64_t n_dst, int64_t D) {
  const std::vector<int32_t> ids = D ? pick(n_dst, D) : std::vector<int32_t>();
  static const int64_t widths[TG_NODE_ROWS_MAX] = {1, 4, 8, 16, 32, 688, 48, 64};
  std::vector<std::vector<uint8_t>> src(TG_NODE_ROWS_MAX), dst(TG_NODE_ROWS_MAX), want(TG_NODE_ROWS_MAX);
  tg_node_rows tabs[TG_NODE_ROWS_MAX];
  for (int t = 0; t < TG_NODE_ROWS_MAX; ++t) {
    const int64_t rows_dst = n_dst - t < 1 ? 1 : n_dst - t;  // a table of fewer rows: the ids beyond it store nothing
    const int64_t rows_src = std::max<int64_t>(D - t, 0);    // a table of fewer packed rows reads a prefix of ids
    src[t].resize((size_t)(rows_src * widths[t]));
    dst[t].assign((size_t)(rows_dst * widths[t]), 0xEE);
    for (size_t i = 0; i < src[t].size(); ++i) src[t][i] = (uint8_t)(i * 131 + (i >> 8) + t);
    want[t] = dst[t];
    for (int64_t j = 0; j < rows_src; ++j)
      if (ids[(size_t)j] < rows_dst)
        std::memcpy(want[t].data() + (int64_t)ids[(size_t)j] * widths[t], src[t].data() + j * widths[t], (size_t)widths[t]);
    tabs[t] = tg_node_rows{src[t].data(), dst[t].data(), widths[t], rows_dst, rows_src};
  }
  EXPECT(tg_node_rows_scatter_host(tabs, TG_NODE_ROWS_MAX, ids.data(), D) == TG_OK);
  for (int t = 0; t < TG_NODE_ROWS_MAX; ++t) EXPECT(dst[t] == want[t]);
  tg_node_rows nine[TG_NODE_ROWS_MAX + 1];
  for (int t = 0; t <= TG_NODE_ROWS_MAX; ++t) nine[t] = tabs[0];
  EXPECT(tg_node_rows_scatter_host(nine, TG_NODE_ROWS_MAX + 1, ids.data(), D) == TG_EINVAL);

  // bits: random words, the listed bits replaced, every other bit - the spare ones included - as it was
  const int64_t W = (n_dst + 63) / 64;
  std::vector<uint64_t> bits((size_t)W), was;
  for (auto& w : bits) w = rnd();
  if (n_dst % 64) bits[(size_t)W - 1] &= (1ull << (n_dst % 64)) - 1ull;
  was = bits;
  std::vector<uint8_t> flags((size_t)D);
  for (auto& f : flags) f = (uint8_t)(rnd() % 3);
  EXPECT(tg_bitmap_scatter_host(flags.data(), ids.data(), D, bits.data(), n_dst) == TG_OK);
  size_t j = 0;
  for (int64_t i = 0; i < 64 * W; ++i) {
    const bool got = (bits[(size_t)(i >> 6)] >> (i & 63)) & 1ull, old = (was[(size_t)(i >> 6)] >> (i & 63)) & 1ull;
    const bool hit = j < ids.size() && ids[j] == i;
    EXPECT(got == (hit ? flags[j] != 0 : old));
    j += hit;
  }
}

int main() {
  static const int64_t counts[] = {0, 1, 2, 63, 64, 65, 2047, 2048, 2049};
  int cases = 0;
  for (int64_t D : counts) {
    pack_splice_case(2100, 2100, D, false);
    pack_splice_case(2100, 2230, D, false);  // growth: listed and untouched new ids
    pack_splice_case(70, D > 70 ? 2100 : 70, std::min<int64_t>(D, 2100), true);  // an empty old graph
    scatter_case(2100, D);
    cases += 4;
  }
  pack_splice_case(2100, 2100, 2100, false);  // every row listed
  scatter_case(129, 5);
  scatter_case(66, 66);
  splice_refusals();
  std::printf("%d cases, %d failures: %s\n", cases + 3, failures, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
