// The slot enumeration of the involved set of ONE (node, time) query by one wavefront, over a visitor - shared by
// tg_involved.hip (the visitor marks a byte per node) and tg_snapshot_refresh.hip (the visitor tests a bit and stops the
// query at the first hit), so that the two cannot disagree about what a query's embedding reads.
//
// involved(nid, t) = {nid}  +  the K sampler slots of (nid, t)  (padding id 0 included, as the sampler marks it)
//                    +  (two layers) the K slots of every hop-1 slot at the slot's float32 time (padding slots: node 0 at
//                       time 0).  The cut is prefix_end_group (strict float64).
//
// A visitor V has
//   void visit(int64_t v)   called by single lanes (divergent): node v is in the set; v may lie outside [0, num_node)
//   bool stop()             called by the whole wavefront between two searches: wave-uniform, true ends the query early.
//                           A visitor that never stops returns a constant false and the checks fold away.
#pragma once
#include <algorithm>
#include <vector>

#include "tg_sample.h"

namespace tg {

// recent_edges (graph.py:117-127).  Lane j holds hop-1 slot j in registers; the second hop is searched by G lanes per
// slot, 64 / G slots at a time (K <= G or G == 64).  All padding slots of a query are the same hop-2 query, searched once.
template <int G, class V>
__device__ __forceinline__ void involved_visit_edges(const tg_tcsr& g, int64_t nid, double t, int K, bool two, int lane,
                                                     V& vis) {
  constexpr int SPW = TG_WAVE / G;
  const int sub = lane % G, grp = lane / G;
  int64_t start;
  const int64_t end = prefix_end_group<64>(g, nid, t, &start, lane);
  // lane j: slot j of the query (left padded: node 0 at time 0); the slot time is the sampler's float32
  int64_t nb = 0;
  double tt = 0.0;
  const int64_t p = end - K + lane;
  if (lane < K && p >= start) {
    nb = g.nbr[p];
    tt = (double)(float)g.ts[p];
  }
  if (lane < K) vis.visit(nb);
  if (lane == 0) vis.visit(nid);
  if (!two || vis.stop()) return;  // (wave-uniform)
  const int64_t n1 = min((int64_t)K, end - start);
  for (int j = n1 < K ? (int)(K - n1 - 1) : 0; j < K; j += SPW) {  // the last padding slot stands for all of them
    const int s = j + grp;
    int64_t nb2 = __shfl(nb, s < K ? s : K - 1, TG_WAVE);
    const double t2 = __shfl(tt, s < K ? s : K - 1, TG_WAVE);
    if (s >= K) nb2 = -1;  // a group without a slot: no entries
    int64_t st2;
    const int64_t e2 = prefix_end_group<G>(g, nb2, t2, &st2, sub);
    for (int i = sub; i < K; i += G) {
      const int64_t p2 = e2 - K + i;
      if (s < K) vis.visit(p2 >= st2 ? (int64_t)g.nbr[p2] : (int64_t)0);
    }
    if (vis.stop()) return;
  }
}

// recent_nodes (graph.py:129-143): the scan of k_sample_recent_nodes (tg_sample.h), hop-1 slots parked in this
// wavefront's LDS (s_new, s_t: TG_WAVE elements each)
template <class V>
__device__ __forceinline__ void involved_visit_nodes(const tg_tcsr& g, int64_t nid, double t, int K, bool two, int lane,
                                                     int* s_new, float* s_t, V& vis) {
  int64_t start;
  const int64_t end = prefix_end_group<64>(g, nid, t, &start, lane);
  const int c = recent_nodes_scan(g, start, end, K, s_new, lane, [&](int slot, int64_t p, int) { s_t[slot] = (float)g.ts[p]; });
  __builtin_amdgcn_wave_barrier();
  int nb = 0;  // lane j < c: kept entry j; lanes c .. K-1: padding slots
  float tf = 0.f;
  if (lane < c) {
    nb = s_new[lane];
    tf = s_t[lane];
  }
  __builtin_amdgcn_wave_barrier();
  if (lane < K) vis.visit(nb);
  if (lane == 0) vis.visit(nid);
  if (!two || vis.stop()) return;  // (wave-uniform)
  const int n2 = c < K ? c + 1 : K;  // one padding slot stands for all of them
  for (int j = 0; j < n2; ++j) {
    const int64_t nb2 = __shfl(nb, j, TG_WAVE);
    const double t2 = (double)__shfl(tf, j, TG_WAVE);
    int64_t st2;
    const int64_t e2 = prefix_end_group<64>(g, nb2, t2, &st2, lane);
    const int c2 = recent_nodes_scan(g, st2, e2, K, s_new, lane, [&](int, int64_t, int v) { vis.visit(v); });
    if (c2 < K && lane == 0) vis.visit(0);
    if (vis.stop()) return;
  }
}

// ---- the host twins' enumeration: plain C++ over host T-CSR arrays ---------------------------------------------------------
// graph.py:117-143 on the host arrays: the entries of the K slots of (nid, t), in any order -> how many
static int host_tail(const tg_tcsr* g, int64_t nid, double t, int K, int strategy, std::vector<int64_t>& sel) {
  sel.clear();
  const int64_t lo = g->indptr[nid];
  const int64_t hi = std::lower_bound(g->ts + lo, g->ts + g->indptr[nid + 1], t) - g->ts;  // ts < t
  if (strategy == 0) {
    for (int64_t p = std::max(lo, hi - K); p < hi; ++p) sel.push_back(p);
  } else {  // the last occurrence of every distinct neighbour, the K most recent of those
    for (int64_t p = hi - 1; p >= lo && (int)sel.size() < K; --p) {
      bool seen = false;
      for (int64_t s : sel) seen = seen || g->nbr[s] == g->nbr[p];
      if (!seen) sel.push_back(p);
    }
  }
  return (int)sel.size();
}

// visit(v) for every node of involved(nid, t), nid in [0, num_node); visit returns true to end the query early -> whether
// it did.  hop1, hop2: scratch of the caller.
template <class Visit>
static bool host_involved_visit(const tg_tcsr* g, int64_t nid, double t, int K, int n_layers, int strategy,
                                std::vector<int64_t>& hop1, std::vector<int64_t>& hop2, Visit visit) {
  if (visit(nid)) return true;
  const int n1 = host_tail(g, nid, t, K, strategy, hop1);
  for (int64_t p : hop1)
    if (visit((int64_t)g->nbr[p])) return true;
  if (n1 < K && visit((int64_t)0)) return true;  // left padding: the sampler marks id 0
  if (n_layers != 2) return false;
  // data_loader.py:131: every slot is sampled again at its own float32 time, padding slots as node 0 at time 0
  for (int j = n1 < K ? -1 : 0; j < n1; ++j) {
    const int64_t v = j < 0 ? 0 : g->nbr[hop1[j]];
    const double t2 = j < 0 ? 0.0 : (double)(float)g->ts[hop1[j]];
    const int n2 = host_tail(g, v, t2, K, strategy, hop2);
    for (int64_t p : hop2)
      if (visit((int64_t)g->nbr[p])) return true;
    if (n2 < K && visit((int64_t)0)) return true;
  }
  return false;
}

}  // namespace tg
