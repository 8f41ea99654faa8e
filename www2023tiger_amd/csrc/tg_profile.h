// The step profiler (tiger_hip.h: tg_profiler_*): one HIP event at every stage boundary of tg_stream_step and the
// kernel-bound timer of its main launches (tg_common.h: KTimer).  Not part of the C ABI.
#pragma once
#include "tg_common.h"

namespace tg {
enum Stage : int {
  ST_QUERIES = 0, ST_SAMPLE, ST_COMPACT, ST_GATHER, ST_UPDATE, ST_ATTN_PREP, ST_ATTN_Q, ST_ATTN_G, ST_ATTN_CORE,
  ST_ATTN_V, ST_ATTN_O, ST_ATTN_FC1, ST_ATTN_FC2, ST_DEDUP, ST_WRITE_RIGHT, ST_STORE_EVENTS, ST_WRITE_LEFT, ST_EAGER,
  ST_GTAB, ST_COUNT
};
}  // namespace tg

struct tg_profiler {
  hipEvent_t ev[tg::ST_COUNT + 1];
  bool armed;
  tg::KTimer kt;
};

static inline void prof_mark(tg_profiler* p, int i, hipStream_t st) {
  if (p) (void)hipEventRecord(p->ev[i], st);
}
