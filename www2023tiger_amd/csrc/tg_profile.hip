// tg_profiler_* (include/tiger_hip.h): per-stage and per-kernel times of a profiled tg_stream_step.
#include "tg_profile.h"

namespace tg {
static const char* const kStageNames[ST_COUNT] = {
    "zero_flags", "sample_recent_edges", "unique_compact", "gather_right_memory", "apply_messages(gru)",
    "attn_centres+qconst", "attn_gemm_q", "attn_gemm_g", "attn_core(gather+softmax)", "attn_gemm_v", "attn_gemm_out",
    "attn_gemm_fc1", "attn_gemm_fc2", "dedup_positive", "writeback_phase0", "restarter_targets", "writeback_phase1",
    "eager_updater(gru)", "eager_query_rows(G)"};
thread_local KTimer* g_kt = nullptr;
thread_local int g_kt_slot = KT_NONE;
static const char* const kSlotNames[KT_COUNT] = {"collate(sampler+centres)", "attn_core", "fc1", "fc2", "updater", "query_rows",
                                                 "writeback", "gather"};
}  // namespace tg

using namespace tg;

extern "C" tg_profiler* tg_profiler_create(void) {
  tg_profiler* p = new tg_profiler();
  p->armed = false;
  for (int i = 0; i <= ST_COUNT; ++i)
    if (hipEventCreate(&p->ev[i]) != hipSuccess) {
      delete p;
      return nullptr;
    }
  for (int i = 0; i < KT_COUNT; ++i) {
    p->kt.name[i] = "";
    p->kt.hit[i] = false;
    for (int j = 0; j < 2; ++j)
      if (hipEventCreate(&p->kt.ev[i][j]) != hipSuccess) {
        delete p;
        return nullptr;
      }
  }
  return p;
}
extern "C" void tg_profiler_destroy(tg_profiler* p) {
  if (!p) return;
  for (int i = 0; i <= ST_COUNT; ++i) (void)hipEventDestroy(p->ev[i]);
  for (int i = 0; i < KT_COUNT; ++i)
    for (int j = 0; j < 2; ++j) (void)hipEventDestroy(p->kt.ev[i][j]);
  delete p;
}
extern "C" int tg_profiler_num_stages(void) { return ST_COUNT; }
extern "C" const char* tg_profiler_stage_name(int stage) {
  return (stage >= 0 && stage < ST_COUNT) ? kStageNames[stage] : "";
}
extern "C" int tg_profiler_read(tg_profiler* p, float* ms_out) {
  if (!p || !ms_out || !p->armed) return TG_EINVAL;
  hipError_t e = hipEventSynchronize(p->ev[ST_COUNT]);
  if (e != hipSuccess) {
    set_hip_error(e, "tg_profiler_read");
    return TG_EHIP;
  }
  for (int i = 0; i < ST_COUNT; ++i) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, p->ev[i], p->ev[i + 1]);
    ms_out[i] = ms;
  }
  return TG_OK;
}

extern "C" int tg_profiler_num_kernel_slots(void) { return KT_COUNT; }
extern "C" const char* tg_profiler_kernel_slot_name(int slot) { return (slot >= 0 && slot < KT_COUNT) ? kSlotNames[slot] : ""; }
// kernel-bound durations of the last profiled step: ms_out[slot] (< 0: no launch was made under the slot),
// names_out[slot] (nullable) = the launch expression of the timed kernel
extern "C" int tg_profiler_kernel_ms(tg_profiler* p, float* ms_out, const char** names_out) {
  if (!p || !ms_out || !p->armed) return TG_EINVAL;
  hipError_t e = hipEventSynchronize(p->ev[ST_COUNT]);
  if (e != hipSuccess) {
    set_hip_error(e, "tg_profiler_kernel_ms");
    return TG_EHIP;
  }
  for (int i = 0; i < KT_COUNT; ++i) {
    float ms = -1.f;
    if (p->kt.hit[i] && hipEventElapsedTime(&ms, p->kt.ev[i][0], p->kt.ev[i][1]) != hipSuccess) ms = -1.f;
    ms_out[i] = ms;
    if (names_out) names_out[i] = p->kt.hit[i] ? p->kt.name[i] : "";
  }
  return TG_OK;
}
