// Per-node trajectory encoding: fold a step's source / destination embeddings into one float64 row per node.
// Reference: tiger/eval_utils.py:132-183 (encode_trajectory).  The reference reads h back per batch and walks the 2B
// events in a Python loop over a float64 numpy table.  Here one launch per batch applies the same sequence on the device:
// the applied sequence of a batch is its sources in index order (if used), then its destinations in index order (if used);
// one wavefront per position.  The wave of a node's FIRST position owns the node for this launch: it loads the float64
// row once, walks the later positions of the same id in order applying the operation in registers, and stores the row and
// the count once.  Every node has one owner, so no two waves touch a row: no atomics, and the result is bit for bit the
// sequential float64 loop's over the same h.
#include "tg_common.h"

namespace tg {

constexpr int TRAJ_NR = 4;  // float64 registers per lane and column chunk: d <= 256 is one chunk, a wider row takes several

struct TrajSeq {
  int64_t B, S;  // events of the batch; positions of the applied sequence
  int use_src;
  const int64_t *src, *dst;
};
__host__ __device__ __forceinline__ int64_t traj_id(const TrajSeq& s, int64_t q) {
  return (s.use_src && q < s.B) ? s.src[q] : s.dst[s.use_src ? q - s.B : q];
}
// (with the sources applied the sequence is cat[src, dst] and h's rows line up with it; without them it starts at row B)
__host__ __device__ __forceinline__ int64_t traj_row(const TrajSeq& s, int64_t q) { return s.use_src ? q : s.B + q; }
__host__ __device__ __forceinline__ bool traj_is_dst(const TrajSeq& s, int64_t q) { return !(s.use_src && q < s.B); }

// eval_utils.py:162-167,172-177: 'last' assigns; 'max' is numpy's maximum (a NaN on either side propagates); any other mode
// ADDS a source row and ASSIGNS a destination row
__host__ __device__ __forceinline__ double traj_apply(double r, double v, int mode, bool is_dst) {
  if (mode == TG_TRAJ_LAST || (mode == TG_TRAJ_SUM && is_dst)) return v;
  if (mode == TG_TRAJ_MAX) return (v > r || v != v) ? v : r;
  return r + v;
}

__global__ void __launch_bounds__(256) k_trajectory_accumulate(TrajSeq s, int d, const float* __restrict__ h,
                                                               const int64_t* __restrict__ offset_dev, int mode,
                                                               int64_t n_nodes, double* __restrict__ table,
                                                               double* __restrict__ counts, uint32_t* __restrict__ err) {
  const int lane = lane_id();
  const int64_t p = (int64_t)blockIdx.x * (blockDim.x / TG_WAVE) + threadIdx.x / TG_WAVE;
  if (p >= s.S) return;  // wave-uniform, as every branch on p and `my` below
  if (offset_dev) {
    s.src += *offset_dev;
    s.dst += *offset_dev;
  }
  const int64_t my = traj_id(s, p);
  if (my < 0 || my >= n_nodes) {
    if (lane == 0) atomicOr(err, TG_TRAJ_ERR_BAD_ID);
    return;
  }
  // the owner is the node's first position: 64 earlier ids per round
  for (int64_t base = 0; base < p; base += TG_WAVE) {
    const int64_t q = base + lane;
    if (__ballot(q < p && traj_id(s, q) == my)) return;
  }
  int64_t n = 0;
  for (int c0 = 0; c0 < d; c0 += TG_WAVE * TRAJ_NR) {
    double r[TRAJ_NR];
#pragma unroll
    for (int k = 0; k < TRAJ_NR; ++k) {
      const int c = c0 + k * TG_WAVE + lane;
      r[k] = c < d ? table[my * d + c] : 0.0;
    }
    n = 0;
    for (int64_t base = p - (p % TG_WAVE); base < s.S; base += TG_WAVE) {
      const int64_t q = base + lane;
      unsigned long long m = __ballot(q >= p && q < s.S && traj_id(s, q) == my);
      while (m) {  // the matching positions of this round in ascending order
        const int64_t hit = base + __ffsll(m) - 1;
        m &= m - 1;
        const float* row = h + traj_row(s, hit) * d;
        const bool is_dst = traj_is_dst(s, hit);
#pragma unroll
        for (int k = 0; k < TRAJ_NR; ++k) {
          const int c = c0 + k * TG_WAVE + lane;
          if (c < d) r[k] = traj_apply(r[k], (double)row[c], mode, is_dst);
        }
        ++n;
      }
    }
#pragma unroll
    for (int k = 0; k < TRAJ_NR; ++k) {
      const int c = c0 + k * TG_WAVE + lane;
      if (c < d) table[my * d + c] = r[k];
    }
  }
  if (lane == 0) counts[my] += (double)n;  // n ones added to an integer-valued double: exact
}

__global__ void k_trajectory_finish(int64_t n_nodes, int d, double* __restrict__ table, const double* __restrict__ counts) {
  const int64_t total = n_nodes * d;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
    table[i] /= counts[i / d] + 1e-7;
}

static bool traj_args_ok(int64_t B, int32_t d, int32_t mode, int64_t n_nodes) {
  return B >= 0 && B <= 0x3fffffffLL && d > 0 && n_nodes > 0 && n_nodes <= INT64_MAX / d &&
         (mode == TG_TRAJ_LAST || mode == TG_TRAJ_MAX || mode == TG_TRAJ_SUM);
}

}  // namespace tg

using namespace tg;

// ---- host twins -------------------------------------------------------------------------------------------------------
extern "C" int tg_trajectory_accumulate_host(int64_t B, int32_t d, const float* h, const int64_t* src, const int64_t* dst,
                                             const int64_t* offset, int32_t mode, int32_t use_src, int32_t use_dst,
                                             int64_t n_nodes, double* table, double* counts, uint32_t* err) {
  if (!traj_args_ok(B, d, mode, n_nodes)) return TG_EINVAL;
  TrajSeq s{B, (use_src ? B : 0) + (use_dst ? B : 0), use_src != 0, src, dst};
  if (s.S == 0) return TG_OK;
  if (!h || (use_src && !src) || (use_dst && !dst) || !table || !counts || !err) return TG_EINVAL;
  if (offset) {
    s.src += *offset;
    s.dst += *offset;
  }
  for (int64_t q = 0; q < s.S; ++q) {
    const int64_t id = traj_id(s, q);
    if (id < 0 || id >= n_nodes) {
      *err |= TG_TRAJ_ERR_BAD_ID;
      continue;
    }
    const float* row = h + traj_row(s, q) * d;
    const bool is_dst = traj_is_dst(s, q);
    for (int c = 0; c < d; ++c) table[id * d + c] = traj_apply(table[id * d + c], (double)row[c], mode, is_dst);
    counts[id] += 1.0;
  }
  return TG_OK;
}

extern "C" int tg_trajectory_finish_host(int64_t n_nodes, int32_t d, double* table, const double* counts) {
  if (n_nodes < 0 || d <= 0) return TG_EINVAL;
  if (n_nodes == 0) return TG_OK;
  if (!table || !counts) return TG_EINVAL;
  for (int64_t n = 0; n < n_nodes; ++n)
    for (int c = 0; c < d; ++c) table[n * d + c] /= counts[n] + 1e-7;
  return TG_OK;
}

// ---- device entries ---------------------------------------------------------------------------------------------------
extern "C" int tg_trajectory_accumulate(int64_t B, int32_t d, const float* h, const int64_t* src, const int64_t* dst,
                                        const int64_t* offset_dev, int32_t mode, int32_t use_src, int32_t use_dst,
                                        int64_t n_nodes, double* table, double* counts, uint32_t* err, void* stream) {
  if (!traj_args_ok(B, d, mode, n_nodes)) return TG_EINVAL;
  const TrajSeq s{B, (use_src ? B : 0) + (use_dst ? B : 0), use_src != 0, src, dst};
  if (s.S == 0) return TG_OK;
  if (!h || (use_src && !src) || (use_dst && !dst) || !table || !counts || !err) return TG_EINVAL;
  const int waves = 256 / TG_WAVE;
  hipLaunchKernelGGL(k_trajectory_accumulate, dim3((unsigned)((s.S + waves - 1) / waves)), dim3(256), 0, as_stream(stream), s,
                     (int)d, h, offset_dev, (int)mode, n_nodes, table, counts, err);
  return check_launch("tg_trajectory_accumulate");
}

extern "C" int tg_trajectory_finish(int64_t n_nodes, int32_t d, double* table, const double* counts, void* stream) {
  if (n_nodes < 0 || d <= 0) return TG_EINVAL;
  if (n_nodes == 0) return TG_OK;
  if (!table || !counts) return TG_EINVAL;
  hipLaunchKernelGGL(k_trajectory_finish, dim3(flat_grid(n_nodes * d, 256)), dim3(256), 0, as_stream(stream), n_nodes, (int)d,
                     table, counts);
  return check_launch("tg_trajectory_finish");
}
