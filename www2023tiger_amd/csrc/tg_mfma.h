// What the three float32-MFMA units share (tg_gemm.hip: forward products, tg_gru.hip: the fused GRU cell, tg_gemm_tn.hip:
// weight gradients): the accumulator vector types, the k extent of a staged tile, the float4 staging helpers and the
// switch of the compiled-in phase stamps.  Included by those three units only, not by tg_dense.h.
#pragma once
#include "tg_dense.h"

namespace tg {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4m __attribute__((ext_vector_type(4)));

constexpr int BK = 32;
constexpr int LDK = BK + 1;

__device__ __forceinline__ float4 ldg4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void sts4(float* row, int k, float4 v) {
  row[k] = v.x;
  row[k + 1] = v.y;
  row[k + 2] = v.z;
  row[k + 3] = v.w;
}

// The stamps of the LDS-free kernels (k_gemm_ks16, k_gemm_direct, k_gru_direct16) are compiled in with -DTG_PHASE_TRACE only:
// in the production build they cost k_gemm_direct<11, 2, 2> its second block per CU (188 -> 256 registers).
#ifdef TG_PHASE_TRACE
#define TG_PT(...) __VA_ARGS__
#else
#define TG_PT(...)
#endif

}  // namespace tg
