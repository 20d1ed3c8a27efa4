// aa_common.hpp — constants and small device/host helpers shared by every translation unit (the
// optimizer kernels included; what only the model's units share is in aa_internal.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "adaptive_amd.h"
#include "aa_gemm.hpp"

namespace aa {

// Phase timestamps for tools/ktrace (an instrumented build only: -DAA_TS_ENABLE): thread 0 of each
// workgroup writes s_memrealtime (100 MHz) to aa_ts_buf[kernel][blockIdx.x][slot].  Empty in the
// product build.  Objects are compiled without relocatable device code, so each has its own copy of
// the pointer: a unit whose kernels use AA_TS defines a setter of its copy with ts_set_local, and
// aa_ts_setup (aa_kernels.hip) calls them all (that unit's own and the four k_lstm objects').
#ifdef AA_TS_ENABLE
static __device__ __attribute__((unused)) uint64_t* aa_ts_buf = nullptr;
static inline int ts_set_local(void* buf) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(aa_ts_buf), &buf, sizeof(buf)); }
__device__ __forceinline__ void aa_ts(int kid, int slot) {
  if (threadIdx.x == 0 && aa_ts_buf) {
    uint64_t* p = aa_ts_buf + ((size_t)kid * 2048 + blockIdx.x) * 16 + slot;
    p[0] = __builtin_amdgcn_s_memrealtime();
    p[8] = __builtin_amdgcn_s_memtime();  // shader clock: (memtime delta) / (realtime delta) = clock
  }
}
#define AA_TS(kid, slot) aa_ts(kid, slot)
// a value (e.g. a count) in slot 7 of the workgroup's record
#define AA_TSV(kid, v)                                                                      \
  do {                                                                                      \
    if (threadIdx.x == 0 && aa_ts_buf) aa_ts_buf[((size_t)(kid) * 2048 + blockIdx.x) * 16 + 7] = (v); \
  } while (0)
#else
#define AA_TS(kid, slot)
#define AA_TSV(kid, v)
#endif

constexpr int P = 49;          // attention width == 7x7 spatial locations (adaptive_attention.py:16-19)
constexpr int PP = 64;         // padded attention width (VWv row pitch, W_v rows)
constexpr int MAX_H = 1024;    // kernels keep h / s / u rows in LDS
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// accurate libm (expf / tanhf from the device library, no fast-math)
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float reluf_(float x) { return x < 0.f ? 0.f : x; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

}  // namespace aa

#define AA_TRY(expr)                           \
  do {                                         \
    hipError_t e_ = (expr);                    \
    if (e_ != hipSuccess) return (int)e_;      \
  } while (0)

static inline int aa_launch_status() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? AA_OK : (int)e;
}
static inline bool aa_al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// Host dispatch on the hidden size: calls f(std::integral_constant<int, H>{}) for the supported H
// (256, 512, 768, 1024; check_model admits no other), so a launch names its kernel as k<h.value>.
template <class F>
static inline void aa_for_hidden(int H, F&& f) {
  switch (H) {
    case 256: f(std::integral_constant<int, 256>{}); break;
    case 512: f(std::integral_constant<int, 512>{}); break;
    case 768: f(std::integral_constant<int, 768>{}); break;
    default: f(std::integral_constant<int, 1024>{}); break;
  }
}
