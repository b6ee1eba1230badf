// Shared by every part of _hipstore: error check, tuning knobs, dtype codes
// with their conversions, and the 16-byte vector types of the copy paths.

#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>

#define HIP_CHECK(expr)                                                        \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      (void)hipGetLastError(); /* clear the sticky error so the caller's */    \
      /* process (torch's own error checks) is not poisoned */                 \
      throw std::runtime_error(std::string(#expr) + " failed: " +              \
                               hipGetErrorString(_e));                         \
    }                                                                          \
  } while (0)

// tuning knobs
//
// Every knob is an environment variable that is read on EVERY call, so a
// tuning sweep can vary it without a fresh process.  A value outside the
// accepted range means "use the default".
//
//   knob                  default                accepted
//   HIPSTORE_TILE         16384 (32768 when the  >= 4096
//                         launch moves > 512 MiB)
//   HIPSTORE_GRID         8192 general kernel,   >= 64
//                         65536 flat kernel
//   HIPSTORE_NT           1                      0 = plain stores
//   HIPSTORE_FLAT         1                      0 = never the flat kernel
//   HIPSTORE_FLAT_SPAN    16384                  4096 .. 16 MiB, multiple of
//                                                4096
//   HIPSTORE_FLAT_NTLOAD  1                      0 = plain loads
//   HIPSTORE_CAST_GRID    1024                   >= 64
//   HIPSTORE_CAST_V       8                      >= 1; 16 and above run the
//                                                16-element kernel
//   HIPSTORE_QUANT_GRID   65536                  >= 64
//   HIPSTORE_MX_GRID      65536                  >= 64
//
// The measurements behind each default stand next to the code that uses it.

static inline uint32_t env_u32(const char* name, uint32_t lo, uint32_t hi,
                               uint32_t dflt) {
  const char* e = getenv(name);
  if (!e) return dflt;
  const uint32_t v = (uint32_t)atoi(e);
  return (v >= lo && v <= hi) ? v : dflt;
}

static inline bool env_flag(const char* name, bool dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) != 0 : dflt;
}

// dtypes

enum class DType : int32_t { F32 = 0, F16 = 1, BF16 = 2 };

// every conversion goes through fp32 (the identity where it already is one)
__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(__half v) { return __half2float(v); }
__device__ __forceinline__ float to_f32(__hip_bfloat16 v) { return __bfloat162float(v); }
template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ __half from_f32<__half>(float v) { return __float2half(v); }
template <> __device__ __forceinline__ __hip_bfloat16 from_f32<__hip_bfloat16>(float v) {
  return __float2bfloat16(v);
}
template <typename SrcT, typename DstT>
__device__ __forceinline__ DstT convert(SrcT v) { return from_f32<DstT>(to_f32(v)); }

// 16-byte vectors

// uint4 is a class; the nontemporal builtins need a real vector type
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
// where addresses arrive as integers, naming the global address space lets
// the compiler emit global_load/global_store instead of generic flat ops
typedef __attribute__((address_space(1))) v4u gv4u;

template <bool NT, typename P>
__device__ __forceinline__ void store16(P p, v4u v) {
  if (NT) __builtin_nontemporal_store(v, p); else *p = v;
}

template <bool NT, typename P>
__device__ __forceinline__ v4u load16(P p) {
  return NT ? __builtin_nontemporal_load(p) : *p;
}
