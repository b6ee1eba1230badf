// MXFP4 (OCP Microscaling v1.0: packed e2m1 values, one e8m0 scale byte per
// 32-element block, "floor" scale rule) quantise / dequantise kernels, K6/K7.
//
// Format (per tensor, rows = the last dimension, blocks of 32 elements, the
// last block of a row may be short and its missing elements count as +0):
//   amax  = max |x| over the block
//   code  = max(expfield(amax) - 2, 0)      (stored, one byte per block)
//   v     = x * 2^(127 - code)              (one fp32 multiply)
//   q     = rne_e2m1(v), saturating at +-6, sign of v kept (also on zero)
//   y     = rne_dst(float(q) * 2^(code - 127))
// Element 2j of a row is the low nibble of the row's byte j, element 2j + 1
// the high one; rows never share a byte (odd cols: the last high nibble is
// 0).  Every step is integer work on the bits or one correctly rounded IEEE
// fp32 operation, so the result is byte-identical to the torch CPU
// implementation in ops/mx.py.  2^-127 (code 0) is an f32 subnormal: this
// file must stay free of fast-math and of denormal flushing, like
// quant_fp8.h.  Scale code 255 dequantises its block to NaN.  Non-finite
// inputs are outside the contract (they poison their own block only).
//
// Work layout: a unit is kMxUnitBlocks = 256 consecutive blocks of ONE
// tensor; blocks take units interleaved over a capped grid and find their
// tensor with the unit walk, as the FP8 kernels do.
//
// Fast path (wide and payload bases 16B aligned, cols % 32 == 0): rows are
// whole blocks, so block b of the tensor is elements [32 b, 32 b + 32), its
// payload the 16 bytes at 16 b and its scale byte b: no row arithmetic.
// kMxLanes lanes own a block (see the constant).  Everything else takes the
// generic path of the same kernel: one lane per block, element by element;
// both elements of a payload byte belong to that lane, so no byte is ever
// shared between lanes.

#pragma once

#include "common.h"
#include "desc_ring.h"
#include "plan.h"
#include "quant_fp8.h"  // quant_mul / dequant_mul: the fma-fold fences
#include "unit_walk.h"

#include <algorithm>
#include <atomic>

// Lanes per block on the fast path.  2: a lane owns 16 consecutive elements,
// which is the wide-side access pattern of the FP8 kernels (2 or 4 16B loads
// per lane, adjacent lanes 32 / 64 B apart), one DPP-able __shfl_xor joins
// the two amax halves and the payload leaves as one 8B store per lane.  1: a
// lane owns the whole block (4 or 8 loads, lanes 64 / 128 B apart), one 16B
// payload store, no cross-lane traffic.  Measured on 1 GiB of bf16
// (profiles/mx_sync.log): quantise 5.56 TB/s either way, dequantise 4.84
// TB/s with 2 lanes against 4.09 with 1 (its 16B stores of adjacent lanes
// lie 64 B apart), so 2; the register count limits neither (occupancy 7 / 8).
#ifndef HIPSTORE_MX_LANES
#define HIPSTORE_MX_LANES 2
#endif
static constexpr uint32_t kMxLanes = HIPSTORE_MX_LANES;
static_assert(kMxLanes == 1 || kMxLanes == 2, "one or two lanes per block");
static constexpr uint32_t kMxLaneElems = kMxBlock / kMxLanes;
static constexpr uint32_t kMxPassBlocks = 256 / kMxLanes;
static constexpr uint32_t kMxPasses = kMxUnitBlocks / kMxPassBlocks;

typedef uint32_t v2u __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) v2u gv2u;
typedef __attribute__((address_space(1))) uint8_t gu8;

__device__ __forceinline__ uint32_t mx_abs_bits(float x) {
  return __float_as_uint(x) & 0x7fffffffu;
}

// e8m0 code of a block from the bits of its amax (finite: at most 252)
__device__ __forceinline__ uint32_t mx_scale_code(uint32_t amax_bits) {
  const uint32_t e = amax_bits >> 23;
  return e > 2u ? e - 2u : 0u;
}

// 2^(127 - code): exponent field 254 - code >= 1, always a normal number
__device__ __forceinline__ float mx_inv_scale(uint32_t code) {
  return __uint_as_float((254u - code) << 23);
}

// 2^(code - 127); code 0 is the subnormal 2^-127, code 255 is NaN
__device__ __forceinline__ float mx_scale(uint32_t code) {
  const uint32_t bits =
      code == 0u ? 0x00400000u : (code == 255u ? 0x7fc00000u : code << 23);
  return __uint_as_float(bits);
}

// eight already scaled values -> eight nibbles, element k in bits 4k..4k+3
__device__ __forceinline__ uint32_t mx_pack8(const float* v) {
  // v_cvt_scalef32_pk_fp4_f32 with a scale of 1: round to nearest even,
  // saturate at +-6, first operand into the low nibble of the chosen byte
  uint32_t w = 0;
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v[0], v[1], 1.0f, 0);
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v[2], v[3], 1.0f, 1);
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v[4], v[5], 1.0f, 2);
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, v[6], v[7], 1.0f, 3);
  return w;
}

// the reverse: eight nibbles -> their exact values as f32
__device__ __forceinline__ void mx_unpack8(uint32_t w, float* q) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2 a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 0);
  const f32x2 b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 1);
  const f32x2 c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 2);
  const f32x2 d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, 3);
  q[0] = a[0]; q[1] = a[1]; q[2] = b[0]; q[3] = b[1];
  q[4] = c[0]; q[5] = c[1]; q[6] = d[0]; q[7] = d[1];
}

// generic path: where block gb of the tensor sits
struct MxBlockPos {
  uint64_t eoff;  // element offset of its first column
  uint64_t poff;  // byte offset of its first payload byte
  uint32_t n;     // its elements, 1..32
};

__device__ __forceinline__ MxBlockPos mx_block_pos(const MxDesc& d,
                                                   uint32_t gb) {
  const uint32_t row = gb / d.nblk;
  const uint32_t b = gb - row * d.nblk;
  const uint32_t col0 = b * kMxBlock;
  const uint64_t row_bytes = ((uint64_t)d.cols + 1u) / 2u;
  return MxBlockPos{(uint64_t)row * d.cols + col0,
                    (uint64_t)row * row_bytes + b * (kMxBlock / 2u),
                    min(kMxBlock, d.cols - col0)};
}

template <typename T>
__device__ __forceinline__ void mx_quant_unit(const MxDesc& d,
                                              uint32_t local_unit) {
  gu8* scales = reinterpret_cast<gu8*>(d.scales);
  if (d.fast) {
    constexpr uint32_t NV = kMxLaneElems * sizeof(T) / 16u;  // loads per pass
    const uint32_t sub = threadIdx.x % kMxLanes;
    const uint32_t gb0 = local_unit * kMxUnitBlocks + threadIdx.x / kMxLanes;
    v4u raw[kMxPasses][NV];
    // all loads of the unit first, as in quant_fp8.h
#pragma unroll
    for (uint32_t p = 0; p < kMxPasses; ++p) {
      const uint32_t gb = gb0 + p * kMxPassBlocks;
#pragma unroll
      for (uint32_t k = 0; k < NV; ++k) raw[p][k] = v4u{0, 0, 0, 0};
      if (gb < d.nblocks) {
        const gv4u* s = reinterpret_cast<const gv4u*>(
            d.wide +
            ((uint64_t)gb * kMxBlock + sub * kMxLaneElems) * sizeof(T));
#pragma unroll
        for (uint32_t k = 0; k < NV; ++k) raw[p][k] = s[k];
      }
    }
#pragma unroll
    for (uint32_t p = 0; p < kMxPasses; ++p) {
      const uint32_t gb = gb0 + p * kMxPassBlocks;
      T e[kMxLaneElems];
      __builtin_memcpy(e, raw[p], sizeof(e));
      float x[kMxLaneElems];
      uint32_t amax = 0;
#pragma unroll
      for (uint32_t k = 0; k < kMxLaneElems; ++k) {
        x[k] = convert<T, float>(e[k]);
        amax = max(amax, mx_abs_bits(x[k]));
      }
      // the pair is live or dead as a whole, and the unit's descriptor is
      // uniform over the workgroup: all 64 lanes reach the shuffle
      if (kMxLanes == 2) amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1));
      const uint32_t code = mx_scale_code(amax);
      const float inv = mx_inv_scale(code);
#pragma unroll
      for (uint32_t k = 0; k < kMxLaneElems; ++k) x[k] = quant_mul(x[k], inv);
      uint32_t w[4] = {0, 0, 0, 0};  // two lanes per block fill two of them
#pragma unroll
      for (uint32_t k = 0; k < kMxLaneElems / 8u; ++k) w[k] = mx_pack8(x + 8 * k);
      if (gb < d.nblocks) {
        const uintptr_t out =
            d.payload + (uint64_t)gb * (kMxBlock / 2u) + sub * (kMxLaneElems / 2u);
        if (kMxLanes == 1) {
          *reinterpret_cast<gv4u*>(out) = v4u{w[0], w[1], w[2], w[3]};
        } else {
          *reinterpret_cast<gv2u*>(out) = v2u{w[0], w[1]};
        }
        if (sub == 0) scales[gb] = (uint8_t)code;
      }
    }
    return;
  }
  // generic: lane t of the workgroup takes block t of the unit
  const uint32_t gb = local_unit * kMxUnitBlocks + threadIdx.x;
  if (gb >= d.nblocks) return;
  const MxBlockPos pos = mx_block_pos(d, gb);
  const T* src = reinterpret_cast<const T*>(d.wide) + pos.eoff;
  gu8* payload = reinterpret_cast<gu8*>(d.payload) + pos.poff;
  float x[kMxBlock];
  uint32_t amax = 0;
#pragma unroll
  for (uint32_t c = 0; c < kMxBlock; ++c) {
    x[c] = c < pos.n ? convert<T, float>(src[c]) : 0.0f;
    amax = max(amax, mx_abs_bits(x[c]));
  }
  const uint32_t code = mx_scale_code(amax);
  const float inv = mx_inv_scale(code);
#pragma unroll
  for (uint32_t c = 0; c < kMxBlock; ++c) x[c] = quant_mul(x[c], inv);
#pragma unroll
  for (uint32_t k = 0; k < kMxBlock / 8u; ++k) {
    const uint32_t w = mx_pack8(x + 8 * k);
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      // byte 4k + j holds elements 8k + 2j and 8k + 2j + 1
      if (8u * k + 2u * j < pos.n) payload[4u * k + j] = (uint8_t)(w >> (8u * j));
    }
  }
  scales[gb] = (uint8_t)code;
}

template <typename T>
__device__ __forceinline__ void mx_dequant_unit(const MxDesc& d,
                                                uint32_t local_unit) {
  const gu8* scales = reinterpret_cast<const gu8*>(d.scales);
  if (d.fast) {
    constexpr uint32_t NV = kMxLaneElems * sizeof(T) / 16u;  // stores per pass
    constexpr uint32_t NW = kMxLaneElems / 8u;               // payload words
    const uint32_t sub = threadIdx.x % kMxLanes;
    const uint32_t gb0 = local_unit * kMxUnitBlocks + threadIdx.x / kMxLanes;
    uint32_t w[kMxPasses][4];  // two lanes per block use two of the words
    uint32_t code[kMxPasses];
#pragma unroll
    for (uint32_t p = 0; p < kMxPasses; ++p) {
      const uint32_t gb = gb0 + p * kMxPassBlocks;
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) w[p][k] = 0;
      code[p] = 0;
      if (gb < d.nblocks) {
        const uintptr_t in =
            d.payload + (uint64_t)gb * (kMxBlock / 2u) + sub * (kMxLaneElems / 2u);
        if (kMxLanes == 1) {
          const v4u r = *reinterpret_cast<const gv4u*>(in);
          w[p][0] = r[0]; w[p][1] = r[1]; w[p][2] = r[2]; w[p][3] = r[3];
        } else {
          const v2u r = *reinterpret_cast<const gv2u*>(in);
          w[p][0] = r[0]; w[p][1] = r[1];
        }
        // the lanes of a pair read one address: a single broadcast fetch
        code[p] = scales[gb];
      }
    }
#pragma unroll
    for (uint32_t p = 0; p < kMxPasses; ++p) {
      const uint32_t gb = gb0 + p * kMxPassBlocks;
      if (gb >= d.nblocks) continue;
      const float scale = mx_scale(code[p]);
      T e[kMxLaneElems];
#pragma unroll
      for (uint32_t k = 0; k < NW; ++k) {
        float q[8];
        mx_unpack8(w[p][k], q);
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j)
          e[8 * k + j] = convert<float, T>(dequant_mul(q[j], scale));
      }
      v4u out[NV];
      __builtin_memcpy(out, e, sizeof(e));
      gv4u* dst = reinterpret_cast<gv4u*>(
          d.wide + ((uint64_t)gb * kMxBlock + sub * kMxLaneElems) * sizeof(T));
#pragma unroll
      for (uint32_t k = 0; k < NV; ++k) dst[k] = out[k];
    }
    return;
  }
  const uint32_t gb = local_unit * kMxUnitBlocks + threadIdx.x;
  if (gb >= d.nblocks) return;
  const MxBlockPos pos = mx_block_pos(d, gb);
  T* dst = reinterpret_cast<T*>(d.wide) + pos.eoff;
  const gu8* payload = reinterpret_cast<const gu8*>(d.payload) + pos.poff;
  const float scale = mx_scale(scales[gb]);
  for (uint32_t c = 0; c < pos.n; c += 2u) {
    float q[8];
    mx_unpack8(payload[c / 2u], q);
    dst[c] = convert<float, T>(dequant_mul(q[0], scale));
    if (c + 1u < pos.n) dst[c + 1u] = convert<float, T>(dequant_mul(q[1], scale));
  }
}

template <bool DEQUANT>
__global__ void __launch_bounds__(256)
quant_mx_kernel(const MxDesc* __restrict__ descs, uint32_t ndescs,
                uint64_t total_units) {
  UnitWalk w;
  MxDesc d = {};
  for (uint64_t unit = blockIdx.x; unit < total_units; unit += gridDim.x) {
    if (unit >= w.next_prefix) walk_seek(w, d, descs, ndescs, unit);
    const uint32_t local = (uint32_t)(unit - d.units_prefix);
    // d is uniform over the workgroup: every wave takes one branch whole
    switch (static_cast<DType>(d.dtype)) {
      case DType::F32:
        if (DEQUANT) mx_dequant_unit<float>(d, local);
        else mx_quant_unit<float>(d, local);
        break;
      case DType::F16:
        if (DEQUANT) mx_dequant_unit<__half>(d, local);
        else mx_quant_unit<__half>(d, local);
        break;
      default:
        if (DEQUANT) mx_dequant_unit<__hip_bfloat16>(d, local);
        else mx_quant_unit<__hip_bfloat16>(d, local);
        break;
    }
  }
}

// launches of either kernel, counted apart from the FP8 ones
static std::atomic<uint64_t> g_mx_launches{0};

// One launch of either kernel, async on `stream`.  Grid cap (workgroups):
// the sweep on 1 GiB of bf16 (profiles/mx_sync.log) gained all the way up to
// 65536, about one unit per workgroup, and nothing beyond (262144): 5.55 TB/s
// quant and 4.80 dequant against 4.99 / 3.69 at 1024
template <bool DEQUANT>
static void launch_quant_mx(const Plan<MxDesc>& p, int device,
                            hipStream_t stream) {
  if (p.descs.empty()) return;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(
      p.units, env_u32("HIPSTORE_MX_GRID", 64, UINT32_MAX, 65536));
  stage_descs_and_launch(device, stream, p.descs, [&](const MxDesc* d) {
    hipLaunchKernelGGL(quant_mx_kernel<DEQUANT>, dim3(grid), dim3(256), 0,
                       stream, d, (uint32_t)p.descs.size(), p.units);
  });
  g_mx_launches.fetch_add(1, std::memory_order_relaxed);
}
