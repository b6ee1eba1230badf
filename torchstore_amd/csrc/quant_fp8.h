// Block-scaled FP8 (OCP e4m3) quantise / dequantise kernels — K4/K5.
//
// Format (per tensor, rows = the last dimension, blocks of 128 elements, the
// last block of a row may be short):
//   amax  = max(max|x| over the block, 2^-96)
//   scale = amax / 448            (stored, f32, index = row * nblk + block)
//   q     = rne_e4m3(clamp(x * (448 / amax), -448, 448))
//   y     = rne_dst(float(q) * scale)
// Every step is one correctly rounded IEEE fp32 operation, so the result is
// byte-identical to the torch CPU implementation in ops/quant.py.  This file
// must stay free of fast-math: the divides have to be the IEEE ones.
// Non-finite inputs are outside the contract (a NaN or Inf in a block makes
// that block's payload and scale unspecified; other blocks are unaffected).
//
// Work layout: 8 lanes own one 128-element block, so a wave covers 8 blocks
// and a 256-thread workgroup 32 per pass.  A unit is kQuantPasses passes of
// one workgroup over consecutive blocks of ONE tensor; blocks take units
// interleaved over a capped grid and find their tensor like copy_flat_kernel
// (search once, then walk forward).
//
// Fast path (base pointers 16B aligned, cols % 16 == 0): a lane owns 16
// consecutive elements — 2 (bf16/f16) or 4 (f32) 16B accesses on the wide
// side and one 16B access on the payload side; short last blocks are
// predicated against cols.  Everything else takes the generic path of the
// same kernel: the 8 lanes stride over the block element by element.

#pragma once

#include "common.h"
#include "desc_ring.h"
#include "plan.h"
#include "unit_walk.h"

#include <algorithm>
#include <atomic>

static constexpr float kFp8Max = 448.0f;
static constexpr float kAmaxFloor = 0x1p-96f;

// 16 elements of T as raw 16B vectors (sizeof(T) of them)
template <typename T>
struct QuantRaw {
  v4u q[sizeof(T)];
};

__device__ __forceinline__ float group8_max(float a) {
  a = fmaxf(a, __shfl_xor(a, 1));
  a = fmaxf(a, __shfl_xor(a, 2));
  a = fmaxf(a, __shfl_xor(a, 4));
  return a;
}

// float(q) * scale as an fp32 value of its own.  Left to itself the compiler
// folds the multiply and the narrowing to f16 into v_fma_mixlo_f16 (x * y + 0
// rounded once): that turns a -0 product into +0 and skips the fp32 rounding
// of the recipe.  The empty asm keeps the product out of that fold.
__device__ __forceinline__ float dequant_mul(float q, float scale) {
  float y = q * scale;
  asm("" : "+v"(y));
  return y;
}

// same for the widening side: x * inv must not become v_fma_mix_f32 with a +0
// addend (a -0 input would quantise to +0)
__device__ __forceinline__ float quant_mul(float x, float inv) {
  float y = x * inv;
  asm("" : "+v"(y));
  return y;
}

__device__ __forceinline__ float quant_scaled(float x, float inv) {
  return fminf(fmaxf(quant_mul(x, inv), -kFp8Max), kFp8Max);
}

// block index -> (element offset of the block's first column, first column)
__device__ __forceinline__ void quant_block_pos(const QuantDesc& d,
                                                uint32_t gb, uint64_t& eoff,
                                                uint32_t& col0) {
  const uint32_t row = gb / d.nblk;
  col0 = (gb - row * d.nblk) * kQuantBlock;
  eoff = (uint64_t)row * d.cols + col0;
}

template <typename T>
__device__ __forceinline__ void quant_unit(const QuantDesc& d,
                                           uint32_t local_unit) {
  const uint32_t group = threadIdx.x >> 3;
  const uint32_t gl = threadIdx.x & 7u;
  const uint32_t gb0 = local_unit * kQuantUnitBlocks + group;
  float* scales = reinterpret_cast<float*>(d.scales);
  if (d.fast) {
    QuantRaw<T> raw[kQuantPasses];
    uint64_t eoff[kQuantPasses];
    bool live[kQuantPasses];
    // all loads of the unit first: 64 B (bf16/f16) or 128 B (f32) in flight
    // per lane before the first dependent instruction
#pragma unroll
    for (uint32_t p = 0; p < kQuantPasses; ++p) {
      const uint32_t gb = gb0 + p * 32u;
      uint32_t col0 = 0;
      eoff[p] = 0;
      live[p] = false;
      if (gb < d.nblocks) {
        quant_block_pos(d, gb, eoff[p], col0);
        const uint32_t c = col0 + gl * 16u;
        live[p] = c < d.cols;  // cols % 16 == 0: all 16 elements or none
        eoff[p] += gl * 16u;
      }
#pragma unroll
      for (uint32_t k = 0; k < sizeof(T); ++k) raw[p].q[k] = v4u{0, 0, 0, 0};
      if (live[p]) {
        const gv4u* s = reinterpret_cast<const gv4u*>(
            d.wide + eoff[p] * sizeof(T));
#pragma unroll
        for (uint32_t k = 0; k < sizeof(T); ++k) raw[p].q[k] = s[k];
      }
    }
#pragma unroll
    for (uint32_t p = 0; p < kQuantPasses; ++p) {
      const uint32_t gb = gb0 + p * 32u;
      T e[16];
      __builtin_memcpy(e, &raw[p], sizeof(e));
      float x[16];
      float amax = 0.0f;
#pragma unroll
      for (uint32_t k = 0; k < 16; ++k) {
        x[k] = convert<T, float>(e[k]);
        amax = fmaxf(amax, fabsf(x[k]));
      }
      // dead lanes hold zeros, so they add nothing to the block's amax
      amax = fmaxf(group8_max(amax), kAmaxFloor);
      const float inv = kFp8Max / amax;
      v4u out;
#pragma unroll
      for (uint32_t w = 0; w < 4; ++w) {
        int packed = 0;
        packed = __builtin_amdgcn_cvt_pk_fp8_f32(
            quant_scaled(x[4 * w], inv), quant_scaled(x[4 * w + 1], inv),
            packed, false);
        packed = __builtin_amdgcn_cvt_pk_fp8_f32(
            quant_scaled(x[4 * w + 2], inv), quant_scaled(x[4 * w + 3], inv),
            packed, true);
        out[w] = (uint32_t)packed;
      }
      if (live[p]) {
        *reinterpret_cast<gv4u*>(d.payload + eoff[p]) = out;
      }
      if (gl == 0 && gb < d.nblocks) scales[gb] = amax / kFp8Max;
    }
    return;
  }
  // generic: lane gl of the group takes elements gl, gl+8, ... of the block
  const T* src = reinterpret_cast<const T*>(d.wide);
  uint8_t* payload = reinterpret_cast<uint8_t*>(d.payload);
  for (uint32_t p = 0; p < kQuantPasses; ++p) {
    const uint32_t gb = gb0 + p * 32u;
    uint64_t eoff = 0;
    uint32_t n = 0;  // elements of this block; 0 = no block for this group
    if (gb < d.nblocks) {
      uint32_t col0;
      quant_block_pos(d, gb, eoff, col0);
      n = min(kQuantBlock, d.cols - col0);
    }
    float x[16];
    float amax = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
      const uint32_t c = gl + 8u * k;
      x[k] = c < n ? convert<T, float>(src[eoff + c]) : 0.0f;
      amax = fmaxf(amax, fabsf(x[k]));
    }
    amax = fmaxf(group8_max(amax), kAmaxFloor);
    const float inv = kFp8Max / amax;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
      const uint32_t c = gl + 8u * k;
      const float v = quant_scaled(x[k], inv);
      const int packed = __builtin_amdgcn_cvt_pk_fp8_f32(v, v, 0, false);
      if (c < n) payload[eoff + c] = (uint8_t)(packed & 0xff);
    }
    if (gl == 0 && n != 0) scales[gb] = amax / kFp8Max;
  }
}

template <typename T>
__device__ __forceinline__ void dequant_unit(const QuantDesc& d,
                                             uint32_t local_unit) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const uint32_t group = threadIdx.x >> 3;
  const uint32_t gl = threadIdx.x & 7u;
  const uint32_t gb0 = local_unit * kQuantUnitBlocks + group;
  const float* scales = reinterpret_cast<const float*>(d.scales);
  if (d.fast) {
    v4u raw[kQuantPasses];
    float scale[kQuantPasses];
    uint64_t eoff[kQuantPasses];
    bool live[kQuantPasses];
#pragma unroll
    for (uint32_t p = 0; p < kQuantPasses; ++p) {
      const uint32_t gb = gb0 + p * 32u;
      uint32_t col0 = 0;
      eoff[p] = 0;
      live[p] = false;
      if (gb < d.nblocks) {
        quant_block_pos(d, gb, eoff[p], col0);
        live[p] = col0 + gl * 16u < d.cols;
        eoff[p] += gl * 16u;
      }
      raw[p] = v4u{0, 0, 0, 0};
      scale[p] = 0.0f;
      if (live[p]) {
        raw[p] = *reinterpret_cast<const gv4u*>(d.payload + eoff[p]);
        // the 8 lanes of a group read one address: a single broadcast fetch
        scale[p] = scales[gb];
      }
    }
#pragma unroll
    for (uint32_t p = 0; p < kQuantPasses; ++p) {
      if (!live[p]) continue;
      T e[16];
#pragma unroll
      for (uint32_t w = 0; w < 4; ++w) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[p][w], false);
        const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw[p][w], true);
        e[4 * w] = convert<float, T>(dequant_mul(lo[0], scale[p]));
        e[4 * w + 1] = convert<float, T>(dequant_mul(lo[1], scale[p]));
        e[4 * w + 2] = convert<float, T>(dequant_mul(hi[0], scale[p]));
        e[4 * w + 3] = convert<float, T>(dequant_mul(hi[1], scale[p]));
      }
      QuantRaw<T> out;
      __builtin_memcpy(&out, e, sizeof(e));
      gv4u* dst =
          reinterpret_cast<gv4u*>(d.wide + eoff[p] * sizeof(T));
#pragma unroll
      for (uint32_t k = 0; k < sizeof(T); ++k) dst[k] = out.q[k];
    }
    return;
  }
  T* dst = reinterpret_cast<T*>(d.wide);
  const uint8_t* payload = reinterpret_cast<const uint8_t*>(d.payload);
  for (uint32_t p = 0; p < kQuantPasses; ++p) {
    const uint32_t gb = gb0 + p * 32u;
    if (gb >= d.nblocks) continue;
    uint64_t eoff;
    uint32_t col0;
    quant_block_pos(d, gb, eoff, col0);
    const uint32_t n = min(kQuantBlock, d.cols - col0);
    const float scale = scales[gb];
    for (uint32_t c = gl; c < n; c += 8u) {
      const f32x2 v =
          __builtin_amdgcn_cvt_pk_f32_fp8((int)payload[eoff + c], false);
      dst[eoff + c] = convert<float, T>(dequant_mul(v[0], scale));
    }
  }
}

template <bool DEQUANT>
__global__ void __launch_bounds__(256)
quant_fp8_kernel(const QuantDesc* __restrict__ descs, uint32_t ndescs,
                 uint64_t total_units) {
  UnitWalk w;
  QuantDesc d = {};
  for (uint64_t unit = blockIdx.x; unit < total_units; unit += gridDim.x) {
    if (unit >= w.next_prefix) walk_seek(w, d, descs, ndescs, unit);
    const uint32_t local = (uint32_t)(unit - d.units_prefix);
    // d is uniform over the workgroup, so every wave takes one branch whole
    // and the 8-lane shuffles inside always see all 64 lanes active
    switch (static_cast<DType>(d.dtype)) {
      case DType::F32:
        if (DEQUANT) dequant_unit<float>(d, local);
        else quant_unit<float>(d, local);
        break;
      case DType::F16:
        if (DEQUANT) dequant_unit<__half>(d, local);
        else quant_unit<__half>(d, local);
        break;
      default:
        if (DEQUANT) dequant_unit<__hip_bfloat16>(d, local);
        else quant_unit<__hip_bfloat16>(d, local);
        break;
    }
  }
}

// launches of either kernel (tests check the batching through this)
static std::atomic<uint64_t> g_quant_launches{0};

// One launch of either kernel, async on `stream`.  Grid cap (workgroups):
// the sweep on 1 GiB of bf16 (profiles/quant_sync.log) kept gaining up to
// 65536, about one unit per workgroup, as the flat copy kernel did: 5.6 TB/s
// quant and 5.4 TB/s dequant against 4.9 / 4.8 at the cast kernel's 1024
template <bool DEQUANT>
static void launch_quant_fp8(const Plan<QuantDesc>& p, int device,
                             hipStream_t stream) {
  if (p.descs.empty()) return;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(
      p.units, env_u32("HIPSTORE_QUANT_GRID", 64, UINT32_MAX, 65536));
  stage_descs_and_launch(device, stream, p.descs, [&](const QuantDesc* d) {
    hipLaunchKernelGGL(quant_fp8_kernel<DEQUANT>, dim3(grid), dim3(256), 0,
                       stream, d, (uint32_t)p.descs.size(), p.units);
  });
  g_quant_launches.fetch_add(1, std::memory_order_relaxed);
}
