// MXFP8 (OCP Microscaling v1.0: e4m3 values, one e8m0 scale byte per
// 32-element block, "floor" scale rule) quantise / dequantise kernels, K16/K17.
//
// Format (per tensor, rows = the last dimension, blocks of 32 elements, the
// last block of a row may be short and its missing elements count as +0):
//   amax  = max |x| over the block
//   code  = max(expfield(amax) - 8, 0)      (stored, one byte per block)
//   X     = 2^(code - 127)                  (code 0: the f32 subnormal 2^-127,
//                                            code 255: NaN)
//   v     = x * 2^(127 - code)              (exact, or both sides zero)
//   q     = rne_e4m3fn(clamp(v, -448, 448)), sign of v kept (also on zero)
//   y     = rne_dst(float(q) * X)           (one fp32 multiply)
// 8 is emax of e4m3: the rule of quant_mx.h with its 2 replaced.  |v| < 512,
// and a block whose amax lies in (448 X, 512 X) saturates its top values to
// 448 X.  The payload is one byte per element in the element order of the
// source, so rows and blocks never share a byte.  Every step is integer work
// on the bits or one correctly rounded IEEE fp32 operation, so the bytes equal
// those of the torch implementation in ops/mx8.py; this file must stay free
// of fast-math and of denormal flushing, like quant_mx.h.  Finite input never
// produces scale code 255 nor the e4m3 NaN codes; non-finite input is outside
// the contract (it poisons its own block only).
//
// Work layout: units of kMxUnitBlocks blocks of one tensor, the unit walk, the
// descriptors (MxDesc) and the planner (plan_mx) are those of the MXFP4
// kernels; all loads of a unit are issued before the first dependent
// instruction, as there.
//
// Fast path (wide and payload bases 16B aligned, cols % 32 == 0): block b of
// the tensor is elements [32 b, 32 b + 32), its payload the 32 bytes at 32 b
// and its scale byte b.  Two lanes own a block, 16 consecutive elements each:
// 2 (bf16/f16) or 4 (f32) 16B accesses on the wide side, one __shfl_xor joins
// the two amax halves, and the lane's 16 payload bytes move as ONE 16B access,
// so adjacent lanes lie 16 B apart and a wave covers 1 KiB without a gap (the
// layout MXFP4 could not have: its lanes end in 8B stores).  Scale bytes:
// HIPSTORE_MX8_SCALE_DWORD below.  Everything else takes the generic path of
// the same kernel: one lane per block, element by element, byte accesses; a
// payload byte is one element, so no byte is shared between lanes.
//
// Conversion: HIPSTORE_MX8_SCALED_QUANT / HIPSTORE_MX8_SCALED_DEQUANT below.
//
// Resources on gfx950 (hipcc -O3, -Rpass-analysis=kernel-resource-usage), as
// built by default: K16 60 VGPRs, K17 38 VGPRs, occupancy 8 waves per SIMD
// both, no scratch, no SGPR or VGPR spills, no LDS.

#pragma once

#include "common.h"
#include "desc_ring.h"
#include "plan.h"
#include "quant_fp8.h"  // quant_mul / dequant_mul / quant_scaled
#include "quant_mx.h"   // mx_abs_bits, mx_inv_scale, mx_scale, gu8
#include "unit_walk.h"

#include <algorithm>
#include <atomic>

// Conversion form.  1: gfx950's scaled conversions, v_cvt_scalef32_pk_fp8_f32
// to quantise and v_cvt_scalef32_pk_f32_fp8 to dequantise, with the scale
// operand __uint_as_float(code << 23): its exponent field IS the e8m0 byte, so
// scaling and rounding are one instruction per two elements, with no fp32
// multiply.  0: the path of K4/K5, quant_mul by 2^(127 - code), a clamp to
// +-448 and v_cvt_pk_fp8_f32; on the way back v_cvt_pk_f32_fp8 and
// dequant_mul by X.  A side may use form 1 only while it is byte-identical to
// the recipe above on every test of tests/test_gpu_mx8.py.  As found on an
// MI355X:
//   quantise: form 1 does NOT saturate.  A block's top value in the band
//     (448 X, 512 X) came out as the NaN code 0x7F where the recipe wants 448
//     (the first thing the tests hit, for all three source dtypes), so K16
//     takes form 0, the K4 path.  Nothing else was judged for form 1 on this
//     side.
//   dequantise: form 1 passed every test: all 256 codes under the scale
//     codes 0 (2^-127, subnormal products), 1, 107, 127, 143, 254 (448 X
//     overflows to inf) and 255 (NaN), into f32, bf16 and f16, fast and
//     generic path; -0 stays -0.  K17 takes form 1.
// Neither choice shows in the rates: on 1 GiB of bf16 the builds differ by no
// more than two runs of one build do (docs/PERFORMANCE.md, "MXFP8 sync").
#ifndef HIPSTORE_MX8_SCALED_QUANT
#define HIPSTORE_MX8_SCALED_QUANT 0
#endif
#ifndef HIPSTORE_MX8_SCALED_DEQUANT
#define HIPSTORE_MX8_SCALED_DEQUANT 1
#endif
static constexpr bool kMx8ScaledQuant = HIPSTORE_MX8_SCALED_QUANT;
static constexpr bool kMx8ScaledDequant = HIPSTORE_MX8_SCALED_DEQUANT;

// Scale bytes of the quantise fast path.  1: the codes of four consecutive
// blocks are gathered across their eight lanes (two __shfl_xor) and leave as
// one dword from one lane in eight, where the scales base is 4B aligned and
// all four blocks exist; the tensor's last, partial group and tensors with an
// odd scales base write bytes.  0: one byte from every second lane, as MXFP4
// does.  Measured on 1 GiB of bf16, one build each in one session: quantise
// 5.59 TB/s with dwords against 5.54 with bytes, 0.8 % apart with a scatter
// of 0.7 to 1.4 % between repeats: no difference that the measurement can
// show.  1 stays, for a quarter of the store instructions.  Dequantise reads
// the byte per lane pair either way.
#ifndef HIPSTORE_MX8_SCALE_DWORD
#define HIPSTORE_MX8_SCALE_DWORD 1
#endif
static constexpr bool kMx8ScaleDword = HIPSTORE_MX8_SCALE_DWORD;

static constexpr uint32_t kMx8LaneElems = kMxBlock / 2u;   // 16
static constexpr uint32_t kMx8PassBlocks = 256u / 2u;      // 128 per pass
static constexpr uint32_t kMx8Passes = kMxUnitBlocks / kMx8PassBlocks;
static_assert(kMx8PassBlocks % 4u == 0 && kMxUnitBlocks % 4u == 0,
              "a group of four scale bytes never straddles a pass or a unit");

typedef short v2s __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) uint32_t gu32_mx8;

// e8m0 code of a block from the bits of its amax (finite: at most 246)
__device__ __forceinline__ uint32_t mx8_scale_code(uint32_t amax_bits) {
  const uint32_t e = amax_bits >> 23;
  return e > 8u ? e - 8u : 0u;
}

// the scale operand of the scaled conversions: only the exponent field is
// read, and it is the e8m0 byte itself (0 means 2^-127, 255 NaN)
__device__ __forceinline__ float mx8_scale_operand(uint32_t code) {
  return __uint_as_float(code << 23);
}

// four values of a block -> four e4m3 codes, element k in bits 8k..8k+7
__device__ __forceinline__ uint32_t mx8_pack4(const float* x, uint32_t code) {
  if (kMx8ScaledQuant) {
    const float s = mx8_scale_operand(code);
    v2s r = {0, 0};
    r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, x[0], x[1], s, false);
    r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(r, x[2], x[3], s, true);
    uint32_t w;
    __builtin_memcpy(&w, &r, sizeof(w));
    return w;
  }
  const float inv = mx_inv_scale(code);
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(quant_scaled(x[0], inv),
                                      quant_scaled(x[1], inv), w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(quant_scaled(x[2], inv),
                                      quant_scaled(x[3], inv), w, true);
  return (uint32_t)w;
}

// the reverse: four e4m3 codes -> float(q) * X, each as one fp32 product
__device__ __forceinline__ void mx8_unpack4(uint32_t w, uint32_t code,
                                            float* y) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  if (kMx8ScaledDequant) {
    const float s = mx8_scale_operand(code);
    const f32x2 lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, s, false);
    const f32x2 hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, s, true);
    y[0] = lo[0]; y[1] = lo[1]; y[2] = hi[0]; y[3] = hi[1];
    return;
  }
  const float scale = mx_scale(code);
  const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
  const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  y[0] = dequant_mul(lo[0], scale); y[1] = dequant_mul(lo[1], scale);
  y[2] = dequant_mul(hi[0], scale); y[3] = dequant_mul(hi[1], scale);
}

// generic path: where block gb of the tensor sits; an element is a payload
// byte, so one offset serves both sides
struct Mx8BlockPos {
  uint64_t eoff;  // element offset of its first column
  uint32_t n;     // its elements, 1..32
};

__device__ __forceinline__ Mx8BlockPos mx8_block_pos(const MxDesc& d,
                                                     uint32_t gb) {
  const uint32_t row = gb / d.nblk;
  const uint32_t col0 = (gb - row * d.nblk) * kMxBlock;
  return Mx8BlockPos{(uint64_t)row * d.cols + col0,
                     min(kMxBlock, d.cols - col0)};
}

template <typename T>
__device__ __forceinline__ void mx8_quant_unit(const MxDesc& d,
                                               uint32_t local_unit) {
  gu8* scales = reinterpret_cast<gu8*>(d.scales);
  if (d.fast) {
    constexpr uint32_t NV = kMx8LaneElems * sizeof(T) / 16u;  // loads per pass
    const uint32_t sub = threadIdx.x & 1u;
    const uint32_t gb0 = local_unit * kMxUnitBlocks + threadIdx.x / 2u;
    // uniform over the workgroup: the descriptor's scales base
    const bool dword_ok = kMx8ScaleDword && (d.scales & 3u) == 0;
    v4u raw[kMx8Passes][NV];
#pragma unroll
    for (uint32_t p = 0; p < kMx8Passes; ++p) {
      const uint32_t gb = gb0 + p * kMx8PassBlocks;
#pragma unroll
      for (uint32_t k = 0; k < NV; ++k) raw[p][k] = v4u{0, 0, 0, 0};
      if (gb < d.nblocks) {
        const gv4u* s = reinterpret_cast<const gv4u*>(
            d.wide +
            ((uint64_t)gb * kMxBlock + sub * kMx8LaneElems) * sizeof(T));
#pragma unroll
        for (uint32_t k = 0; k < NV; ++k) raw[p][k] = s[k];
      }
    }
#pragma unroll
    for (uint32_t p = 0; p < kMx8Passes; ++p) {
      const uint32_t gb = gb0 + p * kMx8PassBlocks;
      T e[kMx8LaneElems];
      __builtin_memcpy(e, raw[p], sizeof(e));
      float x[kMx8LaneElems];
      uint32_t amax = 0;
#pragma unroll
      for (uint32_t k = 0; k < kMx8LaneElems; ++k) {
        x[k] = convert<T, float>(e[k]);
        amax = max(amax, mx_abs_bits(x[k]));
      }
      // the pair is live or dead as a whole, and the unit's descriptor is
      // uniform over the workgroup: all 64 lanes reach every shuffle here
      amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1));
      const uint32_t code = mx8_scale_code(amax);
      v4u out;
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) out[k] = mx8_pack4(x + 4 * k, code);
      // the codes of blocks gb & ~3 .. gb | 3, block j in bits 8j..8j+7; a
      // dead pair holds zeros (code 0) and only registers are exchanged
      uint32_t four = code << (8u * ((threadIdx.x >> 1) & 3u));
      if (kMx8ScaleDword) {
        four |= (uint32_t)__shfl_xor((int)four, 2);
        four |= (uint32_t)__shfl_xor((int)four, 4);
      }
      if (gb < d.nblocks) {
        *reinterpret_cast<gv4u*>(d.payload + (uint64_t)gb * kMxBlock +
                                 sub * kMx8LaneElems) = out;
        // (gb | 3) < nblocks: all four blocks of the group exist, so the
        // dword lies inside the scales; gb & ~3 is a multiple of 4 from a 4B
        // aligned base
        if (dword_ok && (gb | 3u) < d.nblocks) {
          if ((threadIdx.x & 7u) == 0)
            *reinterpret_cast<gu32_mx8*>(d.scales + gb) = four;
        } else if (sub == 0) {
          scales[gb] = (uint8_t)code;
        }
      }
    }
    return;
  }
  // generic: lane t of the workgroup takes block t of the unit
  const uint32_t gb = local_unit * kMxUnitBlocks + threadIdx.x;
  if (gb >= d.nblocks) return;
  const Mx8BlockPos pos = mx8_block_pos(d, gb);
  const T* src = reinterpret_cast<const T*>(d.wide) + pos.eoff;
  gu8* payload = reinterpret_cast<gu8*>(d.payload) + pos.eoff;
  float x[kMxBlock];
  uint32_t amax = 0;
#pragma unroll
  for (uint32_t c = 0; c < kMxBlock; ++c) {
    x[c] = c < pos.n ? convert<T, float>(src[c]) : 0.0f;
    amax = max(amax, mx_abs_bits(x[c]));
  }
  const uint32_t code = mx8_scale_code(amax);
#pragma unroll
  for (uint32_t k = 0; k < kMxBlock / 4u; ++k) {
    const uint32_t w = mx8_pack4(x + 4 * k, code);
    if (4u * k >= pos.n) continue;
    // the word's live bytes, counted from the word: comparing every column
    // with n again would keep the 32 lane masks of the loads alive until
    // here, more than the scalar registers hold
    const uint32_t left = pos.n - 4u * k;
    payload[4u * k] = (uint8_t)w;
#pragma unroll
    for (uint32_t j = 1; j < 4; ++j) {
      if (j < left) payload[4u * k + j] = (uint8_t)(w >> (8u * j));
    }
  }
  scales[gb] = (uint8_t)code;
}

template <typename T>
__device__ __forceinline__ void mx8_dequant_unit(const MxDesc& d,
                                                 uint32_t local_unit) {
  const gu8* scales = reinterpret_cast<const gu8*>(d.scales);
  if (d.fast) {
    constexpr uint32_t NV = kMx8LaneElems * sizeof(T) / 16u;  // stores per pass
    const uint32_t sub = threadIdx.x & 1u;
    const uint32_t gb0 = local_unit * kMxUnitBlocks + threadIdx.x / 2u;
    v4u w[kMx8Passes];
    uint32_t code[kMx8Passes];
#pragma unroll
    for (uint32_t p = 0; p < kMx8Passes; ++p) {
      const uint32_t gb = gb0 + p * kMx8PassBlocks;
      w[p] = v4u{0, 0, 0, 0};
      code[p] = 0;
      if (gb < d.nblocks) {
        w[p] = *reinterpret_cast<const gv4u*>(
            d.payload + (uint64_t)gb * kMxBlock + sub * kMx8LaneElems);
        // the lanes of a pair read one address: a single broadcast fetch
        code[p] = scales[gb];
      }
    }
#pragma unroll
    for (uint32_t p = 0; p < kMx8Passes; ++p) {
      const uint32_t gb = gb0 + p * kMx8PassBlocks;
      if (gb >= d.nblocks) continue;
      T e[kMx8LaneElems];
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        float y[4];
        mx8_unpack4(w[p][k], code[p], y);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) e[4 * k + j] = convert<float, T>(y[j]);
      }
      v4u out[NV];
      __builtin_memcpy(out, e, sizeof(e));
      gv4u* dst = reinterpret_cast<gv4u*>(
          d.wide + ((uint64_t)gb * kMxBlock + sub * kMx8LaneElems) * sizeof(T));
#pragma unroll
      for (uint32_t k = 0; k < NV; ++k) dst[k] = out[k];
    }
    return;
  }
  const uint32_t gb = local_unit * kMxUnitBlocks + threadIdx.x;
  if (gb >= d.nblocks) return;
  const Mx8BlockPos pos = mx8_block_pos(d, gb);
  T* dst = reinterpret_cast<T*>(d.wide) + pos.eoff;
  const gu8* payload = reinterpret_cast<const gu8*>(d.payload) + pos.eoff;
  const uint32_t code = scales[gb];
  for (uint32_t c = 0; c < pos.n; ++c) {
    float y[4];
    mx8_unpack4(payload[c], code, y);
    dst[c] = convert<float, T>(y[0]);
  }
}

template <bool DEQUANT>
__global__ void __launch_bounds__(256)
quant_mx8_kernel(const MxDesc* __restrict__ descs, uint32_t ndescs,
                 uint64_t total_units) {
  UnitWalk w;
  MxDesc d = {};
  for (uint64_t unit = blockIdx.x; unit < total_units; unit += gridDim.x) {
    if (unit >= w.next_prefix) walk_seek(w, d, descs, ndescs, unit);
    const uint32_t local = (uint32_t)(unit - d.units_prefix);
    // d is uniform over the workgroup: every wave takes one branch whole
    switch (static_cast<DType>(d.dtype)) {
      case DType::F32:
        if (DEQUANT) mx8_dequant_unit<float>(d, local);
        else mx8_quant_unit<float>(d, local);
        break;
      case DType::F16:
        if (DEQUANT) mx8_dequant_unit<__half>(d, local);
        else mx8_quant_unit<__half>(d, local);
        break;
      default:
        if (DEQUANT) mx8_dequant_unit<__hip_bfloat16>(d, local);
        else mx8_quant_unit<__hip_bfloat16>(d, local);
        break;
    }
  }
}

// launches of either kernel, counted apart from every other format's
static std::atomic<uint64_t> g_mx8_launches{0};

// One launch of either kernel, async on `stream`.  Grid cap (workgroups):
// the sweep on 1 GiB of bf16 (profiles/mx8_sync.log) gained up to 65536,
// about one unit per workgroup, and nothing beyond (262144): 5.63 TB/s quant
// and 5.34 dequant against 4.97 / 4.85 at 1024
template <bool DEQUANT>
static void launch_quant_mx8(const Plan<MxDesc>& p, int device,
                             hipStream_t stream) {
  if (p.descs.empty()) return;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(
      p.units, env_u32("HIPSTORE_MX8_GRID", 64, UINT32_MAX, 65536));
  stage_descs_and_launch(device, stream, p.descs, [&](const MxDesc* d) {
    hipLaunchKernelGGL(quant_mx8_kernel<DEQUANT>, dim3(grid), dim3(256), 0,
                       stream, d, (uint32_t)p.descs.size(), p.units);
  });
  g_mx8_launches.fetch_add(1, std::memory_order_relaxed);
}
