// Row-scaled FP8 (OCP e4m3, one f32 scale per row) quantise / dequantise
// kernels — K10/K11.
//
// Format (per tensor, rows = the last dimension, a 1-D tensor is one row):
//   amax  = max(max|x| over the row, 2^-96)
//   scale = amax / 448            (stored, f32, index = row)
//   q     = rne_e4m3(clamp(x * (448 / amax), -448, 448))
//   y     = rne_dst(float(q) * scale)
// This is the recipe of quant_fp8.h with the block being the whole row: every
// step is one correctly rounded IEEE fp32 operation (no fast-math here), the
// fences quant_mul / dequant_mul and the conversions are the ones of that
// file, and max is exact and associative on finite values, so whatever tree
// reduces the row, the bytes equal those of the torch implementation in
// ops/quant_row.py.  Non-finite input is outside the contract.
//
// Quantise.  The reduction runs over a whole row, so the work split follows
// the row length; plan_row fixes the regime per tensor (RowDesc::mode).  In
// each, a lane moves 16 consecutive elements per step on the fast path (bases
// 16B aligned, cols % 16 == 0): 2 (bf16/f16) or 4 (f32) 16B loads and one 16B
// payload store, the wide-side pattern of K4 to K9.
//   wave   (cols <= kRowWave = 4096): a unit is kRowWaveRows = 4 consecutive
//          rows, one per wave of the 256-thread workgroup.  The row stays in
//          registers, up to kRowSteps = 4 steps per lane at a stride of 1024
//          elements, all loads issued first.  The amax is reduced over the
//          wave by shuffles; no LDS, no barrier.  A wave whose row does not
//          exist skips as a whole.
//   held   (kRowWave < cols <= kRowWg = 16384): a unit is one row, held in the
//          workgroup's registers, up to 4 steps per lane at a stride of 4096.
//          Each wave reduces its lanes and lane 0 writes one float to LDS;
//          one barrier; every lane reads the four partials.
//   stream (cols > kRowWg): a unit is one row; the workgroup streams it once
//          for the amax (the same reduction) and a second time to convert.
//          There is no reduction across workgroups, so a giant 1-D tensor is
//          ONE workgroup's work: the slow case of a format meant for matrices.
// The LDS partials live in TWO slots of four floats taken alternately (a
// counter that every lane of the workgroup advances per reduction): a wave
// can only write slot s again after the barrier of the reduction in between,
// which no wave passes before all have read slot s.  One barrier per row.
// Everything else (an unaligned base, cols % 16 != 0) takes the generic path
// of the same regimes: the same row ownership and reductions, but the lanes
// stride over the row element by element, twice (amax, then convert), and
// store payload bytes singly, so nothing is written past a row.  All control
// flow around the shuffles is uniform over the wave, around the barrier over
// the workgroup (the descriptor and the unit are); dead lanes add 0.0f.
//
// Dequantise is element-wise: a unit is kRowDqPasses passes of the workgroup
// over consecutive 16-element chunks of the whole tensor (the flat pattern of
// K5).  With cols % 16 == 0 a chunk lies in one row, whose scale index is
// element_offset / cols in 64 bits; the lanes of one row read one address.
// The generic path takes the row per element.
//
// Measured on an MI355X, 1 GiB of bf16 per shape, the block-scaled kernels
// (K4/K5) on the same data in the same run as the yardstick
// (profiles/row_sync.log; read + write, medians of 3 x 300 calls, the four
// kernels taking their repeats in turn, scatter at most 1 %):
//   shape            regime   quant        vs K4    dequant      vs K5
//   131072 x 4096    wave     5.43 TB/s    0.96     5.37 TB/s    0.98
//   37449 x 14336    held     5.38 TB/s    0.95     5.37 TB/s    0.98
//   8192 x 65536     stream   4.01 TB/s    0.71     5.38 TB/s    0.99
// so the wave and held regimes are 4 to 5 % behind the block kernel, the
// dequantise 1 to 2 %.  W = 4096 and R = 16384 stand: with the limits lowered
// (HIPSTORE_ROW_WAVE / HIPSTORE_ROW_WG) the 4096-wide rows fell to 4.98 TB/s
// held by the workgroup and 4.79 streamed, the 14336-wide ones to 4.99
// streamed; both limits are also all the registers hold (f32 quantise, plain
// hipcc -O3 for gfx950: 115 VGPRs, occupancy 4, no scratch).  The streamed
// regime stays clearly below the yardstick:
// 0.402 ms against 0.289.  Re-reading 1 GiB from HBM at the yardstick's rate
// would make it 0.48 ms, a free second read 0.29, so the second pass is
// served from cache only in part (the 128 KiB row is re-read right after the
// first pass, but 65536 workgroups' rows together do not stay in L2); the
// barrier between the passes, which leaves a workgroup with nothing in
// flight, is supposed to cost the rest.  Not pursued: rows above 16384
// elements are rare in weight matrices.

#pragma once

#include "common.h"
#include "desc_ring.h"
#include "plan.h"
#include "quant_fp8.h"  // conversions, quant_scaled, dequant_mul, QuantRaw
#include "unit_walk.h"

#include <algorithm>
#include <atomic>

__device__ __forceinline__ float wave_max(float a) {
  a = fmaxf(a, __shfl_xor(a, 1));
  a = fmaxf(a, __shfl_xor(a, 2));
  a = fmaxf(a, __shfl_xor(a, 4));
  a = fmaxf(a, __shfl_xor(a, 8));
  a = fmaxf(a, __shfl_xor(a, 16));
  a = fmaxf(a, __shfl_xor(a, 32));
  return a;
}

// amax over the owners of a row: the wave, or (WG) the whole workgroup through
// the LDS slot of this reduction; `red` counts the workgroup's reductions
template <bool WG>
__device__ __forceinline__ float row_reduce(float a, float* lds,
                                            uint32_t& red) {
  a = wave_max(a);
  if (!WG) return a;
  float* slot = lds + (red & 1u) * 4u;
  ++red;
  if ((threadIdx.x & 63u) == 0) slot[threadIdx.x >> 6] = a;
  __syncthreads();
  return fmaxf(fmaxf(slot[0], slot[1]), fmaxf(slot[2], slot[3]));
}

template <typename T>
__device__ __forceinline__ float row_amax16(const QuantRaw<T>& raw) {
  T e[16];
  __builtin_memcpy(e, &raw, sizeof(e));
  float amax = 0.0f;
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k)
    amax = fmaxf(amax, fabsf(convert<T, float>(e[k])));
  return amax;
}

template <typename T>
__device__ __forceinline__ v4u row_cvt16(const QuantRaw<T>& raw, float inv) {
  T e[16];
  __builtin_memcpy(e, &raw, sizeof(e));
  v4u out;
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) {
    int packed = 0;
    packed = __builtin_amdgcn_cvt_pk_fp8_f32(
        quant_scaled(convert<T, float>(e[4 * w]), inv),
        quant_scaled(convert<T, float>(e[4 * w + 1]), inv), packed, false);
    packed = __builtin_amdgcn_cvt_pk_fp8_f32(
        quant_scaled(convert<T, float>(e[4 * w + 2]), inv),
        quant_scaled(convert<T, float>(e[4 * w + 3]), inv), packed, true);
    out[w] = (uint32_t)packed;
  }
  return out;
}

template <typename T>
__device__ __forceinline__ QuantRaw<T> row_load16(const RowDesc& d,
                                                  uint64_t eoff) {
  QuantRaw<T> raw;
  const gv4u* s = reinterpret_cast<const gv4u*>(d.wide + eoff * sizeof(T));
#pragma unroll
  for (uint32_t k = 0; k < sizeof(T); ++k) raw.q[k] = s[k];
  return raw;
}

// fast path of the wave and held regimes: the row in the registers of its
// owners (LANES = 64 or 256 of them), lane `lane` taking the 16 elements at
// column (s * LANES + lane) * 16 in step s
template <typename T, bool WG>
__device__ __forceinline__ void row_quant_held(const RowDesc& d, uint64_t row,
                                               float* lds, uint32_t& red) {
  constexpr uint32_t LANES = WG ? 256u : 64u;
  const uint32_t lane = threadIdx.x & (LANES - 1u);
  const uint64_t e0 = row * d.cols;
  QuantRaw<T> raw[kRowSteps];
  bool live[kRowSteps];
  // all loads of the row first: up to 128 B (bf16/f16) or 256 B (f32) in
  // flight per lane before the first dependent instruction
#pragma unroll
  for (uint32_t s = 0; s < kRowSteps; ++s) {
    const uint32_t c = (s * LANES + lane) * 16u;  // < 2^15: no overflow
    live[s] = c < d.cols;  // cols % 16 == 0: all 16 elements or none
#pragma unroll
    for (uint32_t k = 0; k < sizeof(T); ++k) raw[s].q[k] = v4u{0, 0, 0, 0};
    if (live[s]) raw[s] = row_load16<T>(d, e0 + c);
  }
  float amax = 0.0f;  // dead steps hold zeros and add nothing
#pragma unroll
  for (uint32_t s = 0; s < kRowSteps; ++s)
    amax = fmaxf(amax, row_amax16<T>(raw[s]));
  amax = fmaxf(row_reduce<WG>(amax, lds, red), kAmaxFloor);
  const float inv = kFp8Max / amax;
#pragma unroll
  for (uint32_t s = 0; s < kRowSteps; ++s) {
    const uint32_t c = (s * LANES + lane) * 16u;
    if (live[s])
      *reinterpret_cast<gv4u*>(d.payload + e0 + c) = row_cvt16<T>(raw[s], inv);
  }
  if (lane == 0) reinterpret_cast<float*>(d.scales)[row] = amax / kFp8Max;
}

// fast path of the stream regime: two passes of the workgroup over the row
template <typename T>
__device__ __forceinline__ void row_quant_stream(const RowDesc& d,
                                                 uint64_t row, float* lds,
                                                 uint32_t& red) {
  const uint64_t e0 = row * d.cols;
  const uint64_t cols = d.cols;  // 64-bit columns: cols may be close to 2^32
  float amax = 0.0f;
  for (uint64_t c = threadIdx.x * 16u; c < cols; c += 4096u)
    amax = fmaxf(amax, row_amax16<T>(row_load16<T>(d, e0 + c)));
  // lanes leave the loop at different trips and meet again before the barrier
  amax = fmaxf(row_reduce<true>(amax, lds, red), kAmaxFloor);
  const float inv = kFp8Max / amax;
  for (uint64_t c = threadIdx.x * 16u; c < cols; c += 4096u)
    *reinterpret_cast<gv4u*>(d.payload + e0 + c) =
        row_cvt16<T>(row_load16<T>(d, e0 + c), inv);
  if (threadIdx.x == 0) reinterpret_cast<float*>(d.scales)[row] = amax / kFp8Max;
}

// generic path of every regime: the owners stride over the row by elements
template <typename T, bool WG>
__device__ __forceinline__ void row_quant_generic(const RowDesc& d,
                                                  uint64_t row, float* lds,
                                                  uint32_t& red) {
  constexpr uint32_t LANES = WG ? 256u : 64u;
  const uint32_t lane = threadIdx.x & (LANES - 1u);
  const T* src = reinterpret_cast<const T*>(d.wide) + row * d.cols;
  uint8_t* payload = reinterpret_cast<uint8_t*>(d.payload) + row * d.cols;
  const uint64_t cols = d.cols;
  float amax = 0.0f;
  for (uint64_t c = lane; c < cols; c += LANES)
    amax = fmaxf(amax, fabsf(convert<T, float>(src[c])));
  amax = fmaxf(row_reduce<WG>(amax, lds, red), kAmaxFloor);
  const float inv = kFp8Max / amax;
  for (uint64_t c = lane; c < cols; c += LANES) {
    const float v = quant_scaled(convert<T, float>(src[c]), inv);
    const int packed = __builtin_amdgcn_cvt_pk_fp8_f32(v, v, 0, false);
    payload[c] = (uint8_t)(packed & 0xff);
  }
  if (lane == 0) reinterpret_cast<float*>(d.scales)[row] = amax / kFp8Max;
}

template <typename T>
__device__ __forceinline__ void row_quant_unit(const RowDesc& d,
                                               uint64_t local_unit, float* lds,
                                               uint32_t& red) {
  if (d.mode == kRowModeWave) {
    const uint64_t row = local_unit * kRowWaveRows + (threadIdx.x >> 6);
    if (row >= d.rows) return;  // the whole wave: its row does not exist
    if (d.fast) row_quant_held<T, false>(d, row, lds, red);
    else row_quant_generic<T, false>(d, row, lds, red);
    return;
  }
  // one row per unit and the workgroup whole: every lane reaches the barrier
  if (!d.fast) row_quant_generic<T, true>(d, local_unit, lds, red);
  else if (d.mode == kRowModeHeld) row_quant_held<T, true>(d, local_unit, lds, red);
  else row_quant_stream<T>(d, local_unit, lds, red);
}

template <typename T>
__device__ __forceinline__ void row_dequant_unit(const RowDesc& d,
                                                 uint64_t local_unit) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const float* scales = reinterpret_cast<const float*>(d.scales);
  const uint64_t base = local_unit * kRowDqUnitElems;
  if (d.fast) {
    v4u raw[kRowDqPasses];
    float scale[kRowDqPasses];
    uint64_t eoff[kRowDqPasses];
#pragma unroll
    for (uint32_t p = 0; p < kRowDqPasses; ++p) {
      eoff[p] = base + (p * 256u + threadIdx.x) * 16u;
      raw[p] = v4u{0, 0, 0, 0};
      scale[p] = 0.0f;
      if (eoff[p] < d.numel) {  // numel % 16 == 0: all 16 elements or none
        raw[p] = *reinterpret_cast<const gv4u*>(d.payload + eoff[p]);
        // cols % 16 == 0: the chunk lies in one row, and the lanes of a row
        // read one address
        scale[p] = scales[eoff[p] / d.cols];
      }
    }
#pragma unroll
    for (uint32_t p = 0; p < kRowDqPasses; ++p) {
      if (eoff[p] >= d.numel) continue;
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
      gv4u* dst = reinterpret_cast<gv4u*>(d.wide + eoff[p] * sizeof(T));
#pragma unroll
      for (uint32_t k = 0; k < sizeof(T); ++k) dst[k] = out.q[k];
    }
    return;
  }
  T* dst = reinterpret_cast<T*>(d.wide);
  const uint8_t* payload = reinterpret_cast<const uint8_t*>(d.payload);
  const uint64_t end =
      base + kRowDqUnitElems < d.numel ? base + kRowDqUnitElems : d.numel;
  for (uint64_t e = base + threadIdx.x; e < end; e += 256u) {
    const f32x2 v = __builtin_amdgcn_cvt_pk_f32_fp8((int)payload[e], false);
    dst[e] = convert<float, T>(dequant_mul(v[0], scales[e / d.cols]));
  }
}

template <bool DEQUANT>
__global__ void __launch_bounds__(256)
quant_row_kernel(const RowDesc* __restrict__ descs, uint32_t ndescs,
                 uint64_t total_units) {
  __shared__ float lds[8];  // two slots of one partial per wave
  uint32_t red = 0;
  UnitWalk w;
  RowDesc d = {};
  for (uint64_t unit = blockIdx.x; unit < total_units; unit += gridDim.x) {
    if (unit >= w.next_prefix) walk_seek(w, d, descs, ndescs, unit);
    const uint64_t local = unit - d.units_prefix;
    // d and the unit are uniform over the workgroup: its waves take the same
    // branch down to the row each of them owns
    switch (static_cast<DType>(d.dtype)) {
      case DType::F32:
        if (DEQUANT) row_dequant_unit<float>(d, local);
        else row_quant_unit<float>(d, local, lds, red);
        break;
      case DType::F16:
        if (DEQUANT) row_dequant_unit<__half>(d, local);
        else row_quant_unit<__half>(d, local, lds, red);
        break;
      default:
        if (DEQUANT) row_dequant_unit<__hip_bfloat16>(d, local);
        else row_quant_unit<__hip_bfloat16>(d, local, lds, red);
        break;
    }
  }
}

// launches of either kernel, counted apart from the other formats'
static std::atomic<uint64_t> g_row_launches{0};

// One launch of either kernel, async on `stream`.  Grid cap (workgroups),
// from profiles/row_sync.log.  The three 1 GiB shapes have at most 65536
// units, so on them the sweep only shows that a cap below the unit count
// costs: quant 5.20 / 5.03 TB/s at 1024 against 5.43 / 5.39 at one workgroup
// per unit (wave / held), dequant 4.88 at 1024 and 4.90 at 16384 against
// 5.37; the streamed quantise does not care (4.01 to 4.02 TB/s).  A cap
// ABOVE 65536 was measured on 2 GiB of 1024-wide rows (262144 quantise,
// 131072 dequantise units): the quantise is best capped (5.33 TB/s at 65536
// and 16384, 5.18 at 131072, 4.77 at 262144), the dequantise best with one
// workgroup per unit (5.06 at 65536, 5.39 at 131072 and above).  65536, the
// other kernels' cap, is kept for both: a larger one for the dequantise
// alone would gain it about 6 % on tensors above 512 Mi elements and on
// batches of that size; not settled here, HIPSTORE_ROW_GRID serves meanwhile
template <bool DEQUANT>
static void launch_quant_row(const Plan<RowDesc>& p, int device,
                             hipStream_t stream) {
  if (p.descs.empty()) return;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(
      p.units, env_u32("HIPSTORE_ROW_GRID", 64, UINT32_MAX, 65536));
  stage_descs_and_launch(device, stream, p.descs, [&](const RowDesc* d) {
    hipLaunchKernelGGL(quant_row_kernel<DEQUANT>, dim3(grid), dim3(256), 0,
                       stream, d, (uint32_t)p.descs.size(), p.units);
  });
  g_row_launches.fetch_add(1, std::memory_order_relaxed);
}
