// Per-tensor FP8 (OCP e4m3, one f32 scale per matrix) quantise / dequantise
// kernels — K14/K15.
//
// Format.  A tensor is a stack of matrices [*lead, R, C] (a 1-D tensor of n
// elements is the matrix [1, n]) and every matrix has ONE scale: the payload
// is e4m3 in the source's shape, the scales are f32 [*lead, 1, 1], the stored
// scale being the dequantisation multiplier.  This is the FP8 checkpoint
// format with one weight_scale per weight (strategy "tensor", the tensor-wise
// operand of scaled GEMMs), and of fused MoE stacks [E, R, C] with one scale
// per expert.  Per matrix:
//   amax  = max(max|x| over the matrix, 2^-96)
//   scale = amax / 448            (stored, f32)
//   q     = rne_e4m3(clamp(x * (448 / amax), -448, 448))
//   y     = rne_dst(float(q) * scale)
// This is the recipe of quant_fp8.h with the matrix as the block: every step
// is one correctly rounded IEEE fp32 operation (no fast-math here), the fences
// quant_mul / dequant_mul and the conversions are the ones of that file, and
// max is exact and associative on finite values, so whatever tree and
// whatever order of atomics reduces the matrix, the bytes equal those of the
// torch implementation in ops/quant_tensor.py.  Non-finite input is outside
// the contract.
//
// Quantise (K14).  A matrix is spread over thousands of workgroups, so its
// amax cannot be reduced inside one: it travels through memory between TWO
// launches on the caller's stream, and the stream order is the only
// synchronisation.  No workgroup waits for another, there is no flag, ticket
// or last-block pattern and no cooperative launch.  Both launches walk the
// same plan: a unit is a run of up to kTensorUnitElems = 16384 elements
// inside one matrix (kTensorPasses = 4 passes of 256 lanes x 16 elements),
// units are counted per matrix, so none straddles two scales.
//   pass A (quant_tensor_amax_kernel): a lane loads its 4 chunks as 16 B
//     vectors, all loads before the first dependent instruction (the pattern
//     of K4 and K12), and folds |x| into a running maximum that it keeps in a
//     register over the units of one matrix in the workgroup's walk, which
//     is a run of consecutive units (ceil(units / grid) of them).  When the walk reaches another matrix, and at its
//     end, the workgroup reduces the running maxima (shuffles, then the four
//     wave partials through the two alternating LDS slots of row_reduce: one
//     barrier per publication, not per unit) and ONE lane publishes the
//     result with one vector atomic max on its u32 bit pattern into the
//     matrix's amax slot; non-negative finite floats order like their bits.
//     A maximum of 0 is not published: the slot is zeroed before the launch.
//     The slots are one u32 per matrix, apart from the scales (pass B reads a
//     slot while another workgroup writes the scale), carved and zeroed by
//     the caller on the same stream.
//   pass B (quant_tensor_convert_kernel): a lane loads the same chunks and
//     the matrix's slot, applies the floor, and converts with inv = 448 /
//     amax, one 16 B payload store per chunk.  One lane of the workgroup that
//     takes a matrix's first unit stores amax / 448 into the scales.  No LDS,
//     no barrier.  Pass B takes the units in REVERSE order (workgroup 0 starts
//     at the last unit), so it begins on what pass A read last and the
//     256 MB last-level cache may still hold.
// An unaligned base or R * C % 16 != 0 (for a single matrix: numel % 16 != 0)
// takes the generic path of both passes: the same units, the lanes striding
// over the run element by element and storing payload bytes singly, so
// nothing is written past a matrix.  Every lane of the workgroup reaches the
// shuffles and the barrier of every publication: the descriptor, the unit and
// the slot are uniform over the workgroup, and edges are predicated.
//
// Dequantise (K15) is one launch, element-wise: a unit is kTensorDqPasses
// passes of the workgroup over consecutive 16-element chunks of the whole
// tensor (the flat pattern of K13).  With R * C % 16 == 0 a chunk lies in one
// matrix, whose scale index is element_offset / (R * C) in 64 bits; the
// generic path takes the index per element.
//
// Resources (plain hipcc -O3 for gfx950, resource-usage remarks): pass A 89
// VGPRs, occupancy 5, 32 B of LDS; pass B 80 VGPRs, occupancy 6; dequantise
// 36 VGPRs, occupancy 8; none uses scratch or spills a register.
//
// Measured on an MI355X, 1 GiB of bf16 per shape, the block-scaled kernels
// (K4/K5) on the same data in the same run as the yardstick
// (profiles/tensor_sync.log; one read + one write per element, medians of 3 x
// 300 calls, the four kernels taking their repeats in turn, scatter at most
// 0.5 %, of these kernels at most 0.2 %):
//   shape                      matrices  quant        vs K4   dequant     vs K5
//   131072 x 4096              1         3.33 TB/s    0.59    5.40 TB/s   0.99
//   256 x 1024 x 2048          256       3.21 TB/s    0.57    5.40 TB/s   0.99
//   Llama-like mix, 19 tensors 19        3.27 TB/s    0.58    5.39 TB/s   0.99
// The quantise reads the source twice, 5 bytes per bf16 element against K4's
// 3, so 0.60 is what the bytes allow.  The variants, same log: (a) with one
// workgroup and one atomic per unit (cap 65536) the 32768 atomics on the ONE
// slot of the large matrix cost 0.2 ms (0.686 ms against 0.484), the mix
// loses as much (0.648 against 0.492) and the stack 1 %; at 2048 the stack
// gains 1 % and the others lose 4 and 5 %.  8192 stands for the quantise,
// 65536 for the dequantise, which loses 13 % at 8192.  (b) pass B in reverse
// order gained 0.3 to 0.6 % at cap 65536 and 0.5 to 2.0 % at 8192 on every
// shape, and is kept.  (c) grid-strided units against consecutive ones, at
// cap 8192: strided is 2 and 1 % faster on the large matrix and the stack
// (0.475 / 0.488 ms against 0.484 / 0.494) and 27 % slower on the mix (0.635
// against 0.501), where a stride of 8192 units is longer than any matrix (at
// most 3584 units) and every unit was published on its own; consecutive units
// are kept, for batches are what a state_dict push quantises.  Also tried and
// dropped: reading the slot before the atomic and skipping it when the slot
// is already as large; at cap 65536 it brought the large matrix to 0.492 ms
// and took the stack from 0.509 to 1.49 ms; the cause was not traced.
// Not measured: caps between 2048 and 8192 or 8192 and 65536, and f32 or f16
// sources.

#pragma once

#include "common.h"
#include "desc_ring.h"
#include "plan.h"
#include "quant_row.h"  // wave_max, row_reduce, row_amax16, row_cvt16
#include "unit_walk.h"

#include <algorithm>
#include <atomic>

// where a quantise unit lies: unit = mat * units_per_mat + u
struct TensorPos {
  uint64_t mat;
  uint64_t e0;   // first element of the run, counted inside the matrix
  uint64_t end;  // one past its last element, at most mat_elems
};

__device__ __forceinline__ TensorPos tensor_pos(const TensorDesc& d,
                                                uint64_t unit) {
  TensorPos t;
  t.mat = unit / d.units_per_mat;
  t.e0 = (unit - t.mat * d.units_per_mat) * kTensorUnitElems;
  t.end = t.e0 + kTensorUnitElems < d.mat_elems ? t.e0 + kTensorUnitElems
                                                : d.mat_elems;
  return t;
}

// the lane's chunks of a unit on the fast path: chunk (p * 256 + lane) of the
// run in pass p; mat_elems % 16 == 0, so a chunk is all there or not at all
template <typename T>
__device__ __forceinline__ void tensor_load_unit(const TensorDesc& d,
                                                 const TensorPos& t,
                                                 QuantRaw<T> (&raw)[kTensorPasses],
                                                 bool (&live)[kTensorPasses]) {
  const uint64_t m0 = t.mat * d.mat_elems;
#pragma unroll
  for (uint32_t p = 0; p < kTensorPasses; ++p) {
    const uint64_t e = t.e0 + (p * 256u + threadIdx.x) * 16u;
    live[p] = e < t.end;
#pragma unroll
    for (uint32_t k = 0; k < sizeof(T); ++k) raw[p].q[k] = v4u{0, 0, 0, 0};
    if (live[p]) {
      const gv4u* s =
          reinterpret_cast<const gv4u*>(d.wide + (m0 + e) * sizeof(T));
#pragma unroll
      for (uint32_t k = 0; k < sizeof(T); ++k) raw[p].q[k] = s[k];
    }
  }
}

// pass A: the lane's share of max|x| over the unit (dead chunks add 0.0f)
template <typename T>
__device__ __forceinline__ float tensor_unit_amax(const TensorDesc& d,
                                                  uint64_t local_unit) {
  const TensorPos t = tensor_pos(d, local_unit);
  float amax = 0.0f;
  if (d.fast) {
    QuantRaw<T> raw[kTensorPasses];
    bool live[kTensorPasses];
    tensor_load_unit<T>(d, t, raw, live);
#pragma unroll
    for (uint32_t p = 0; p < kTensorPasses; ++p)
      amax = fmaxf(amax, row_amax16<T>(raw[p]));
    return amax;
  }
  const T* src = reinterpret_cast<const T*>(d.wide) + t.mat * d.mat_elems;
  for (uint64_t e = t.e0 + threadIdx.x; e < t.end; e += 256u)
    amax = fmaxf(amax, fabsf(convert<T, float>(src[e])));
  return amax;
}

// pass A: the workgroup's maximum of one matrix into that matrix's slot.  All
// lanes come here together (the slot is uniform) and meet at the barrier.
__device__ __forceinline__ void tensor_publish(float run, uint32_t* slot,
                                               float* lds, uint32_t& red) {
  const float a = row_reduce<true>(run, lds, red);
  // a >= +0 and finite: its bits order like its value; 0 is what the slot
  // holds.  The result is not used, so the atomic returns nothing and the
  // workgroup does not wait for it.
  if (threadIdx.x == 0 && a != 0.0f) atomicMax(slot, __float_as_uint(a));
}

// pass B: convert the unit with the amax that pass A left in the slot
template <typename T>
__device__ __forceinline__ void tensor_unit_convert(const TensorDesc& d,
                                                    uint64_t local_unit) {
  const TensorPos t = tensor_pos(d, local_unit);
  const uint32_t* slot = reinterpret_cast<const uint32_t*>(d.amax) + t.mat;
  float* scales = reinterpret_cast<float*>(d.scales);
  const uint64_t m0 = t.mat * d.mat_elems;
  if (d.fast) {
    QuantRaw<T> raw[kTensorPasses];
    bool live[kTensorPasses];
    tensor_load_unit<T>(d, t, raw, live);
    const float amax = fmaxf(__uint_as_float(*slot), kAmaxFloor);
    const float inv = kFp8Max / amax;
#pragma unroll
    for (uint32_t p = 0; p < kTensorPasses; ++p) {
      const uint64_t e = t.e0 + (p * 256u + threadIdx.x) * 16u;
      if (live[p])
        *reinterpret_cast<gv4u*>(d.payload + m0 + e) = row_cvt16<T>(raw[p], inv);
    }
    if (t.e0 == 0 && threadIdx.x == 0) scales[t.mat] = amax / kFp8Max;
    return;
  }
  const float amax = fmaxf(__uint_as_float(*slot), kAmaxFloor);
  const float inv = kFp8Max / amax;
  const T* src = reinterpret_cast<const T*>(d.wide) + m0;
  uint8_t* payload = reinterpret_cast<uint8_t*>(d.payload) + m0;
  for (uint64_t e = t.e0 + threadIdx.x; e < t.end; e += 256u) {
    const float v = quant_scaled(convert<T, float>(src[e]), inv);
    const int packed = __builtin_amdgcn_cvt_pk_fp8_f32(v, v, 0, false);
    payload[e] = (uint8_t)(packed & 0xff);
  }
  if (t.e0 == 0 && threadIdx.x == 0) scales[t.mat] = amax / kFp8Max;
}

template <typename T>
__device__ __forceinline__ void tensor_dequant_unit(const TensorDesc& d,
                                                    uint64_t local_unit) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const float* scales = reinterpret_cast<const float*>(d.scales);
  const uint64_t base = local_unit * kTensorDqUnitElems;
  if (d.fast) {
    v4u raw[kTensorDqPasses];
    float scale[kTensorDqPasses];
    uint64_t eoff[kTensorDqPasses];
#pragma unroll
    for (uint32_t p = 0; p < kTensorDqPasses; ++p) {
      eoff[p] = base + (p * 256u + threadIdx.x) * 16u;
      raw[p] = v4u{0, 0, 0, 0};
      scale[p] = 0.0f;
      if (eoff[p] < d.numel) {  // numel % 16 == 0: all 16 elements or none
        raw[p] = *reinterpret_cast<const gv4u*>(d.payload + eoff[p]);
        // mat_elems % 16 == 0: the chunk lies in one matrix, and the lanes of
        // a matrix read one address
        scale[p] = scales[eoff[p] / d.mat_elems];
      }
    }
#pragma unroll
    for (uint32_t p = 0; p < kTensorDqPasses; ++p) {
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
      base + kTensorDqUnitElems < d.numel ? base + kTensorDqUnitElems : d.numel;
  for (uint64_t e = base + threadIdx.x; e < end; e += 256u) {
    const f32x2 v = __builtin_amdgcn_cvt_pk_f32_fp8((int)payload[e], false);
    dst[e] = convert<float, T>(dequant_mul(v[0], scales[e / d.mat_elems]));
  }
}

// pass A and pass B give a workgroup `per` CONSECUTIVE units, not grid-strided
// ones: in a batch of many tensors a stride of one grid is longer than most
// matrices, and a running maximum that never spans two units publishes after
// every one of them
__global__ void __launch_bounds__(256)
quant_tensor_amax_kernel(const TensorDesc* __restrict__ descs, uint32_t ndescs,
                         uint64_t total_units, uint64_t per) {
  __shared__ float lds[8];  // two slots of one partial per wave
  uint32_t red = 0;
  UnitWalk w;
  TensorDesc d = {};
  uint32_t* slot = nullptr;  // of the matrix whose maximum `run` holds
  float run = 0.0f;
  const uint64_t first = blockIdx.x * per;
  const uint64_t stop = first + per < total_units ? first + per : total_units;
  for (uint64_t unit = first; unit < stop; ++unit) {
    if (unit >= w.next_prefix) walk_seek(w, d, descs, ndescs, unit);
    const uint64_t local = unit - d.units_prefix;
    uint32_t* s = reinterpret_cast<uint32_t*>(d.amax) + local / d.units_per_mat;
    // d, the unit and so the slot are uniform over the workgroup: all its
    // lanes publish together or not at all
    if (s != slot) {
      if (slot) tensor_publish(run, slot, lds, red);
      slot = s;
      run = 0.0f;
    }
    switch (static_cast<DType>(d.dtype)) {
      case DType::F32:
        run = fmaxf(run, tensor_unit_amax<float>(d, local));
        break;
      case DType::F16:
        run = fmaxf(run, tensor_unit_amax<__half>(d, local));
        break;
      default:
        run = fmaxf(run, tensor_unit_amax<__hip_bfloat16>(d, local));
        break;
    }
  }
  if (slot) tensor_publish(run, slot, lds, red);
}

__global__ void __launch_bounds__(256)
quant_tensor_convert_kernel(const TensorDesc* __restrict__ descs,
                            uint32_t ndescs, uint64_t total_units,
                            uint64_t per) {
  UnitWalk w;
  TensorDesc d = {};
  const uint64_t first = blockIdx.x * per;
  const uint64_t stop = first + per < total_units ? first + per : total_units;
  for (uint64_t i = first; i < stop; ++i) {
    // backwards from the last unit; the descriptor search only moves
    // forwards, so it starts over whenever the walk leaves a descriptor
    const uint64_t unit = total_units - 1 - i;
    if (unit >= w.next_prefix || unit < d.units_prefix) {
      w.lo = 0;
      walk_seek(w, d, descs, ndescs, unit);
    }
    const uint64_t local = unit - d.units_prefix;
    switch (static_cast<DType>(d.dtype)) {
      case DType::F32:
        tensor_unit_convert<float>(d, local);
        break;
      case DType::F16:
        tensor_unit_convert<__half>(d, local);
        break;
      default:
        tensor_unit_convert<__hip_bfloat16>(d, local);
        break;
    }
  }
}

__global__ void __launch_bounds__(256)
dequant_tensor_kernel(const TensorDesc* __restrict__ descs, uint32_t ndescs,
                      uint64_t total_units) {
  UnitWalk w;
  TensorDesc d = {};
  for (uint64_t unit = blockIdx.x; unit < total_units; unit += gridDim.x) {
    if (unit >= w.next_prefix) walk_seek(w, d, descs, ndescs, unit);
    const uint64_t local = unit - d.units_prefix;
    switch (static_cast<DType>(d.dtype)) {
      case DType::F32:
        tensor_dequant_unit<float>(d, local);
        break;
      case DType::F16:
        tensor_dequant_unit<__half>(d, local);
        break;
      default:
        tensor_dequant_unit<__hip_bfloat16>(d, local);
        break;
    }
  }
}

// launches of the three kernels, counted apart from the other formats': a
// quantise call adds 2, a dequantise call 1
static std::atomic<uint64_t> g_tensor_launches{0};

// Quantise: pass A and pass B back to back on `stream`, over the same staged
// descriptors.  Dequantise: one launch.  Grid cap (workgroups), from
// profiles/tensor_sync.log: the dequantise is best with one workgroup per
// unit, like the other quant kernels (65536); the quantise is best with
// several units per workgroup (8192), which makes a workgroup's running
// maximum span them and cuts the atomics on a large matrix's one slot to a
// quarter.  HIPSTORE_TENSOR_GRID sets both.
template <bool DEQUANT>
static void launch_quant_tensor(const Plan<TensorDesc>& p, int device,
                                hipStream_t stream) {
  if (p.descs.empty()) return;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(
      p.units, env_u32("HIPSTORE_TENSOR_GRID", 64, UINT32_MAX,
                       DEQUANT ? 65536 : 8192));
  const uint64_t per = (p.units + grid - 1) / grid;  // units per workgroup
  stage_descs_and_launch(device, stream, p.descs, [&](const TensorDesc* d) {
    const uint32_t n = (uint32_t)p.descs.size();
    if (DEQUANT) {
      hipLaunchKernelGGL(dequant_tensor_kernel, dim3(grid), dim3(256), 0,
                         stream, d, n, p.units);
    } else {
      hipLaunchKernelGGL(quant_tensor_amax_kernel, dim3(grid), dim3(256), 0,
                         stream, d, n, p.units, per);
      hipLaunchKernelGGL(quant_tensor_convert_kernel, dim3(grid), dim3(256), 0,
                         stream, d, n, p.units, per);
    }
  });
  g_tensor_launches.fetch_add(DEQUANT ? 1 : 2, std::memory_order_relaxed);
}
