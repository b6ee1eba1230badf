// MXFP6 (OCP Microscaling v1.0: packed e2m3 values, one e8m0 scale byte per
// 32-element block, "floor" scale rule) quantise / dequantise kernels, K8/K9.
//
// Format (per tensor, rows = the last dimension, blocks of 32 elements, the
// last block of a row may be short and its missing elements count as +0):
//   amax  = max |x| over the block
//   code  = max(expfield(amax) - 2, 0)      (stored, one byte per block)
//   v     = x * 2^(127 - code)              (one fp32 multiply)
//   q     = rne_e2m3(v), saturating at +-7.5, sign of v kept (also on zero)
//   y     = rne_dst(float(q) * 2^(code - 127))
// An e2m3 code is sign << 5 | exp << 3 | man.  Element k of a row occupies
// bits [6k, 6k + 6) of the row's byte string, little-endian (bit i of the
// string is bit i % 8 of byte i / 8); a row is ceil(3 cols / 4) bytes with
// zero padding bits, a full block exactly kMx6BlockBytes = 24 of them, and
// block b of a row starts at the row's byte 24 b: no byte is ever shared
// between blocks.  Scales, the exactness argument (integer work on the bits
// or one correctly rounded fp32 operation, no fast-math, no denormal
// flushing) and the treatment of non-finite input are those of quant_mx.h;
// the bytes equal those of the torch implementation in ops/mx6.py.
//
// The hardware conversions, as found on an MI355X against a host model of
// the format (all 64 codes, every tie midpoint and both of its fp32
// neighbours, the band (7.5, 8), +-0 and +-1e-30):
//   v_cvt_scalef32_2xpk16_fp6_f32 d, a, b, 1.0 interleaves its sources:
//     a[i] becomes element 2i and b[i] element 2i + 1 of the 32 (NOT the two
//     halves); the 192 bits are in the little-endian order above; ties go to
//     the even code; anything above 7.5 saturates to 7.5; the sign of the
//     input is kept on a zero result.
//   v_cvt_scalef32_pk32_f32_fp6 d, w, 1.0 returns element k in d[k], exact,
//     -0 for code 32.
// Both match the format as they are, so nothing is done in integer code.
// Feeding zeros as a[8..15] and b[8..15] packs 16 elements into the first
// three dwords (96 bits), and the last three dwords of the unpack are simply
// not used: a lane can own HALF a block.
//
// Work layout: units of kMxUnitBlocks blocks of one tensor, the unit walk and
// the descriptors are those of the MXFP4 kernels (plan.h).
//
// Fast path (wide and payload bases 16B aligned, cols % 32 == 0): block b of
// the tensor is elements [32 b, 32 b + 32), its payload the 24 bytes at 24 b.
// Two lanes own a block, 16 consecutive elements each, exactly as in
// quant_mx.h (one __shfl_xor joins the amax halves), so the wide side keeps
// the access pattern that won there.  A lane's 16 elements are 12 payload
// bytes, and adjacent lanes' 12 bytes are adjacent in memory.  How they
// travel is HIPSTORE_MX6_LDS (below).  Everything else takes the generic
// path: one lane per block converts all 32 (missing ones +0) and moves only
// the block's own ceil(3 n / 4) bytes, byte by byte.

#pragma once

#include "common.h"
#include "desc_ring.h"
#include "plan.h"
#include "quant_fp8.h"  // quant_mul / dequant_mul: the fma-fold fences
#include "quant_mx.h"   // scale helpers shared with MXFP4
#include "unit_walk.h"

#include <algorithm>
#include <atomic>

// Payload movement on the fast path.  0: every lane stores / loads its own 12
// bytes (one dwordx3, a wave covers 768 contiguous bytes).  1: the workgroup's
// pass of payload (128 blocks, 3072 contiguous bytes) is staged in LDS and
// crosses to memory as 16B per lane from 192 of the 256 lanes, at the price
// of two workgroup barriers per unit.  Measured on 1 GiB of bf16, both builds
// in one run (profiles/mx6_sync.log holds the chosen one): quantise 5.55 TB/s
// direct against 5.54 staged, the same within the 0.8 % scatter; dequantise
// 5.13 TB/s direct against 4.99 staged.  The 12B accesses of a wave are as
// contiguous as 16B ones would be, so the staging only adds its barriers: 0.
// Register count limits neither (occupancy 7 / 8, as in quant_mx.h).  A lane
// owning a whole block was not built: it is the wide-side pattern that lost
// in quant_mx.h, and the half-block conversion above removes its only
// attraction here, the conversion wanting 32 elements in one lane.
#ifndef HIPSTORE_MX6_LDS
#define HIPSTORE_MX6_LDS 0
#endif
static constexpr uint32_t kMx6Lds = HIPSTORE_MX6_LDS;
static_assert(kMx6Lds == 0 || kMx6Lds == 1, "direct or LDS-staged payload");
static constexpr uint32_t kMx6LaneElems = kMxBlock / 2u;   // 16
static constexpr uint32_t kMx6PassBlocks = 256u / 2u;      // 128 per pass
static constexpr uint32_t kMx6Passes = kMxUnitBlocks / kMx6PassBlocks;
static constexpr uint32_t kMx6PassWords = kMx6PassBlocks * kMx6BlockBytes / 4u;

typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v32f __attribute__((ext_vector_type(32)));
typedef uint32_t v6u __attribute__((ext_vector_type(6)));
// a lane's 12 bytes move as three dwords, which the compiler joins into one
// dwordx3 access (a 3-vector type would be padded to 16 bytes)
typedef __attribute__((address_space(1))) uint32_t gu32;

// N (16 or 32) already scaled values -> N / 16 * 3 dwords of packed codes
template <uint32_t N>
__device__ __forceinline__ void mx6_pack(const float* v, uint32_t* w) {
  v16f a, b;
#pragma unroll
  for (uint32_t i = 0; i < 16; ++i) {
    a[i] = 2 * i < N ? v[2 * i] : 0.0f;
    b[i] = 2 * i < N ? v[2 * i + 1] : 0.0f;
  }
  const v6u r = __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(a, b, 1.0f);
#pragma unroll
  for (uint32_t k = 0; k < N / 16u * 3u; ++k) w[k] = r[k];
}

// the reverse: the first N codes of six dwords -> their exact values as f32
template <uint32_t N>
__device__ __forceinline__ void mx6_unpack(const uint32_t* w, float* q) {
  v6u r;
#pragma unroll
  for (uint32_t k = 0; k < 6; ++k) r[k] = k < N / 16u * 3u ? w[k] : 0u;
  const v32f f = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(r, 1.0f);
#pragma unroll
  for (uint32_t k = 0; k < N; ++k) q[k] = f[k];
}

// generic path: where block gb of the tensor sits
struct Mx6BlockPos {
  uint64_t eoff;    // element offset of its first column
  uint64_t poff;    // byte offset of its first payload byte
  uint32_t n;       // its elements, 1..32
  uint32_t nbytes;  // its payload bytes, ceil(3 n / 4)
};

__device__ __forceinline__ Mx6BlockPos mx6_block_pos(const MxDesc& d,
                                                     uint32_t gb) {
  const uint32_t row = gb / d.nblk;
  const uint32_t b = gb - row * d.nblk;
  const uint32_t col0 = b * kMxBlock;
  const uint64_t row_bytes = (3ull * d.cols + 3u) / 4u;
  const uint32_t n = min(kMxBlock, d.cols - col0);
  return Mx6BlockPos{(uint64_t)row * d.cols + col0,
                     (uint64_t)row * row_bytes + b * kMx6BlockBytes, n,
                     (3u * n + 3u) / 4u};
}

// LDS-staged payload: the bytes of pass p of the unit that exist, and where
// they start.  The pass starts at a multiple of 3072 bytes, so 16B aligned;
// its end is a multiple of 24, so the last lane may move 8 bytes only.
struct Mx6Pass {
  uintptr_t base;
  uint32_t valid;  // bytes, 0 when the pass lies past the tensor
};

__device__ __forceinline__ Mx6Pass mx6_pass(const MxDesc& d,
                                            uint32_t local_unit, uint32_t p) {
  const uint32_t pb0 = local_unit * kMxUnitBlocks + p * kMx6PassBlocks;
  const uint32_t nb = pb0 < d.nblocks ? min(kMx6PassBlocks, d.nblocks - pb0) : 0u;
  return Mx6Pass{d.payload + (uint64_t)pb0 * kMx6BlockBytes,
                 nb * kMx6BlockBytes};
}

template <typename T>
__device__ __forceinline__ void mx6_quant_unit(const MxDesc& d,
                                               uint32_t local_unit,
                                               uint32_t* lds) {
  gu8* scales = reinterpret_cast<gu8*>(d.scales);
  if (d.fast) {
    constexpr uint32_t NV = kMx6LaneElems * sizeof(T) / 16u;  // loads per pass
    const uint32_t sub = threadIdx.x & 1u;
    const uint32_t gb0 = local_unit * kMxUnitBlocks + threadIdx.x / 2u;
    v4u raw[kMx6Passes][NV];
    // all loads of the unit first, as in quant_mx.h
#pragma unroll
    for (uint32_t p = 0; p < kMx6Passes; ++p) {
      const uint32_t gb = gb0 + p * kMx6PassBlocks;
#pragma unroll
      for (uint32_t k = 0; k < NV; ++k) raw[p][k] = v4u{0, 0, 0, 0};
      if (gb < d.nblocks) {
        const gv4u* s = reinterpret_cast<const gv4u*>(
            d.wide +
            ((uint64_t)gb * kMxBlock + sub * kMx6LaneElems) * sizeof(T));
#pragma unroll
        for (uint32_t k = 0; k < NV; ++k) raw[p][k] = s[k];
      }
    }
#pragma unroll
    for (uint32_t p = 0; p < kMx6Passes; ++p) {
      const uint32_t gb = gb0 + p * kMx6PassBlocks;
      T e[kMx6LaneElems];
      __builtin_memcpy(e, raw[p], sizeof(e));
      float x[kMx6LaneElems];
      uint32_t amax = 0;
#pragma unroll
      for (uint32_t k = 0; k < kMx6LaneElems; ++k) {
        x[k] = convert<T, float>(e[k]);
        amax = max(amax, mx_abs_bits(x[k]));
      }
      // the pair is live or dead as a whole, and the unit's descriptor is
      // uniform over the workgroup: all 64 lanes reach the shuffle
      amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1));
      const uint32_t code = mx_scale_code(amax);
      const float inv = mx_inv_scale(code);
#pragma unroll
      for (uint32_t k = 0; k < kMx6LaneElems; ++k) x[k] = quant_mul(x[k], inv);
      uint32_t w[3];
      mx6_pack<kMx6LaneElems>(x, w);
      if (kMx6Lds) {
        // dead lanes stage the zeros of their zero input; nobody reads them
        uint32_t* mine = lds + p * kMx6PassWords + 3u * threadIdx.x;
        mine[0] = w[0]; mine[1] = w[1]; mine[2] = w[2];
      }
      if (gb < d.nblocks) {
        if (!kMx6Lds) {
          gu32* out = reinterpret_cast<gu32*>(d.payload +
                                              (uint64_t)gb * kMx6BlockBytes +
                                              sub * (kMx6BlockBytes / 2u));
          out[0] = w[0]; out[1] = w[1]; out[2] = w[2];
        }
        if (sub == 0) scales[gb] = (uint8_t)code;
      }
    }
    if (kMx6Lds) {
      __syncthreads();
      const uint32_t off = 16u * threadIdx.x;
#pragma unroll
      for (uint32_t p = 0; p < kMx6Passes; ++p) {
        const Mx6Pass ps = mx6_pass(d, local_unit, p);
        const uint32_t* s = lds + p * kMx6PassWords + 4u * threadIdx.x;
        if (off + 16u <= ps.valid) {
          *reinterpret_cast<gv4u*>(ps.base + off) = v4u{s[0], s[1], s[2], s[3]};
        } else if (off + 8u <= ps.valid) {
          *reinterpret_cast<gv2u*>(ps.base + off) = v2u{s[0], s[1]};
        }
      }
      __syncthreads();  // the next unit stages into the same words
    }
    return;
  }
  // generic: lane t of the workgroup takes block t of the unit
  const uint32_t gb = local_unit * kMxUnitBlocks + threadIdx.x;
  if (gb >= d.nblocks) return;
  const Mx6BlockPos pos = mx6_block_pos(d, gb);
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
  uint32_t w[6];
  mx6_pack<kMxBlock>(x, w);
  // the missing elements are +0, code 0: the padding bits of a last partial
  // byte are 0, and no byte past the block's own is touched
#pragma unroll
  for (uint32_t j = 0; j < kMx6BlockBytes; ++j) {
    if (j < pos.nbytes) payload[j] = (uint8_t)(w[j / 4u] >> (8u * (j % 4u)));
  }
  scales[gb] = (uint8_t)code;
}

template <typename T>
__device__ __forceinline__ void mx6_dequant_unit(const MxDesc& d,
                                                 uint32_t local_unit,
                                                 uint32_t* lds) {
  const gu8* scales = reinterpret_cast<const gu8*>(d.scales);
  if (d.fast) {
    constexpr uint32_t NV = kMx6LaneElems * sizeof(T) / 16u;  // stores per pass
    const uint32_t sub = threadIdx.x & 1u;
    const uint32_t gb0 = local_unit * kMxUnitBlocks + threadIdx.x / 2u;
    uint32_t w[kMx6Passes][3];
    uint32_t code[kMx6Passes];
    if (kMx6Lds) {
      const uint32_t off = 16u * threadIdx.x;
#pragma unroll
      for (uint32_t p = 0; p < kMx6Passes; ++p) {
        const Mx6Pass ps = mx6_pass(d, local_unit, p);
        uint32_t* s = lds + p * kMx6PassWords + 4u * threadIdx.x;
        if (off + 16u <= ps.valid) {
          const v4u r = *reinterpret_cast<const gv4u*>(ps.base + off);
          s[0] = r[0]; s[1] = r[1]; s[2] = r[2]; s[3] = r[3];
        } else if (off + 8u <= ps.valid) {
          const v2u r = *reinterpret_cast<const gv2u*>(ps.base + off);
          s[0] = r[0]; s[1] = r[1];
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (uint32_t p = 0; p < kMx6Passes; ++p) {
      const uint32_t gb = gb0 + p * kMx6PassBlocks;
      w[p][0] = w[p][1] = w[p][2] = 0;
      code[p] = 0;
      if (gb < d.nblocks) {
        if (kMx6Lds) {
          const uint32_t* mine = lds + p * kMx6PassWords + 3u * threadIdx.x;
          w[p][0] = mine[0]; w[p][1] = mine[1]; w[p][2] = mine[2];
        } else {
          const gu32* in = reinterpret_cast<const gu32*>(
              d.payload + (uint64_t)gb * kMx6BlockBytes +
              sub * (kMx6BlockBytes / 2u));
          w[p][0] = in[0]; w[p][1] = in[1]; w[p][2] = in[2];
        }
        // the lanes of a pair read one address: a single broadcast fetch
        code[p] = scales[gb];
      }
    }
#pragma unroll
    for (uint32_t p = 0; p < kMx6Passes; ++p) {
      const uint32_t gb = gb0 + p * kMx6PassBlocks;
      if (gb >= d.nblocks) continue;
      const float scale = mx_scale(code[p]);
      float q[kMx6LaneElems];
      mx6_unpack<kMx6LaneElems>(w[p], q);
      T e[kMx6LaneElems];
#pragma unroll
      for (uint32_t k = 0; k < kMx6LaneElems; ++k)
        e[k] = convert<float, T>(dequant_mul(q[k], scale));
      v4u out[NV];
      __builtin_memcpy(out, e, sizeof(e));
      gv4u* dst = reinterpret_cast<gv4u*>(
          d.wide + ((uint64_t)gb * kMxBlock + sub * kMx6LaneElems) * sizeof(T));
#pragma unroll
      for (uint32_t k = 0; k < NV; ++k) dst[k] = out[k];
    }
    if (kMx6Lds) __syncthreads();  // the next unit stages into the same words
    return;
  }
  const uint32_t gb = local_unit * kMxUnitBlocks + threadIdx.x;
  if (gb >= d.nblocks) return;
  const Mx6BlockPos pos = mx6_block_pos(d, gb);
  T* dst = reinterpret_cast<T*>(d.wide) + pos.eoff;
  const gu8* payload = reinterpret_cast<const gu8*>(d.payload) + pos.poff;
  const float scale = mx_scale(scales[gb]);
  uint32_t w[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (uint32_t j = 0; j < kMx6BlockBytes; ++j) {
    if (j < pos.nbytes) w[j / 4u] |= (uint32_t)payload[j] << (8u * (j % 4u));
  }
  float q[kMxBlock];
  mx6_unpack<kMxBlock>(w, q);
#pragma unroll
  for (uint32_t c = 0; c < kMxBlock; ++c) {
    if (c < pos.n) dst[c] = convert<float, T>(dequant_mul(q[c], scale));
  }
}

template <bool DEQUANT>
__global__ void __launch_bounds__(256)
quant_mx6_kernel(const MxDesc* __restrict__ descs, uint32_t ndescs,
                 uint64_t total_units) {
  __shared__ uint32_t lds[kMx6Lds ? kMx6Passes * kMx6PassWords : 1];
  UnitWalk w;
  MxDesc d = {};
  for (uint64_t unit = blockIdx.x; unit < total_units; unit += gridDim.x) {
    if (unit >= w.next_prefix) walk_seek(w, d, descs, ndescs, unit);
    const uint32_t local = (uint32_t)(unit - d.units_prefix);
    // d is uniform over the workgroup: every wave takes one branch whole
    switch (static_cast<DType>(d.dtype)) {
      case DType::F32:
        if (DEQUANT) mx6_dequant_unit<float>(d, local, lds);
        else mx6_quant_unit<float>(d, local, lds);
        break;
      case DType::F16:
        if (DEQUANT) mx6_dequant_unit<__half>(d, local, lds);
        else mx6_quant_unit<__half>(d, local, lds);
        break;
      default:
        if (DEQUANT) mx6_dequant_unit<__hip_bfloat16>(d, local, lds);
        else mx6_quant_unit<__hip_bfloat16>(d, local, lds);
        break;
    }
  }
}

// launches of either kernel, counted apart from the FP8 and MXFP4 ones
static std::atomic<uint64_t> g_mx6_launches{0};

// One launch of either kernel, async on `stream`.  Grid cap (workgroups):
// the sweep on 1 GiB of bf16 (profiles/mx6_sync.log) gained all the way up to
// 65536, about one unit per workgroup, and nothing beyond (262144): 5.53 TB/s
// quant and 5.15 dequant against 5.01 / 4.35 at 1024
template <bool DEQUANT>
static void launch_quant_mx6(const Plan<MxDesc>& p, int device,
                             hipStream_t stream) {
  if (p.descs.empty()) return;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(
      p.units, env_u32("HIPSTORE_MX6_GRID", 64, UINT32_MAX, 65536));
  stage_descs_and_launch(device, stream, p.descs, [&](const MxDesc* d) {
    hipLaunchKernelGGL(quant_mx6_kernel<DEQUANT>, dim3(grid), dim3(256), 0,
                       stream, d, (uint32_t)p.descs.size(), p.units);
  });
  g_mx6_launches.fetch_add(1, std::memory_order_relaxed);
}
