// Tile-scaled FP8 (OCP e4m3, one f32 scale per 128 x 128 tile) quantise /
// dequantise kernels — K12/K13.
//
// Format.  A tensor is a stack of matrices [*lead, R, C] (a 1-D tensor of n
// elements is the matrix [1, n]); each matrix is cut into 128 x 128 tiles,
// the last tile of a tile row or column may be short, and a tile never
// crosses a leading index.  The payload is e4m3 in the source's shape, the
// scales are f32 [*lead, ceil(R / 128), ceil(C / 128)]: the layout of
// block-FP8 weights (weight_block_size = [128, 128]), the stored scale being
// the dequantisation multiplier (weight_scale_inv).  Per tile:
//   amax  = max(max|x| over the tile, 2^-96)
//   scale = amax / 448            (stored, f32)
//   q     = rne_e4m3(clamp(x * (448 / amax), -448, 448))
//   y     = rne_dst(float(q) * scale)
// This is the recipe of quant_fp8.h with the tile as the block: every step is
// one correctly rounded IEEE fp32 operation (no fast-math here), the fences
// quant_mul / dequant_mul and the conversions are the ones of that file, and
// max is exact and associative on finite values, so whatever tree reduces the
// tile, the bytes equal those of the torch implementation in
// ops/quant_tile.py.  Non-finite input is outside the contract.
//
// Quantise (K12).  The reduction is two-dimensional: 128 row segments of 256 B
// (bf16/f16) or 512 B (f32) that lie `cols` elements apart.  A unit is one
// tile, numbered like its scale with the tile column fastest, so neighbouring
// workgroups read neighbouring segments of the same rows.  The 256-thread
// workgroup holds the whole tile in registers and reads HBM once: 8 lanes own
// one tile row, 16 consecutive elements each (the wide-side pattern of K4),
// the workgroup covers 32 rows per pass and takes kTilePasses = 4 passes, all
// loads issued before the first dependent instruction: 32 (bf16/f16) or 64
// (f32) raw VGPRs per lane.  Rows and 16-element chunks beyond the matrix
// edge are predicated and contribute 0.0f.  The amax is reduced over the
// lane's 64 values, over the wave by shuffles, then lane 0 of each wave
// writes one float to LDS, one barrier, and every lane reads the four
// partials (row_reduce of quant_row.h, with its two alternating slots: one
// barrier per tile however many tiles a workgroup takes).  The lanes convert
// from registers and make one 16 B payload store per pass; one lane stores
// the scale.  An unaligned base or cols % 16 != 0 takes the generic path: the
// same tile ownership and reduction, the 8 lanes of a row striding over its
// 128 columns element by element, twice (amax, then convert), and storing
// payload bytes singly, so nothing is written past a row or a tile.  Every
// lane of the workgroup reaches the shuffles and the barrier of every unit:
// the descriptor and the unit are uniform, and edges are predicated.
//
// Dequantise (K13) is element-wise: a unit is kTileDqPasses passes of the
// workgroup over consecutive 16-element chunks of the whole tensor (the flat
// pattern of K5 and K11).  With cols % 16 == 0 a chunk lies in one tile,
// whose scale index is (mat * ntr + row / 128) * ntc + col / 128 from the
// 64-bit element offset; the generic path takes the index per element.
//
// Resources (plain hipcc -O3 for gfx950, resource-usage remarks): quantise 94
// VGPRs, occupancy 5, dequantise 36 VGPRs, occupancy 8; neither uses scratch
// or spills a register.
//
// Measured on an MI355X, 1 GiB of bf16 per shape, the block-scaled kernels
// (K4/K5) on the same data in the same run as the yardstick
// (profiles/tile_sync.log; read + write, medians of 3 x 300 calls, the four
// kernels taking their repeats in turn, scatter at most 1 %, of these two
// kernels at most 0.16 %):
//   shape            tiles    quant        vs K4    dequant      vs K5
//   131072 x 4096    32768    5.47 TB/s    0.97     5.47 TB/s    1.00
//   37449 x 14336    32816    5.37 TB/s    0.95     5.46 TB/s    1.00
//   8192 x 65536     32768    5.43 TB/s    0.96     5.48 TB/s    1.00
// The quantise moves K4's bytes once; the barrier per 32 KiB tile and the
// 256 B bursts cost 3 to 5 %, what the wave and held regimes of quant_row.h
// cost.  One variant was tried, a grid cap below the tile count, so that a
// workgroup takes several tiles: it loses everywhere (quantise 5.25 / 5.14 /
// 5.20 TB/s at 8192 workgroups, 5.12 / 4.98 / 5.01 at 2048; dequantise 4.78
// and 4.63), so the cap stays at one workgroup per tile up to 65536.

#pragma once

#include "common.h"
#include "desc_ring.h"
#include "plan.h"
#include "quant_row.h"  // wave_max, row_reduce, row_amax16, row_cvt16
#include "unit_walk.h"

#include <algorithm>
#include <atomic>

// where a tile lies: unit = (mat * ntr + tile_row) * ntc + tile_col
struct TilePos {
  uint64_t row0;  // first row of the tile, counted over the whole stack
  uint64_t col0;  // first column
  uint32_t nrows; // rows and columns of the tile that exist (1..128)
  uint32_t ncols;
};

__device__ __forceinline__ TilePos tile_pos(const TileDesc& d, uint64_t unit) {
  const uint64_t rest = unit / d.ntc;
  const uint64_t tc = unit - rest * d.ntc;
  const uint64_t mat = rest / d.ntr;
  const uint64_t tr = rest - mat * d.ntr;
  TilePos t;
  t.row0 = mat * d.rows + tr * kTile;
  t.col0 = tc * kTile;
  const uint64_t rows_left = d.rows - tr * kTile;
  const uint64_t cols_left = d.cols - t.col0;
  t.nrows = rows_left < kTile ? (uint32_t)rows_left : kTile;
  t.ncols = cols_left < kTile ? (uint32_t)cols_left : kTile;
  return t;
}

// fast path: lane (g, gl) takes the 16 elements at column 16 gl of tile row
// 32 p + g in pass p
template <typename T>
__device__ __forceinline__ void tile_quant_fast(const TileDesc& d,
                                                uint64_t unit, float* lds,
                                                uint32_t& red) {
  const uint32_t g = threadIdx.x >> 3;
  const uint32_t gl = threadIdx.x & 7u;
  const TilePos t = tile_pos(d, unit);
  // cols % 16 == 0: all 16 elements of a chunk or none
  const bool col_live = gl * 16u < t.ncols;
  const uint64_t e0 = (t.row0 + g) * d.cols + t.col0 + gl * 16u;
  const uint64_t pass_stride = 32ull * d.cols;
  QuantRaw<T> raw[kTilePasses];
  bool live[kTilePasses];
  // all loads of the tile first: 128 B (bf16/f16) or 256 B (f32) in flight
  // per lane before the first dependent instruction
#pragma unroll
  for (uint32_t p = 0; p < kTilePasses; ++p) {
    live[p] = col_live && p * 32u + g < t.nrows;
#pragma unroll
    for (uint32_t k = 0; k < sizeof(T); ++k) raw[p].q[k] = v4u{0, 0, 0, 0};
    if (live[p]) {
      const gv4u* s = reinterpret_cast<const gv4u*>(
          d.wide + (e0 + p * pass_stride) * sizeof(T));
#pragma unroll
      for (uint32_t k = 0; k < sizeof(T); ++k) raw[p].q[k] = s[k];
    }
  }
  float amax = 0.0f;  // dead chunks hold zeros and add nothing
#pragma unroll
  for (uint32_t p = 0; p < kTilePasses; ++p)
    amax = fmaxf(amax, row_amax16<T>(raw[p]));
  amax = fmaxf(row_reduce<true>(amax, lds, red), kAmaxFloor);
  const float inv = kFp8Max / amax;
#pragma unroll
  for (uint32_t p = 0; p < kTilePasses; ++p) {
    if (live[p])
      *reinterpret_cast<gv4u*>(d.payload + e0 + p * pass_stride) =
          row_cvt16<T>(raw[p], inv);
  }
  if (threadIdx.x == 0) reinterpret_cast<float*>(d.scales)[unit] = amax / kFp8Max;
}

// generic path: lane gl of a row's 8 takes columns gl, gl + 8, ... of the tile
template <typename T>
__device__ __forceinline__ void tile_quant_generic(const TileDesc& d,
                                                   uint64_t unit, float* lds,
                                                   uint32_t& red) {
  const uint32_t g = threadIdx.x >> 3;
  const uint32_t gl = threadIdx.x & 7u;
  const TilePos t = tile_pos(d, unit);
  const T* src = reinterpret_cast<const T*>(d.wide);
  uint8_t* payload = reinterpret_cast<uint8_t*>(d.payload);
  const uint64_t e0 = (t.row0 + g) * d.cols + t.col0;
  const uint64_t pass_stride = 32ull * d.cols;
  // twice over the tile, for the amax and to convert: the second read comes
  // from cache, and no lane holds more than one element
  float amax = 0.0f;
  for (uint32_t p = 0; p < kTilePasses; ++p) {
    if (p * 32u + g >= t.nrows) continue;
    for (uint32_t c = gl; c < t.ncols; c += 8u)
      amax = fmaxf(amax,
                   fabsf(convert<T, float>(src[e0 + p * pass_stride + c])));
  }
  // lanes leave the loops at different trips and meet again before the barrier
  amax = fmaxf(row_reduce<true>(amax, lds, red), kAmaxFloor);
  const float inv = kFp8Max / amax;
  for (uint32_t p = 0; p < kTilePasses; ++p) {
    if (p * 32u + g >= t.nrows) continue;
    for (uint32_t c = gl; c < t.ncols; c += 8u) {
      const uint64_t e = e0 + p * pass_stride + c;
      const float v = quant_scaled(convert<T, float>(src[e]), inv);
      const int packed = __builtin_amdgcn_cvt_pk_fp8_f32(v, v, 0, false);
      payload[e] = (uint8_t)(packed & 0xff);
    }
  }
  if (threadIdx.x == 0) reinterpret_cast<float*>(d.scales)[unit] = amax / kFp8Max;
}

// scale of the element at offset `eoff` of the tensor
__device__ __forceinline__ uint64_t tile_scale_index(const TileDesc& d,
                                                     uint64_t eoff) {
  const uint64_t grow = eoff / d.cols;  // row of the whole stack: 32 bits
  const uint32_t col = (uint32_t)(eoff - grow * d.cols);
  const uint32_t mat = (uint32_t)grow / d.rows;
  const uint32_t row = (uint32_t)grow - mat * d.rows;
  return ((uint64_t)mat * d.ntr + row / kTile) * d.ntc + col / kTile;
}

template <typename T>
__device__ __forceinline__ void tile_dequant_unit(const TileDesc& d,
                                                  uint64_t local_unit) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const float* scales = reinterpret_cast<const float*>(d.scales);
  const uint64_t base = local_unit * kTileDqUnitElems;
  if (d.fast) {
    v4u raw[kTileDqPasses];
    float scale[kTileDqPasses];
    uint64_t eoff[kTileDqPasses];
#pragma unroll
    for (uint32_t p = 0; p < kTileDqPasses; ++p) {
      eoff[p] = base + (p * 256u + threadIdx.x) * 16u;
      raw[p] = v4u{0, 0, 0, 0};
      scale[p] = 0.0f;
      if (eoff[p] < d.numel) {  // numel % 16 == 0: all 16 elements or none
        raw[p] = *reinterpret_cast<const gv4u*>(d.payload + eoff[p]);
        // cols % 16 == 0: the chunk lies in one row and, 16 dividing 128, in
        // one tile; the 8 lanes of a tile row read one address
        scale[p] = scales[tile_scale_index(d, eoff[p])];
      }
    }
#pragma unroll
    for (uint32_t p = 0; p < kTileDqPasses; ++p) {
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
      base + kTileDqUnitElems < d.numel ? base + kTileDqUnitElems : d.numel;
  for (uint64_t e = base + threadIdx.x; e < end; e += 256u) {
    const f32x2 v = __builtin_amdgcn_cvt_pk_f32_fp8((int)payload[e], false);
    dst[e] = convert<float, T>(dequant_mul(v[0], scales[tile_scale_index(d, e)]));
  }
}

template <typename T, bool DEQUANT>
__device__ __forceinline__ void tile_unit(const TileDesc& d, uint64_t local,
                                          float* lds, uint32_t& red) {
  if (DEQUANT) tile_dequant_unit<T>(d, local);
  else if (d.fast) tile_quant_fast<T>(d, local, lds, red);
  else tile_quant_generic<T>(d, local, lds, red);
}

template <bool DEQUANT>
__global__ void __launch_bounds__(256)
quant_tile_kernel(const TileDesc* __restrict__ descs, uint32_t ndescs,
                  uint64_t total_units) {
  __shared__ float lds[8];  // two slots of one partial per wave
  uint32_t red = 0;
  UnitWalk w;
  TileDesc d = {};
  for (uint64_t unit = blockIdx.x; unit < total_units; unit += gridDim.x) {
    if (unit >= w.next_prefix) walk_seek(w, d, descs, ndescs, unit);
    const uint64_t local = unit - d.units_prefix;
    // d and the unit are uniform over the workgroup: all its lanes take one
    // branch and meet at the one barrier of the tile
    switch (static_cast<DType>(d.dtype)) {
      case DType::F32:
        tile_unit<float, DEQUANT>(d, local, lds, red);
        break;
      case DType::F16:
        tile_unit<__half, DEQUANT>(d, local, lds, red);
        break;
      default:
        tile_unit<__hip_bfloat16, DEQUANT>(d, local, lds, red);
        break;
    }
  }
}

// launches of either kernel, counted apart from the other formats'
static std::atomic<uint64_t> g_tile_launches{0};

// One launch of either kernel, async on `stream`, at most HIPSTORE_TILE_GRID
// workgroups (65536, the other quant kernels' cap)
template <bool DEQUANT>
static void launch_quant_tile(const Plan<TileDesc>& p, int device,
                              hipStream_t stream) {
  if (p.descs.empty()) return;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(
      p.units, env_u32("HIPSTORE_TILE_GRID", 64, UINT32_MAX, 65536));
  stage_descs_and_launch(device, stream, p.descs, [&](const TileDesc* d) {
    hipLaunchKernelGGL(quant_tile_kernel<DEQUANT>, dim3(grid), dim3(256), 0,
                       stream, d, (uint32_t)p.descs.size(), p.units);
  });
  g_tile_launches.fetch_add(1, std::memory_order_relaxed);
}
