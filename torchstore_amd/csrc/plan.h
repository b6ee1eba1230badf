// Launch planning: descriptor layouts and the pure functions that turn the
// unpacked python tuples into {descriptors, unit count}.
//
// HIP-free on purpose (<cstdint>, <vector>, <stdexcept> only): the same
// header builds into the extension and into tests/native/plan_check.cpp,
// which checks on the CPU that the units of a plan cover every byte once.

#pragma once

#include <cstdint>
#include <stdexcept>
#include <vector>

static constexpr int kMaxDims = 7;  // outer dims (innermost is the row)

// row-packed units span this many bytes of small rows regardless of the
// launch tile (64 KiB won the scatter sweep at every grid size)
static constexpr uint32_t kRowPackSpan = 65536u;

static constexpr uint32_t kQuantBlock = 128;
static constexpr uint32_t kQuantPasses = 2;
static constexpr uint32_t kQuantUnitBlocks = 32 * kQuantPasses;

// MXFP4: 32-element blocks (OCP Microscaling); a unit is one pass of a
// 256-thread workgroup with a block per lane, or two with a block per lane
// pair, so its size does not depend on how quant_mx.h lays the lanes out
static constexpr uint32_t kMxBlock = 32;
static constexpr uint32_t kMxUnitBlocks = 256;

// MXFP6 (e2m3): the same blocks, units, descriptor (MxDesc) and planner
// (plan_mx, whose fast rule "both bases 16B aligned, whole blocks only" is
// also what quant_mx6.h needs); only the payload differs, 6 bits per element:
// a full block is 24 bytes, a row ceil(3 cols / 4), and the kernels derive
// both from `cols`
static constexpr uint32_t kMx6BlockBytes = kMxBlock * 6 / 8;

// Row-scaled FP8 (K10/K11): one f32 scale per row, so the quantise side
// reduces over a whole row and picks its work split per tensor from `cols`:
//   cols <= kRowWave            a wave holds the row in registers
//   kRowWave < cols <= kRowWg   the workgroup holds the row in registers
//   cols > kRowWg               the workgroup streams the row twice
// Both limits are the register capacity of the kernels (kRowSteps 16-element
// steps per lane) and the defaults of the planner; quant_row.h tells how they
// were settled.
static constexpr uint32_t kRowSteps = 4;
static constexpr uint32_t kRowWave = kRowSteps * 64u * 16u;   // 4096
static constexpr uint32_t kRowWg = kRowSteps * 256u * 16u;    // 16384
static constexpr uint32_t kRowWaveRows = 4;   // rows per unit, one per wave
// dequantise is flat: a unit is kRowDqPasses passes of 256 lanes x 16 elements
static constexpr uint32_t kRowDqPasses = 2;
static constexpr uint32_t kRowDqUnitElems = kRowDqPasses * 256u * 16u;

// Tile-scaled FP8 (K12/K13): one f32 scale per kTile x kTile tile of each
// matrix of a stack [mats, rows, cols].  A quantise unit is one tile, which a
// 256-thread workgroup holds in registers: 8 lanes per tile row, 32 rows per
// pass, kTilePasses passes.  Dequantise is flat like K11.
static constexpr uint32_t kTile = 128;
static constexpr uint32_t kTilePasses = kTile / 32u;
static constexpr uint32_t kTileDqPasses = 2;
static constexpr uint32_t kTileDqUnitElems = kTileDqPasses * 256u * 16u;

// Per-tensor FP8 (K14/K15): one f32 scale per matrix of a stack [mats, rows,
// cols].  A quantise unit is a run of up to kTensorUnitElems elements that
// lies inside ONE matrix (kTensorPasses passes of 256 lanes x 16 elements),
// counted per matrix, so a unit never straddles two scales; both quantise
// launches walk the same units.  Dequantise is flat like K13.
static constexpr uint32_t kTensorPasses = 4;
static constexpr uint32_t kTensorUnitElems = kTensorPasses * 256u * 16u;
static constexpr uint32_t kTensorDqPasses = 2;
static constexpr uint32_t kTensorDqUnitElems = kTensorDqPasses * 256u * 16u;
// largest tensor of one descriptor: byte offsets of an f32 tensor stay below
// 2^49 and no product of the planner or the kernels leaves 64 bits
static constexpr uint64_t kTensorMaxElems = 1ull << 47;

// descriptors (read by the kernels; every one carries the exclusive prefix
// sum of units that unit_walk.h searches)

// K1/K2: rows of `row_bytes` contiguous bytes; row r's source/dest offsets
// come from the outer-dims multi-index against byte strides.  Work unit =
// one tile of one row, or `rows_per_unit` whole rows when row-packed.
struct SliceDesc {
  uintptr_t src;
  uintptr_t dst;
  uint64_t rows;            // product of outer dims
  uint64_t units_prefix;    // exclusive prefix sum of units
  uint32_t row_bytes;
  uint32_t tiles_per_row;
  uint32_t ndim;            // number of outer dims
  // >1 = row-packed: one unit covers this many consecutive rows (small
  // rows, ndim<=1, fully 16B-aligned — the reshard scatter case, where a
  // per-row unit would pay desc-load + search overhead per ~1 KB of work)
  uint32_t rows_per_unit;
  uint64_t shape[kMaxDims];       // outer dims, innermost-last
  int64_t src_stride[kMaxDims];   // byte strides of outer dims
  int64_t dst_stride[kMaxDims];
};
static_assert(sizeof(SliceDesc) == 216, "SliceDesc is meant to be 216 bytes");

// flat copy: unit = one `span`-byte piece of one contiguous range
struct FlatDesc {
  uintptr_t src;
  uintptr_t dst;
  uint64_t nbytes;        // multiple of 16, > 0
  uint64_t units_prefix;  // exclusive prefix sum of units
};
static_assert(sizeof(FlatDesc) == 32, "FlatDesc is meant to be 32 bytes");

// K4/K5: unit = kQuantUnitBlocks consecutive 128-element blocks of a tensor
struct QuantDesc {
  uintptr_t wide;         // f32/bf16/f16 tensor: quant source, dequant dest
  uintptr_t payload;      // e4m3 bytes, same element order as `wide`
  uintptr_t scales;       // f32 [rows, nblk]
  uint64_t rows;
  uint64_t units_prefix;  // exclusive prefix sum of units
  uint32_t cols;
  uint32_t nblk;          // blocks per row = ceil(cols / 128)
  uint32_t nblocks;       // rows * nblk
  uint32_t dtype;         // DType code of `wide` (0 = f32, 1 = f16, 2 = bf16)
  uint32_t fast;          // 1 = 16B-vector path
  uint32_t pad_;
};
static_assert(sizeof(QuantDesc) == 64, "QuantDesc is meant to be 64 bytes");

// K6/K7 and K8/K9: unit = kMxUnitBlocks consecutive 32-element blocks of a
// tensor
struct MxDesc {
  uintptr_t wide;         // f32/bf16/f16 tensor: quant source, dequant dest
  uintptr_t payload;      // packed e2m1, rows of ceil(cols / 2) bytes
                          // (MXFP6: packed e2m3, rows of ceil(3 cols / 4))
  uintptr_t scales;       // e8m0 bytes [rows, nblk]
  uint64_t rows;
  uint64_t units_prefix;  // exclusive prefix sum of units
  uint32_t cols;
  uint32_t nblk;          // blocks per row = ceil(cols / 32)
  uint32_t nblocks;       // rows * nblk
  uint32_t dtype;         // DType code of `wide` (0 = f32, 1 = f16, 2 = bf16)
  uint32_t fast;          // 1 = 16B-vector path (block b sits at element 32 b)
  uint32_t pad_;
};
static_assert(sizeof(MxDesc) == 64, "MxDesc is meant to be 64 bytes");

// K10/K11: quantise unit = kRowWaveRows rows (mode 0) or one row (modes 1,
// 2); dequantise unit = kRowDqUnitElems consecutive elements
enum RowMode : uint32_t { kRowModeWave = 0, kRowModeHeld = 1, kRowModeStream = 2 };
struct RowDesc {
  uintptr_t wide;         // f32/bf16/f16 tensor: quant source, dequant dest
  uintptr_t payload;      // e4m3 bytes, same element order as `wide`
  uintptr_t scales;       // f32 [rows]
  uint64_t rows;
  uint64_t units_prefix;  // exclusive prefix sum of units
  uint64_t numel;         // rows * cols
  uint32_t cols;
  uint32_t dtype;         // DType code of `wide` (0 = f32, 1 = f16, 2 = bf16)
  uint32_t mode;          // RowMode of the quantise side
  uint32_t fast;          // 1 = 16B-vector path
};
static_assert(sizeof(RowDesc) == 64, "RowDesc is meant to be 64 bytes");

// K12/K13: quantise unit = one tile, numbered like its scale, the tile column
// fastest: unit = (mat * ntr + tile_row) * ntc + tile_col; dequantise unit =
// kTileDqUnitElems consecutive elements
struct TileDesc {
  uintptr_t wide;         // f32/bf16/f16 tensor: quant source, dequant dest
  uintptr_t payload;      // e4m3 bytes, same element order as `wide`
  uintptr_t scales;       // f32 [mats, ntr, ntc]
  uint64_t units_prefix;  // exclusive prefix sum of units
  uint64_t numel;         // mats * rows * cols
  uint32_t rows;          // of one matrix; mats * rows fits 32 bits
  uint32_t cols;
  uint32_t ntr;           // tile rows per matrix = ceil(rows / 128)
  uint32_t ntc;           // tile columns = ceil(cols / 128)
  uint32_t dtype;         // DType code of `wide` (0 = f32, 1 = f16, 2 = bf16)
  uint32_t fast;          // 1 = 16B-vector path
};
static_assert(sizeof(TileDesc) == 64, "TileDesc is meant to be 64 bytes");

// K14/K15: quantise unit = the run [u * kTensorUnitElems, ...) of matrix
// `mat`, unit = mat * units_per_mat + u; dequantise unit = kTensorDqUnitElems
// consecutive elements of the whole tensor
struct TensorDesc {
  uintptr_t wide;          // f32/bf16/f16 tensor: quant source, dequant dest
  uintptr_t payload;       // e4m3 bytes, same element order as `wide`
  uintptr_t scales;        // f32 [mats]
  uintptr_t amax;          // u32 [mats]: bit patterns of the matrices' amax,
                           // zeroed before the quantise; 0 on the dequant side
  uint64_t units_prefix;   // exclusive prefix sum of units
  uint64_t numel;          // mats * mat_elems
  uint64_t mat_elems;      // rows * cols of one matrix
  uint64_t units_per_mat;  // quantise units of one matrix
  uint32_t dtype;          // DType code of `wide` (0 = f32, 1 = f16, 2 = bf16)
  uint32_t fast;           // 1 = 16B-vector path
};
static_assert(sizeof(TensorDesc) == 72, "TensorDesc is meant to be 72 bytes");

template <typename Desc>
struct Plan {
  std::vector<Desc> descs;
  uint64_t units = 0;
};

// inputs: one python tuple each, already unpacked

// (src_ptr, dst_ptr, row_bytes, [outer shape], [src strides B], [dst strides B])
// the three arrays hold `ndim` entries; a flat byte copy has ndim == 0
struct SliceIn {
  uintptr_t src, dst;
  uint64_t row_bytes;
  const uint64_t* shape;
  const int64_t *src_stride, *dst_stride;
  uint32_t ndim;
};

// (wide_ptr, payload_ptr, scales_ptr, rows, cols, wide_dtype)
struct QuantIn {
  uintptr_t wide, payload, scales;
  uint64_t rows, cols;
  int dtype;
};

// (wide_ptr, payload_ptr, scales_ptr, mats, rows, cols, wide_dtype)
struct TileIn {
  uintptr_t wide, payload, scales;
  uint64_t mats, rows, cols;
  int dtype;
};

// (wide_ptr, payload_ptr, scales_ptr, amax_ptr, mats, rows, cols, wide_dtype)
struct TensorIn {
  uintptr_t wide, payload, scales, amax;
  uint64_t mats, rows, cols;
  int dtype;
};

inline uint64_t slice_rows(const SliceIn& s) {
  uint64_t rows = 1;
  for (uint32_t k = 0; k < s.ndim; ++k) rows *= s.shape[k];
  return rows;
}

inline uint64_t total_bytes(const std::vector<SliceIn>& in) {
  uint64_t total = 0;
  for (const SliceIn& s : in) total += slice_rows(s) * s.row_bytes;
  return total;
}

// planners

// General slice plan.  A slice is row-packed when it has <=1 outer dim, more
// than one row, everything 16B-aligned and at least TWO rows fit a unit; a
// wider row keeps its tiles (a "pack" of one row would copy one tile of it).
inline Plan<SliceDesc> plan_slices(const std::vector<SliceIn>& in,
                                   uint32_t tile) {
  Plan<SliceDesc> p;
  p.descs.resize(in.size());
  for (size_t i = 0; i < in.size(); ++i) {
    const SliceIn& s = in[i];
    SliceDesc& d = p.descs[i];
    if (s.ndim > (uint32_t)kMaxDims) throw std::runtime_error("too many dims");
    if (s.row_bytes > UINT32_MAX) throw std::runtime_error("row too large");
    d = SliceDesc{};
    d.src = s.src;
    d.dst = s.dst;
    d.ndim = s.ndim;
    d.rows = slice_rows(s);
    for (uint32_t k = 0; k < s.ndim; ++k) {
      d.shape[k] = s.shape[k];
      d.src_stride[k] = s.src_stride[k];
      d.dst_stride[k] = s.dst_stride[k];
    }
    d.row_bytes = (uint32_t)s.row_bytes;
    d.tiles_per_row = (uint32_t)((s.row_bytes + tile - 1) / tile);
    if (d.tiles_per_row == 0) d.tiles_per_row = 1;
    d.rows_per_unit = 1;
    const bool aligned16 =
        s.row_bytes > 0 && (s.row_bytes & 15u) == 0 && (d.src & 15u) == 0 &&
        (d.dst & 15u) == 0 &&
        (d.ndim == 0 ||
         ((d.src_stride[0] & 15) == 0 && (d.dst_stride[0] & 15) == 0));
    if (d.ndim <= 1 && d.rows > 1 && aligned16 &&
        s.row_bytes * 2 <= kRowPackSpan) {
      d.rows_per_unit = (uint32_t)(kRowPackSpan / s.row_bytes);
      d.tiles_per_row = 1;
    }
    d.units_prefix = p.units;
    p.units += d.rows_per_unit > 1
                   ? (d.rows + d.rows_per_unit - 1) / d.rows_per_unit
                   : d.rows * d.tiles_per_row;
  }
  return p;
}

// A launch is flat when every slice is one contiguous 16B-aligned range of
// less than 4 GiB; a single odd entry keeps the whole launch on the general
// kernel (returns false, `out` is then meaningless).  Zero-byte entries are
// dropped, so a flat plan may come back with no units at all.
inline bool plan_flat(const std::vector<SliceIn>& in, uint32_t span,
                      Plan<FlatDesc>& out) {
  out.descs.clear();
  out.descs.reserve(in.size());
  out.units = 0;
  for (const SliceIn& s : in) {
    if (s.ndim != 0 || s.row_bytes > UINT32_MAX) return false;
    if (((s.src | s.dst | (uintptr_t)s.row_bytes) & 15u) != 0) return false;
    if (s.row_bytes == 0) continue;
    out.descs.push_back(FlatDesc{s.src, s.dst, s.row_bytes, out.units});
    out.units += (s.row_bytes + span - 1) / span;
  }
  return true;
}

// Quant / dequant plan; tensors with no elements are dropped.
inline Plan<QuantDesc> plan_quant(const std::vector<QuantIn>& in) {
  Plan<QuantDesc> p;
  p.descs.reserve(in.size());
  for (const QuantIn& it : in) {
    if (it.dtype < 0 || it.dtype > 2)
      throw std::runtime_error("unsupported dtype");
    if (it.rows == 0 || it.cols == 0) continue;
    const uint64_t nblk = (it.cols + kQuantBlock - 1) / kQuantBlock;
    const uint64_t nblocks = it.rows * nblk;
    if (it.cols > UINT32_MAX || nblocks > (1ull << 31))
      throw std::runtime_error("tensor too large for one quant descriptor");
    if (it.scales & 3u) throw std::runtime_error("scales must be 4B aligned");
    const uint32_t es = it.dtype == 0 ? 4u : 2u;
    if (it.wide % es) throw std::runtime_error("misaligned tensor");
    const uint32_t fast =
        (((it.wide | it.payload) & 15u) == 0 && (it.cols & 15u) == 0) ? 1u : 0u;
    p.descs.push_back(QuantDesc{it.wide, it.payload, it.scales, it.rows,
                                p.units, (uint32_t)it.cols, (uint32_t)nblk,
                                (uint32_t)nblocks, (uint32_t)it.dtype, fast, 0});
    p.units += (nblocks + kQuantUnitBlocks - 1) / kQuantUnitBlocks;
  }
  return p;
}

// MXFP4 quant / dequant plan, from the same tuples as plan_quant (the scales
// are bytes here, so they need no alignment); tensors with no elements are
// dropped.  Fast needs whole blocks only: then rows never end inside a block
// or a payload byte, and block b of the tensor is elements [32 b, 32 b + 32).
inline Plan<MxDesc> plan_mx(const std::vector<QuantIn>& in) {
  Plan<MxDesc> p;
  p.descs.reserve(in.size());
  for (const QuantIn& it : in) {
    if (it.dtype < 0 || it.dtype > 2)
      throw std::runtime_error("unsupported dtype");
    if (it.rows == 0 || it.cols == 0) continue;
    const uint64_t nblk = (it.cols + kMxBlock - 1) / kMxBlock;
    const uint64_t nblocks = it.rows * nblk;
    if (it.cols > UINT32_MAX || nblocks > (1ull << 31))
      throw std::runtime_error("tensor too large for one mx descriptor");
    const uint32_t es = it.dtype == 0 ? 4u : 2u;
    if (it.wide % es) throw std::runtime_error("misaligned tensor");
    const uint32_t fast =
        (((it.wide | it.payload) & 15u) == 0 && it.cols % kMxBlock == 0) ? 1u
                                                                        : 0u;
    p.descs.push_back(MxDesc{it.wide, it.payload, it.scales, it.rows, p.units,
                             (uint32_t)it.cols, (uint32_t)nblk,
                             (uint32_t)nblocks, (uint32_t)it.dtype, fast, 0});
    p.units += (nblocks + kMxUnitBlocks - 1) / kMxUnitBlocks;
  }
  return p;
}

// Row-scaled FP8 quant / dequant plan, from the same tuples (scales: one f32
// per row); tensors with no elements are dropped.  `wave` and `wg` are the
// regime limits (at most kRowWave / kRowWg, what the kernels can hold).  The
// mode and the unit count are fixed here, once per tensor, so a descriptor
// means the same to every lane of a workgroup.
inline Plan<RowDesc> plan_row(const std::vector<QuantIn>& in, bool dequant,
                              uint32_t wave = kRowWave,
                              uint32_t wg = kRowWg) {
  if (wave > kRowWave || wg > kRowWg)
    throw std::runtime_error("row regime limit above the kernels' capacity");
  Plan<RowDesc> p;
  p.descs.reserve(in.size());
  for (const QuantIn& it : in) {
    if (it.dtype < 0 || it.dtype > 2)
      throw std::runtime_error("unsupported dtype");
    if (it.rows == 0 || it.cols == 0) continue;
    if (it.cols > UINT32_MAX)
      throw std::runtime_error("tensor too large for one row descriptor");
    if (it.scales & 3u) throw std::runtime_error("scales must be 4B aligned");
    const uint32_t es = it.dtype == 0 ? 4u : 2u;
    if (it.wide % es) throw std::runtime_error("misaligned tensor");
    const uint32_t fast =
        (((it.wide | it.payload) & 15u) == 0 && (it.cols & 15u) == 0) ? 1u : 0u;
    const uint32_t mode = it.cols <= wave ? kRowModeWave
                          : it.cols <= wg ? kRowModeHeld
                                          : kRowModeStream;
    const uint64_t numel = it.rows * it.cols;
    p.descs.push_back(RowDesc{it.wide, it.payload, it.scales, it.rows, p.units,
                              numel, (uint32_t)it.cols, (uint32_t)it.dtype,
                              mode, fast});
    if (dequant) p.units += (numel + kRowDqUnitElems - 1) / kRowDqUnitElems;
    else if (mode == kRowModeWave)
      p.units += (it.rows + kRowWaveRows - 1) / kRowWaveRows;
    else p.units += it.rows;
  }
  return p;
}

// Tile-scaled FP8 quant / dequant plan (scales: one f32 per 128 x 128 tile of
// each of the `mats` matrices); tensors with no elements are dropped.  The
// kernels take rows and columns in 32 bits, and the dequantise side numbers
// the rows of the whole stack in 32 bits as well.
inline Plan<TileDesc> plan_tile(const std::vector<TileIn>& in, bool dequant) {
  Plan<TileDesc> p;
  p.descs.reserve(in.size());
  for (const TileIn& it : in) {
    if (it.dtype < 0 || it.dtype > 2)
      throw std::runtime_error("unsupported dtype");
    if (it.mats == 0 || it.rows == 0 || it.cols == 0) continue;
    if (it.cols > UINT32_MAX || it.rows > UINT32_MAX ||
        it.mats > UINT32_MAX / it.rows)
      throw std::runtime_error("tensor too large for one tile descriptor");
    if (it.scales & 3u) throw std::runtime_error("scales must be 4B aligned");
    const uint32_t es = it.dtype == 0 ? 4u : 2u;
    if (it.wide % es) throw std::runtime_error("misaligned tensor");
    const uint32_t fast =
        (((it.wide | it.payload) & 15u) == 0 && (it.cols & 15u) == 0) ? 1u : 0u;
    const uint64_t ntr = (it.rows + kTile - 1) / kTile;
    const uint64_t ntc = (it.cols + kTile - 1) / kTile;
    const uint64_t numel = it.mats * it.rows * it.cols;
    p.descs.push_back(TileDesc{it.wide, it.payload, it.scales, p.units, numel,
                               (uint32_t)it.rows, (uint32_t)it.cols,
                               (uint32_t)ntr, (uint32_t)ntc,
                               (uint32_t)it.dtype, fast});
    if (dequant) p.units += (numel + kTileDqUnitElems - 1) / kTileDqUnitElems;
    else p.units += it.mats * ntr * ntc;
  }
  return p;
}

// Per-tensor FP8 quant / dequant plan (scales: one f32 per matrix of the
// `mats` matrices); tensors with no elements are dropped.  A tensor of more
// than kTensorMaxElems = 2^47 elements is refused.  Fast needs both bases 16B
// aligned and whole 16-element chunks per matrix, so no chunk straddles two
// scales; for a single matrix that is numel % 16 == 0.  The quantise side
// needs the amax slots (one zeroed u32 per matrix, apart from `scales`).
inline Plan<TensorDesc> plan_tensor(const std::vector<TensorIn>& in,
                                    bool dequant) {
  Plan<TensorDesc> p;
  p.descs.reserve(in.size());
  for (const TensorIn& it : in) {
    if (it.dtype < 0 || it.dtype > 2)
      throw std::runtime_error("unsupported dtype");
    if (it.mats == 0 || it.rows == 0 || it.cols == 0) continue;
    if (it.rows > kTensorMaxElems / it.cols ||
        it.mats > kTensorMaxElems / (it.rows * it.cols))
      throw std::runtime_error("tensor too large for one tensor descriptor");
    if (it.scales & 3u) throw std::runtime_error("scales must be 4B aligned");
    if (!dequant && (it.amax == 0 || (it.amax & 3u)))
      throw std::runtime_error("amax slots must be given and 4B aligned");
    const uint32_t es = it.dtype == 0 ? 4u : 2u;
    if (it.wide % es) throw std::runtime_error("misaligned tensor");
    const uint64_t mat_elems = it.rows * it.cols;
    const uint64_t numel = it.mats * mat_elems;
    const uint32_t fast =
        (((it.wide | it.payload) & 15u) == 0 && (mat_elems & 15u) == 0) ? 1u
                                                                        : 0u;
    const uint64_t upm = (mat_elems + kTensorUnitElems - 1) / kTensorUnitElems;
    p.descs.push_back(TensorDesc{it.wide, it.payload, it.scales,
                                 dequant ? 0 : it.amax, p.units, numel,
                                 mat_elems, upm, (uint32_t)it.dtype, fast});
    if (dequant)
      p.units += (numel + kTensorDqUnitElems - 1) / kTensorDqUnitElems;
    else p.units += it.mats * upm;
  }
  return p;
}
