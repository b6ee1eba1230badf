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

// K6/K7: unit = kMxUnitBlocks consecutive 32-element blocks of a tensor
struct MxDesc {
  uintptr_t wide;         // f32/bf16/f16 tensor: quant source, dequant dest
  uintptr_t payload;      // packed e2m1, rows of ceil(cols / 2) bytes
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
