// K1/K2 — batched strided slice copy, and the flat streaming copy that a
// launch of nothing but contiguous 16B-aligned ranges takes instead.

#pragma once

#include "common.h"
#include "desc_ring.h"
#include "plan.h"
#include "unit_walk.h"

#include <algorithm>
#include <atomic>

// shared copy loops

// N 16B loads in flight per lane before the first dependent store; lane `i`
// advances by N * STRIDE while a whole round still fits
template <uint32_t N, uint32_t STRIDE, bool NTL, bool NT, typename SrcP,
          typename DstP>
__device__ __forceinline__ void copy16_rounds(SrcP s4, DstP d4, uint32_t n4,
                                              uint32_t& i) {
  for (; i + (N - 1) * STRIDE < n4; i += N * STRIDE) {
    v4u v[N];
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) v[k] = load16<NTL>(s4 + i + k * STRIDE);
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) store16<NT>(d4 + i + k * STRIDE, v[k]);
  }
}

// Streaming copy of n4 16-byte words by STRIDE cooperating lanes, lane index
// `i`.  x8 first: 128 B of loads in flight per lane before the first
// dependent store (HBM latency ~300 cyc wants deep MLP); then x4 and x1 for
// what is left.  NTL / NT: non-temporal loads / stores; NT_TAIL: the x4 and
// x1 stores too.
template <uint32_t STRIDE, bool NTL, bool NT, bool NT_TAIL, typename SrcP,
          typename DstP>
__device__ __forceinline__ void stream_copy16(SrcP s4, DstP d4, uint32_t n4,
                                              uint32_t i) {
  copy16_rounds<8, STRIDE, NTL, NT>(s4, d4, n4, i);
  copy16_rounds<4, STRIDE, NTL, NT_TAIL>(s4, d4, n4, i);
  copy16_rounds<1, STRIDE, NTL, NT_TAIL>(s4, d4, n4, i);
}

// what is not 16B-aligned goes one T per lane and round (one wave)
template <typename T>
__device__ __forceinline__ void copy_words(const char* src, char* dst,
                                           uint32_t len, uint32_t lane) {
  const T* s = reinterpret_cast<const T*>(src);
  T* d = reinterpret_cast<T*>(dst);
  for (uint32_t i = lane; i < len / sizeof(T); i += 64) d[i] = s[i];
}

// 16B word index of a row-packed unit -> (row, word in row)
struct RowShift {  // power-of-two row: shift/mask replaces the per-element
  uint32_t sh;     // udiv pair (~30 cycles each — visible in the
  uint32_t msk;    // LLC-resident regime)
  __device__ __forceinline__ uint32_t row(uint32_t i) const { return i >> sh; }
  __device__ __forceinline__ uint32_t col(uint32_t i) const { return i & msk; }
};
struct RowDiv {
  uint32_t rb4;
  __device__ __forceinline__ uint32_t row(uint32_t i) const { return i / rb4; }
  __device__ __forceinline__ uint32_t col(uint32_t i) const { return i % rb4; }
};

template <uint32_t N, typename Map>
__device__ __forceinline__ void packed_rounds(const char* sbase, char* dbase,
                                              int64_t sstride, int64_t dstride,
                                              uint32_t elems, Map m,
                                              uint32_t& i) {
  for (; i + (N - 1) * 64 < elems; i += N * 64) {
    v4u v[N];
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) {
      const uint32_t j = i + k * 64;
      v[k] = *reinterpret_cast<const v4u*>(
          sbase + (int64_t)m.row(j) * sstride + (m.col(j) << 4));
    }
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) {
      const uint32_t j = i + k * 64;
      *reinterpret_cast<v4u*>(
          dbase + (int64_t)m.row(j) * dstride + (m.col(j) << 4)) = v[k];
    }
  }
}

// general kernel
//
// Work unit = one tile_bytes span of one row (or a pack of small rows);
// blocks chunk the global unit list and find their slice in the prefix array.

__device__ __forceinline__ void row_offsets(const SliceDesc& d, uint64_t row,
                                            int64_t& soff, int64_t& doff) {
  soff = 0;
  doff = 0;
  uint64_t rem = row;
  for (int i = (int)d.ndim - 1; i >= 0; --i) {
    uint64_t idx = rem % d.shape[i];
    rem /= d.shape[i];
    soff += (int64_t)idx * d.src_stride[i];
    doff += (int64_t)idx * d.dst_stride[i];
  }
}

// One WAVE per work unit (a <=16 KiB span of one row): a 256-thread block
// runs 4 independent waves, so rows never serialize behind each other
// inside a block, and the unrolled 16B path keeps its loads in flight
// per lane (64 lanes x 16B x 4 = 4 KiB outstanding per wave).
//
// NT: non-temporal stores in the 16B path — a bulk copy's destination is
// never re-read by this kernel, so dropping the lines from L2 leaves the
// cache to traffic that can reuse it (toggle measured on hardware).
// REMOTE: sources are IPC-mapped PEER memory (one-sided batched reads over
// xGMI, replacing per-piece SDMA enqueues); lines from a previous pull may
// be cached locally, so each workgroup issues one system-scope acquire
// before reading (validated by the cross-process staleness GPU test).
template <bool NT, bool REMOTE>
__global__ void __launch_bounds__(256)
copy_slices_kernel(const SliceDesc* __restrict__ descs, uint32_t nslices,
                   uint64_t total_units, uint32_t tile_bytes) {
  if (REMOTE) {
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    }
    __syncthreads();
  }
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t lane = threadIdx.x & 63u;
  // BLOCK-CHUNKED assignment: each wave owns a CONTIGUOUS unit range, so
  // the slice descriptor is loaded once and advanced linearly — a strided
  // grid walk would re-search and re-load ~176 B of desc per unit, which
  // dominated small-row scatters (measured 249 GB/s in round 1)
  const uint64_t nwaves = (uint64_t)gridDim.x * 4;
  const uint64_t wave_id = (uint64_t)blockIdx.x * 4 + wave;
  const uint64_t chunk = (total_units + nwaves - 1) / nwaves;
  uint64_t unit = wave_id * chunk;
  const uint64_t unit_end =
      unit + chunk < total_units ? unit + chunk : total_units;
  if (unit >= unit_end) return;
  UnitWalk w;
  SliceDesc d;
  walk_seek(w, d, descs, nslices, unit);  // ONCE, for the range start
  for (; unit < unit_end; ++unit) {
    walk_step(w, d, descs, nslices, unit);
    uint64_t local = unit - d.units_prefix;
    if (d.rows_per_unit > 1) {
      // rows_per_unit consecutive rows, ndim<=1, all 16B-aligned
      uint64_t row0 = local * d.rows_per_unit;
      uint32_t nrows = (uint32_t)(d.rows - row0 < d.rows_per_unit
                                      ? d.rows - row0
                                      : d.rows_per_unit);
      int64_t sstride = d.ndim ? d.src_stride[0] : d.row_bytes;
      int64_t dstride = d.ndim ? d.dst_stride[0] : d.row_bytes;
      const char* sbase =
          reinterpret_cast<const char*>(d.src) + (int64_t)row0 * sstride;
      char* dbase = reinterpret_cast<char*>(d.dst) + (int64_t)row0 * dstride;
      const uint32_t rb4 = d.row_bytes >> 4;
      const uint32_t elems = nrows * rb4;
      // a flat vectorized loop over the 16B words of the rows keeps ~4
      // independent 16B accesses in flight per lane
      auto copy_rows = [&](auto map) {
        uint32_t i = lane;
        packed_rounds<4>(sbase, dbase, sstride, dstride, elems, map, i);
        packed_rounds<1>(sbase, dbase, sstride, dstride, elems, map, i);
      };
      if ((rb4 & (rb4 - 1)) == 0) copy_rows(RowShift{31u - __clz(rb4), rb4 - 1});
      else copy_rows(RowDiv{rb4});
      continue;
    }
    uint64_t row = local / d.tiles_per_row;
    uint32_t tile = (uint32_t)(local % d.tiles_per_row);
    int64_t soff, doff;
    row_offsets(d, row, soff, doff);
    uint32_t start = tile * tile_bytes;
    uint32_t len = min(tile_bytes, d.row_bytes - start);
    const char* src = reinterpret_cast<const char*>(d.src) + soff + start;
    char* dst = reinterpret_cast<char*>(d.dst) + doff + start;
    uintptr_t sa = reinterpret_cast<uintptr_t>(src);
    uintptr_t da = reinterpret_cast<uintptr_t>(dst);
    if (((sa | da | len) & 15u) == 0) {
      // one wave per unit: lane stride 64; the x4/x1 tail stores stay plain
      stream_copy16<64, false, NT, false>(reinterpret_cast<const v4u*>(src),
                                          reinterpret_cast<v4u*>(dst),
                                          len >> 4, lane);
    } else if (((sa | da | len) & 3u) == 0) {
      copy_words<uint32_t>(src, dst, len, lane);
    } else if (((sa | da | len) & 1u) == 0) {
      copy_words<uint16_t>(src, dst, len, lane);
    } else {
      copy_words<uint8_t>(src, dst, len, lane);
    }
  }
}

// flat streaming copy — every slice of the launch is one contiguous,
// 16B-aligned byte range (the 1-GPU state_dict put and get are entirely this)
//
// Unit = one `span`-byte piece of one copy.  The WHOLE 256-thread block
// works on one unit (each load/store instruction of the block covers 4 KiB
// contiguous) and blocks take units interleaved (blockIdx.x + k*gridDim.x),
// so the resident grid sweeps one compact, advancing window of the buffers
// instead of one private stream per wave.  The descriptor lookup depends on
// blockIdx only, i.e. it is uniform over the block.

// defaults from the span x grid x NT sweep (profiles/flat_copy_ab.log):
// 16 KiB units won every pattern; the Llama-shaped 2 GB sub-batch kept
// gaining up to a 65536-block cap (~2 units per block; 5.94 TB/s vs 5.61 at
// the 2048 that usually suits memory-bound kernels); non-temporal LOADS add
// 3-4% on top of non-temporal stores (HIPSTORE_FLAT_NTLOAD=0 turns them off)
static constexpr uint32_t kFlatSpanDefault = 16384u;
static constexpr uint32_t kFlatGridDefault = 65536u;

template <bool NT, bool NTL>
__global__ void __launch_bounds__(256)
copy_flat_kernel(const FlatDesc* __restrict__ descs, uint32_t ndescs,
                 uint64_t total_units, uint32_t span) {
  UnitWalk w;
  FlatDesc d = {};
  for (uint64_t unit = blockIdx.x; unit < total_units; unit += gridDim.x) {
    // left the current copy?  Big copies span many strides of the grid, so
    // most units skip this and start their loads without a dependent
    // descriptor read in front
    if (unit >= w.next_prefix) walk_seek(w, d, descs, ndescs, unit);
    const uint64_t off = (unit - d.units_prefix) * span;
    const uint64_t rem = d.nbytes - off;
    const uint32_t n4 = (uint32_t)(rem < span ? rem : span) >> 4;
    stream_copy16<256, NTL, NT, NT>(
        reinterpret_cast<const gv4u*>(d.src + off),
        reinterpret_cast<gv4u*>(d.dst + off), n4, threadIdx.x);
  }
}

// launchers

// tile size per launch (general kernel).  Defaults from the hardware tile x
// grid sweep (profiles/kernel_tune.log): 32 KiB tiles + an 8192-block grid
// cap won the flat bulk pattern (+5% over 128 KiB/2048); small batches keep
// 16 KiB tiles so enough waves stay busy
static uint32_t pick_tile(uint64_t total_bytes) {
  return env_u32("HIPSTORE_TILE", 4096, UINT32_MAX,
                 total_bytes > (512ull << 20) ? 32768u : 16384u);
}

// unit span of the flat kernel: a multiple of 4 KiB, so that every unit
// start keeps the 16B alignment and whole-block rows
static uint32_t pick_flat_span() {
  uint32_t v = env_u32("HIPSTORE_FLAT_SPAN", 4096, 1u << 24, kFlatSpanDefault);
  return (v & 4095u) == 0 ? v : kFlatSpanDefault;
}

// launches that went to the flat kernel (tests tell the two paths apart)
static std::atomic<uint64_t> g_flat_launches{0};

// One launch for a batch of slices: the flat kernel when every slice
// qualifies (never for IPC-mapped `remote` sources, which need the general
// kernel's acquire; never with HIPSTORE_FLAT=0), else the general kernel.
static void launch_copy(const std::vector<SliceIn>& in, int device,
                        hipStream_t stream, bool remote) {
  // NT stores default ON: +5% on 1 GiB flat copies, +26% on the reshard
  // scatter (profiles/gpu_primitive_microbench.log, NT1 vs NT0 runs)
  const bool nt = env_flag("HIPSTORE_NT", true);
  Plan<FlatDesc> flat;
  const uint32_t span = pick_flat_span();
  if (!remote && env_flag("HIPSTORE_FLAT", true) && plan_flat(in, span, flat)) {
    if (flat.units == 0) return;  // nothing but empty copies
    const bool ntl = env_flag("HIPSTORE_FLAT_NTLOAD", true);
    stage_descs_and_launch(device, stream, flat.descs, [&](const FlatDesc* d) {
      // one block per unit, interleaved; memory-bound, so cap the grid
      uint32_t grid = (uint32_t)std::min<uint64_t>(
          flat.units, env_u32("HIPSTORE_GRID", 64, UINT32_MAX, kFlatGridDefault));
      auto kern = nt ? (ntl ? copy_flat_kernel<true, true>
                            : copy_flat_kernel<true, false>)
                     : (ntl ? copy_flat_kernel<false, true>
                            : copy_flat_kernel<false, false>);
      hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, stream, d,
                         (uint32_t)flat.descs.size(), flat.units, span);
      g_flat_launches.fetch_add(1, std::memory_order_relaxed);
    });
    return;
  }
  const uint32_t tile = pick_tile(total_bytes(in));
  const Plan<SliceDesc> p = plan_slices(in, tile);
  if (p.units == 0) return;
  stage_descs_and_launch(device, stream, p.descs, [&](const SliceDesc* d) {
    // memory-bound: cap the grid and chunk units over it (guide G11);
    // each block consumes 4 contiguous unit ranges (one per wave)
    uint32_t grid = (uint32_t)std::min<uint64_t>(
        (p.units + 3) / 4, env_u32("HIPSTORE_GRID", 64, UINT32_MAX, 8192u));
    auto kern = nt ? (remote ? copy_slices_kernel<true, true>
                             : copy_slices_kernel<true, false>)
                   : (remote ? copy_slices_kernel<false, true>
                             : copy_slices_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, stream, d,
                       (uint32_t)p.descs.size(), p.units, tile);
  });
}
