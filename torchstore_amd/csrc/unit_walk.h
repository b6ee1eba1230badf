// Device side of every batched kernel: find the descriptor that owns a work
// unit.  Descriptors carry `units_prefix`, the exclusive prefix sum of their
// unit counts; a kernel visits units in growing order, so the position only
// ever moves forward: one binary search, then cheap forward steps.

#pragma once

#include "common.h"

struct UnitWalk {
  uint32_t lo = 0;           // index of the current descriptor
  uint64_t next_prefix = 0;  // first unit past it; 0 forces the first seek
};

// the index is searched and stepped as a local and stored once: updated in
// place as a member it stays live twice in the flat and quant kernels
template <typename Desc>
__device__ __forceinline__ void walk_load(UnitWalk& w, Desc& d,
                                          const Desc* __restrict__ descs,
                                          uint32_t ndescs, uint32_t lo) {
  d = descs[lo];
  w.next_prefix = (lo + 1 < ndescs) ? descs[lo + 1].units_prefix : ~0ull;
  w.lo = lo;
}

// binary search at or after the current position: greatest s with
// prefix <= unit
template <typename Desc>
__device__ __forceinline__ void walk_seek(UnitWalk& w, Desc& d,
                                          const Desc* __restrict__ descs,
                                          uint32_t ndescs, uint64_t unit) {
  uint32_t lo = w.lo, hi = ndescs - 1;
  while (lo < hi) {
    uint32_t mid = (lo + hi + 1) >> 1;
    if (descs[mid].units_prefix <= unit) lo = mid; else hi = mid - 1;
  }
  walk_load(w, d, descs, ndescs, lo);
}

// unit + 1 after unit: at most a few descriptors further, walk linearly
template <typename Desc>
__device__ __forceinline__ void walk_step(UnitWalk& w, Desc& d,
                                          const Desc* __restrict__ descs,
                                          uint32_t ndescs, uint64_t unit) {
  uint32_t lo = w.lo;
  while (unit >= w.next_prefix) walk_load(w, d, descs, ndescs, ++lo);
}
