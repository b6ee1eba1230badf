// Per-device stream pool and the descriptor staging ring that every batched
// kernel launch uploads its descriptors through.

#pragma once

#include "common.h"

#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

// dedicated streams per device for bulk copies
static constexpr int kStreamsPerDevice = 8;

// descriptor ring depth = the state_dict pipeline depth (8 concurrent
// sub-batch RPCs): a launch waits only for the kernel that last used ITS
// slot, so up to 8 launches queue on a stream behind a running kernel
static constexpr int kDescSlots = 8;

// one descriptor staging slot: pinned host buffer + device copy of it
struct DescSlot {
  std::mutex mu;  // held while the slot is waited on, filled and enqueued
  void* h_desc = nullptr;
  void* d_desc = nullptr;
  size_t cap = 0;
  // guards buffer reuse: recorded after the kernel that reads d_desc
  hipEvent_t evt = nullptr;
};

struct DevicePool {
  std::vector<hipStream_t> streams;
  DescSlot slots[kDescSlots];
  uint64_t next_slot = 0;  // under g_mutex
};

static std::mutex g_mutex;
// node-based map: DevicePool (mutexes inside) is never moved once built
static std::unordered_map<int, DevicePool> g_pools;

static DevicePool& pool_for(int device) {
  std::lock_guard<std::mutex> lock(g_mutex);
  auto it = g_pools.find(device);
  if (it != g_pools.end()) return it->second;
  HIP_CHECK(hipSetDevice(device));
  std::vector<hipStream_t> streams(kStreamsPerDevice);
  for (int i = 0; i < kStreamsPerDevice; ++i) {
    HIP_CHECK(hipStreamCreateWithFlags(&streams[i], hipStreamNonBlocking));
  }
  DevicePool& p = g_pools[device];
  p.streams = std::move(streams);
  return p;
}

// caller holds s.mu and has already waited on s.evt, so no kernel still
// reads the buffers that are freed here
static void ensure_desc_capacity(DescSlot& s, int device, size_t bytes) {
  if (s.cap >= bytes) return;
  size_t cap = bytes * 2 + 4096;
  HIP_CHECK(hipSetDevice(device));
  if (s.h_desc) HIP_CHECK(hipHostFree(s.h_desc));
  if (s.d_desc) HIP_CHECK(hipFree(s.d_desc));
  s.h_desc = s.d_desc = nullptr;
  s.cap = 0;
  HIP_CHECK(hipHostMalloc(&s.h_desc, cap, hipHostMallocDefault));
  HIP_CHECK(hipMalloc(&s.d_desc, cap));
  s.cap = cap;
}

// Copy the descriptors to the device through the next ring slot and run
// `launch(d_desc)`, which enqueues on `stream` the one kernel that reads
// them.  The slot's event is recorded behind that kernel, so the slot is
// reused only once the kernel is done.
template <typename Desc, typename Launch>
static void stage_descs_and_launch(int device, hipStream_t stream,
                                   const std::vector<Desc>& descs,
                                   Launch&& launch) {
  const size_t bytes = descs.size() * sizeof(Desc);
  DevicePool& p = pool_for(device);
  HIP_CHECK(hipSetDevice(device));
  DescSlot* slot;
  {
    std::lock_guard<std::mutex> lock(g_mutex);
    slot = &p.slots[p.next_slot++ % kDescSlots];
  }
  std::lock_guard<std::mutex> slot_lock(slot->mu);
  if (slot->evt == nullptr) {
    HIP_CHECK(hipEventCreateWithFlags(&slot->evt, hipEventDisableTiming));
  } else {
    // only the KERNEL that last read this slot must be done before its
    // buffers are reused or regrown; other slots' kernels keep running
    HIP_CHECK(hipEventSynchronize(slot->evt));
  }
  ensure_desc_capacity(*slot, device, bytes);
  std::memcpy(slot->h_desc, descs.data(), bytes);
  HIP_CHECK(hipMemcpyAsync(slot->d_desc, slot->h_desc, bytes,
                           hipMemcpyHostToDevice, stream));
  launch(static_cast<const Desc*>(slot->d_desc));
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipEventRecord(slot->evt, stream));
}
