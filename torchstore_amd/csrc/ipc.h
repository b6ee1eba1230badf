// HIP IPC: export / open / close of hipIpcMemHandle_t at caching-allocator
// block granularity.

#pragma once

#include "common.h"

#include <pybind11/pybind11.h>

#include <cstring>
#include <mutex>
#include <unordered_map>

namespace py = pybind11;

// Export handles are cached per allocator block (hipIpcGetMemHandle does a
// dmabuf export ioctl — tens of ms — while hipMemGetAddressRange is cheap).
// Same design as the reference's (data_ptr, nbytes)-keyed RdmaMemory cache
// (torchstore torchcomms/cache.py:150-187).  A cached handle goes stale
// only when its block is returned to the OS (torch.cuda.empty_cache /
// OOM-retry release) and the same base address is re-allocated; callers
// therefore pass an allocator GENERATION (the caching allocator's
// segment-freed counter): a changed generation flushes that device's
// cache before lookup — no manual clear call needed for correctness.
struct ExportCache {
  long long gen = -(1ll << 62);
  std::unordered_map<uintptr_t, std::string> map;
};
static std::mutex g_export_mutex;
static std::unordered_map<int, ExportCache> g_export_caches;

// Returns (handle_bytes, offset_in_block, block_size).  Callers MUST route
// blocks >= 2 GiB through the chunked-staging path: hipIpcOpenMemHandle of
// a >=2^31-byte dmabuf hangs on this platform (measured; the export itself
// succeeds, the peer's import never returns).
static py::tuple ipc_export(uintptr_t ptr, int device, long long generation) {
  HIP_CHECK(hipSetDevice(device));
  void* base = nullptr;
  size_t size = 0;
  HIP_CHECK(hipMemGetAddressRange(&base, &size, reinterpret_cast<void*>(ptr)));
  uintptr_t base_u = reinterpret_cast<uintptr_t>(base);
  std::string handle_str;
  if (generation >= 0) {  // negative generation = caller opts out of caching
    std::lock_guard<std::mutex> lock(g_export_mutex);
    ExportCache& c = g_export_caches[device];
    if (generation != c.gen) {
      c.map.clear();
      c.gen = generation;
    }
    auto it = c.map.find(base_u);
    if (it != c.map.end()) {
      handle_str = it->second;
    }
  }
  if (handle_str.empty()) {
    hipIpcMemHandle_t handle;
    HIP_CHECK(hipIpcGetMemHandle(&handle, base));
    handle_str.assign(reinterpret_cast<const char*>(&handle), sizeof(handle));
    if (generation >= 0) {
      std::lock_guard<std::mutex> lock(g_export_mutex);
      g_export_caches[device].map.emplace(base_u, handle_str);
    }
  }
  return py::make_tuple(py::bytes(handle_str),
                        static_cast<uint64_t>(ptr - base_u),
                        static_cast<uint64_t>(size));
}

static void ipc_export_cache_clear() {
  std::lock_guard<std::mutex> lock(g_export_mutex);
  g_export_caches.clear();
}

static uintptr_t ipc_open(py::bytes handle_bytes, int local_device,
                          int src_device) {
  std::string raw = handle_bytes;
  if (raw.size() != sizeof(hipIpcMemHandle_t)) {
    throw std::runtime_error("bad ipc handle size");
  }
  hipIpcMemHandle_t handle;
  std::memcpy(&handle, raw.data(), sizeof(handle));
  HIP_CHECK(hipSetDevice(local_device));
  void* ptr = nullptr;
  HIP_CHECK(hipIpcOpenMemHandle(&ptr, handle, hipIpcMemLazyEnablePeerAccess));
  (void)src_device;
  return reinterpret_cast<uintptr_t>(ptr);
}

static void ipc_close(uintptr_t base, int local_device) {
  HIP_CHECK(hipSetDevice(local_device));
  HIP_CHECK(hipIpcCloseMemHandle(reinterpret_cast<void*>(base)));
}
