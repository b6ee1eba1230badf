// _hipstore — native core of torchstore_amd for MI355X (gfx950, CDNA4).
//
// One translation unit; every header under csrc/ includes what it uses.
// Provides (python surface wrapped by torchstore_amd/ops/gpu.py):
//   * HIP IPC (ipc.h):  ipc_export / ipc_open / ipc_close — hipIpcMemHandle_t
//     at caching-allocator block granularity (base via hipMemGetAddressRange,
//     descriptor carries the byte offset), replacing the reference's
//     ibverbs RDMA registration (torchstore transport/monarch_rdma.py).
//   * copy_batch — batched one-sided bulk copies (hipMemcpyPeerAsync /
//     DtoD) striped round-robin over a per-device pool of dedicated HIP
//     streams (desc_ring.h) so concurrent transfers to different peers
//     aggregate xGMI links (7 x ~153 GB/s per GPU); synchronizes the streams
//     it used.
//   * copy_slices (copy_kernels.h) — K1/K2: one kernel launch copying N
//     strided slices (gather: strided->contiguous, scatter:
//     contiguous->strided, or strided->strided), replacing per-slice torch
//     copies in reshard pack/unpack (reference hot loops:
//     storage_volume.py:220-277, utils.py:199-212, direct_weight_sync.py:350).
//     A launch whose slices are all contiguous 16B-aligned ranges (every
//     launch of the 1-GPU state_dict put/get) takes copy_flat_kernel, a
//     block-per-unit streaming copy, instead of the general kernel.
//   * cast_copy (cast_kernel.h) — K3: fused dtype cast + pack
//     (f32<->bf16/f16), one HBM read + one write, vectorized 16B/lane
//     (reference: state_dict_utils.py:177-189 casts every floating param per
//     sync).
//   * quant_fp8_batch / dequant_fp8_batch (quant_fp8.h) — K4/K5: block-scaled
//     FP8 (OCP e4m3, 128-element blocks, f32 scales) over N tensors in one
//     launch each way, bit-exact against the torch recipe.
//   * quant_mx_batch / dequant_mx_batch (quant_mx.h) — K6/K7: MXFP4 (packed
//     OCP e2m1, 32-element blocks, e8m0 scale bytes) the same way, with a
//     launch counter of their own.
//   * host_register / host_unregister — pin SHM pages for DMA.
// Underneath: plan.h turns the python tuples into descriptors (HIP-free; also
// built on the CPU by tests/native/plan_check.cpp), desc_ring.h stages them
// on the device, unit_walk.h finds a unit's descriptor inside the kernels,
// and common.h holds HIP_CHECK, the list and reader of the HIPSTORE_* knobs,
// the dtype conversions and the 16-byte vector types.
//
// Deliberately torch-ABI-free: tensors cross as raw device pointers +
// geometry, so the module builds with plain hipcc + pybind11 and never
// drifts against libtorch.

#include "cast_kernel.h"
#include "common.h"
#include "copy_kernels.h"
#include "desc_ring.h"
#include "ipc.h"
#include "plan.h"
#include "quant_fp8.h"
#include "quant_mx.h"

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <tuple>
#include <unordered_map>
#include <vector>

namespace py = pybind11;

// batched bulk copies over xGMI / HBM; copies: (dst_ptr, dst_dev, src_ptr, src_dev, nbytes)
//
// Same-device copies batch into ONE kernel launch per device (291 sequential
// hipMemcpyAsync enqueues cost ~20 us each on the host — the kernel path
// replaces them with one dispatch).  Cross-device copies and copies of 4 GiB
// or more keep hipMemcpyAsync striped round-robin over the stream pool so
// transfers to different peers ride different xGMI links concurrently.
static void copy_batch(
    const std::vector<std::tuple<uintptr_t, int, uintptr_t, int, uint64_t>>&
        copies) {
  if (copies.empty()) return;
  std::unordered_map<int, std::vector<SliceIn>> per_device;
  std::vector<hipStream_t> used;
  int i = 0;
  for (const auto& c : copies) {
    const auto& [dst, dst_dev, src, src_dev, n] = c;
    if (n == 0) continue;
    if (dst_dev == src_dev && n <= UINT32_MAX) {
      per_device[dst_dev].push_back(
          SliceIn{src, dst, n, nullptr, nullptr, nullptr, 0});
      continue;
    }
    DevicePool& p = pool_for(dst_dev);
    hipStream_t s = p.streams[i++ % kStreamsPerDevice];
    HIP_CHECK(hipSetDevice(dst_dev));
    // UVA-resolved copy: the canonical form for IPC-mapped peer pointers
    // (hipMemcpyPeerAsync requires context-owned pointers on both ends;
    // Default kind lets the driver resolve mapped peer memory)
    HIP_CHECK(hipMemcpyAsync(reinterpret_cast<void*>(dst),
                             reinterpret_cast<void*>(src), n,
                             hipMemcpyDefault, s));
    used.push_back(s);
  }
  for (auto& kv : per_device) {
    hipStream_t s = pool_for(kv.first).streams[0];
    launch_copy(kv.second, kv.first, s, /*remote=*/false);
    used.push_back(s);
  }
  for (hipStream_t s : used) HIP_CHECK(hipStreamSynchronize(s));
}

// copies: (dst_ptr, dst_dev, dpitch, src_ptr, src_dev, spitch, width, height)
// — strided (pitched) one-sided reads/writes: moves ONLY the overlap bytes
// of a reshard instead of whole remote shards (the reference always reads
// the full source shard, direct_weight_sync.py:280-314).
static void copy_batch_2d(
    const std::vector<std::tuple<uintptr_t, int, uint64_t, uintptr_t, int,
                                 uint64_t, uint64_t, uint64_t>>& copies) {
  if (copies.empty()) return;
  std::vector<hipStream_t> used;
  int i = 0;
  for (const auto& c : copies) {
    const auto& [dst, dst_dev, dpitch, src, src_dev, spitch, width, height] = c;
    (void)src_dev;
    DevicePool& p = pool_for(dst_dev);
    hipStream_t s = p.streams[i++ % kStreamsPerDevice];
    HIP_CHECK(hipSetDevice(dst_dev));
    HIP_CHECK(hipMemcpy2DAsync(reinterpret_cast<void*>(dst), dpitch,
                               reinterpret_cast<void*>(src), spitch, width,
                               height, hipMemcpyDefault, s));
    used.push_back(s);
  }
  for (hipStream_t s : used) HIP_CHECK(hipStreamSynchronize(s));
}

// K1/K2; python passes per slice:
//   (src_ptr, dst_ptr, row_bytes, [outer shape], [src strides B], [dst strides B])
using PySlice = std::tuple<uintptr_t, uintptr_t, uint64_t,
                           std::vector<uint64_t>, std::vector<int64_t>,
                           std::vector<int64_t>>;

static void copy_slices(const std::vector<PySlice>& slices, int device,
                        uintptr_t stream_handle, bool blocking,
                        bool remote) {
  if (slices.empty()) return;
  std::vector<SliceIn> in;
  in.reserve(slices.size());
  for (const auto& s : slices) {
    const auto& [src, dst, row_bytes, shape, sst, dstst] = s;
    if (sst.size() != shape.size() || dstst.size() != shape.size())
      throw std::runtime_error("one stride per outer dim expected");
    in.push_back(SliceIn{src, dst, row_bytes, shape.data(), sst.data(),
                         dstst.data(), (uint32_t)shape.size()});
  }
  hipStream_t stream = reinterpret_cast<hipStream_t>(stream_handle);
  launch_copy(in, device, stream, remote);
  if (blocking) HIP_CHECK(hipStreamSynchronize(stream));
}

// K3
static void cast_copy(uintptr_t src, int src_dtype, uintptr_t dst,
                      int dst_dtype, uint64_t numel, int device,
                      uintptr_t stream_handle) {
  HIP_CHECK(hipSetDevice(device));
  launch_cast(static_cast<DType>(src_dtype), static_cast<DType>(dst_dtype),
              src, dst, numel, reinterpret_cast<hipStream_t>(stream_handle));
}

// K4/K5; python passes per tensor:
//   (wide_ptr, payload_ptr, scales_ptr, rows, cols, wide_dtype)
using PyQuantItem =
    std::tuple<uintptr_t, uintptr_t, uintptr_t, uint64_t, uint64_t, int>;

template <bool DEQUANT>
static void quant_fp8_batch(const std::vector<PyQuantItem>& items, int device,
                            uintptr_t stream_handle) {
  std::vector<QuantIn> in;
  in.reserve(items.size());
  for (const auto& it : items) {
    const auto& [wide, payload, scales, rows, cols, dtype] = it;
    in.push_back(QuantIn{wide, payload, scales, rows, cols, dtype});
  }
  launch_quant_fp8<DEQUANT>(plan_quant(in), device,
                            reinterpret_cast<hipStream_t>(stream_handle));
}

// K6/K7; the same tuples, scales being e8m0 bytes
template <bool DEQUANT>
static void quant_mx_batch(const std::vector<PyQuantItem>& items, int device,
                           uintptr_t stream_handle) {
  std::vector<QuantIn> in;
  in.reserve(items.size());
  for (const auto& it : items) {
    const auto& [wide, payload, scales, rows, cols, dtype] = it;
    in.push_back(QuantIn{wide, payload, scales, rows, cols, dtype});
  }
  launch_quant_mx<DEQUANT>(plan_mx(in), device,
                           reinterpret_cast<hipStream_t>(stream_handle));
}

// host pinning and staging

// single UVA-resolved copy on a dedicated pool stream (blocking).  Used by
// the SHM transport for D2H staging: torch's copy_ into externally
// registered host memory runs ~2x slower than a direct hipMemcpyAsync.
static void sdma_copy(uintptr_t dst, uintptr_t src, uint64_t nbytes,
                      int device) {
  DevicePool& p = pool_for(device);
  HIP_CHECK(hipSetDevice(device));
  hipStream_t s = p.streams[1];
  HIP_CHECK(hipMemcpyAsync(reinterpret_cast<void*>(dst),
                           reinterpret_cast<void*>(src), nbytes,
                           hipMemcpyDefault, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

static void host_register(uintptr_t ptr, uint64_t nbytes) {
  HIP_CHECK(hipHostRegister(reinterpret_cast<void*>(ptr), nbytes,
                            hipHostRegisterPortable));
}

static void host_unregister(uintptr_t ptr) {
  HIP_CHECK(hipHostUnregister(reinterpret_cast<void*>(ptr)));
}

static int device_count() {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  return e == hipSuccess ? n : 0;
}

static void sync_device(int device) {
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipDeviceSynchronize());
}

PYBIND11_MODULE(_hipstore, m) {
  m.doc() = "torchstore_amd native core (HIP/CDNA4, gfx950)";
  m.def("ipc_export", &ipc_export, py::arg("ptr"), py::arg("device"),
        py::arg("generation"));
  m.def("ipc_export_cache_clear", &ipc_export_cache_clear);
  m.def("ipc_open", &ipc_open, py::arg("handle"), py::arg("local_device"),
        py::arg("src_device"));
  m.def("ipc_close", &ipc_close, py::arg("base"), py::arg("local_device"));
  m.def("copy_batch", &copy_batch, py::arg("copies"),
        py::call_guard<py::gil_scoped_release>());
  m.def("copy_batch_2d", &copy_batch_2d, py::arg("copies"),
        py::call_guard<py::gil_scoped_release>());
  m.def("copy_slices", &copy_slices, py::arg("slices"), py::arg("device"),
        py::arg("stream"), py::arg("blocking") = true,
        py::arg("remote") = false,
        py::call_guard<py::gil_scoped_release>());
  m.def("cast_copy", &cast_copy, py::arg("src"), py::arg("src_dtype"),
        py::arg("dst"), py::arg("dst_dtype"), py::arg("numel"),
        py::arg("device"), py::arg("stream"));
  // one launch over N tensors each, async on the caller's stream; items are
  // (wide_ptr, payload_ptr, scales_ptr, rows, cols, wide_dtype)
  m.def("quant_fp8_batch", &quant_fp8_batch<false>, py::arg("items"),
        py::arg("device"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
  m.def("dequant_fp8_batch", &quant_fp8_batch<true>, py::arg("items"),
        py::arg("device"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
  m.def("quant_launches", []() {
    return g_quant_launches.load(std::memory_order_relaxed);
  });
  m.attr("QUANT_BLOCK") = kQuantBlock;
  m.def("quant_mx_batch", &quant_mx_batch<false>, py::arg("items"),
        py::arg("device"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
  m.def("dequant_mx_batch", &quant_mx_batch<true>, py::arg("items"),
        py::arg("device"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
  m.def("mx_launches", []() {
    return g_mx_launches.load(std::memory_order_relaxed);
  });
  m.attr("MX_BLOCK") = kMxBlock;
  m.attr("MX_LANES") = kMxLanes;
  m.def("sdma_copy", &sdma_copy, py::arg("dst"), py::arg("src"),
        py::arg("nbytes"), py::arg("device"),
        py::call_guard<py::gil_scoped_release>());
  m.def("host_register", &host_register);
  m.def("host_unregister", &host_unregister);
  m.def("device_count", &device_count);
  // flat-kernel defaults and launch counter, for the tests and A/B runs
  m.attr("FLAT_SPAN_DEFAULT") = kFlatSpanDefault;
  m.attr("DESC_RING_SLOTS") = kDescSlots;
  m.def("flat_launches", []() {
    return g_flat_launches.load(std::memory_order_relaxed);
  });
  m.def("sync_device", &sync_device);
}
