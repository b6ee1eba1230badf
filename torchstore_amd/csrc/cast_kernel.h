// K3 — fused cast + pack (f32 <-> bf16/f16): one HBM read + one write.

#pragma once

#include "common.h"

#include <algorithm>

// V elements per thread per iteration; 16B loads when SrcT is 2 bytes,
// 32B (2x float4) when 4 bytes at V=8 — always >= the 16B/lane coalescing
// sweet spot on the wider side (guide G13).  HIPSTORE_CAST_V sweeps V.
template <typename SrcT, typename DstT, uint32_t V>
__global__ void __launch_bounds__(256)
cast_copy_kernel(const SrcT* __restrict__ src, DstT* __restrict__ dst,
                 uint64_t numel) {
  uint64_t base = (uint64_t)(blockIdx.x * blockDim.x + threadIdx.x) * V;
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x * V;
  struct alignas(16) SrcVec { SrcT v[V]; };
  struct alignas(16) DstVec { DstT v[V]; };
  for (uint64_t i = base; i + V <= numel; i += stride) {
    SrcVec s = *reinterpret_cast<const SrcVec*>(src + i);
    DstVec d;
#pragma unroll
    for (uint32_t k = 0; k < V; ++k) d.v[k] = convert<SrcT, DstT>(s.v[k]);
    *reinterpret_cast<DstVec*>(dst + i) = d;
  }
  // tail
  uint64_t tail_start = (numel / V) * V;
  uint64_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  if (tid < numel - tail_start) {
    uint64_t i = tail_start + tid;
    dst[i] = convert<SrcT, DstT>(src[i]);
  }
}

template <typename SrcT, typename DstT>
static void launch_cast(uintptr_t src, uintptr_t dst, uint64_t numel,
                        hipStream_t stream) {
  const uint32_t v = env_u32("HIPSTORE_CAST_V", 1, UINT32_MAX, 8);
  // the cast kernel prefers a SMALLER grid than the copies (1024 beat 2048
  // by ~8% in the sweep — fewer blocks, longer per-block streams)
  const uint32_t cap = env_u32("HIPSTORE_CAST_GRID", 64, UINT32_MAX, 1024);
  uint64_t work = (numel + v - 1) / v;
  uint32_t grid = (uint32_t)std::min<uint64_t>((work + 255) / 256, cap);
  if (grid == 0) grid = 1;
  auto kern = v >= 16 ? cast_copy_kernel<SrcT, DstT, 16>
                      : cast_copy_kernel<SrcT, DstT, 8>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, stream,
                     reinterpret_cast<const SrcT*>(src),
                     reinterpret_cast<DstT*>(dst), numel);
  HIP_CHECK(hipGetLastError());
}

static void launch_cast(DType s, DType d, uintptr_t src, uintptr_t dst,
                        uint64_t numel, hipStream_t stream) {
  if (s == DType::F32 && d == DType::BF16)
    launch_cast<float, __hip_bfloat16>(src, dst, numel, stream);
  else if (s == DType::BF16 && d == DType::F32)
    launch_cast<__hip_bfloat16, float>(src, dst, numel, stream);
  else if (s == DType::F32 && d == DType::F16)
    launch_cast<float, __half>(src, dst, numel, stream);
  else if (s == DType::F16 && d == DType::F32)
    launch_cast<__half, float>(src, dst, numel, stream);
  else if (s == DType::BF16 && d == DType::F16)
    launch_cast<__hip_bfloat16, __half>(src, dst, numel, stream);
  else if (s == DType::F16 && d == DType::BF16)
    launch_cast<__half, __hip_bfloat16>(src, dst, numel, stream);
  else
    throw std::runtime_error("unsupported cast pair");
}
