"""Per-tensor FP8 (OCP e4m3) quantisation for transfer and storage (K14/K15).

Format, per tensor: view it as a stack of matrices ``[*lead, R, C]`` (a 1-D
tensor of ``n`` elements is the matrix ``[1, n]``, the convention of
``ops/quant_tile.py``).  Every matrix has ONE scale.  The payload is
``torch.float8_e4m3fn`` of the source's shape, the scales are
``torch.float32`` of shape ``[*lead, 1, 1]`` (``[1, 1]`` for 1-D and 2-D
tensors): ``tile_scales_shape`` with the tile being the whole matrix.  This is
what most FP8 inference checkpoints hold, e4m3 weights with one
``weight_scale`` per weight (``strategy="tensor"``, the tensor-wise operand of
``torch._scaled_mm``), and fused MoE stacks ``[E, R, C]`` with one scale per
expert; the stored scale is the dequantisation multiplier, so a generator
that runs such weights can install the bytes it pulls.  All arithmetic is
fp32::

    amax  = max(max|x| over the matrix, 2**-96)
    scale = amax / 448                      (stored)
    q     = rne_to_e4m3(clamp(x * (448 / amax), -448, 448))
    y     = to_dst_dtype_rne(float(q) * scale)

This is the recipe of ``ops/quant.py`` with the matrix as the block, and what
that module says about exactness, non-finite input (outside the contract),
the NaN codes and overflow holds here unchanged; the round-trip bound is ``16
* scale + |x| * 2**-8``.  ``max`` is exact and associative on finite values,
so the HIP kernels (``csrc/quant_tensor.h``: the quantise is two launches per
call over all CUDA tensors of a device, the amax travelling through memory
between them, the dequantise one) and the pure-torch implementation below
(the path for CPU tensors) produce the same bytes.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import torch

from torchstore_amd.ops.quant import (
    AMAX_FLOOR,
    FP8_DTYPE,
    FP8_MAX,
    _check_wide,
    _launch,
    _numel,
    carve_slabs,
)


@dataclass
class TensorQuantizedTensor:
    """A per-tensor FP8 tensor: what ``get_state_dict(dequantize=False)``
    returns per entry pushed with ``transfer_quant="fp8_e4m3_tensor"``, and a
    valid in-place destination for one."""

    payload: torch.Tensor  # float8_e4m3fn, the original shape
    scales: torch.Tensor  # float32, [*lead, 1, 1]
    orig_dtype: torch.dtype

    @property
    def shape(self) -> torch.Size:
        return self.payload.shape

    def dequantize(self, dtype: torch.dtype = None) -> torch.Tensor:
        out = torch.empty(
            self.payload.shape,
            dtype=dtype or self.orig_dtype,
            device=self.payload.device,
        )
        dequantize_fp8_tensor_into([(self.payload, self.scales)], [out])
        return out


def tensor_scales_shape(shape: Sequence[int]) -> Tuple[int, ...]:
    shape = tuple(shape)
    if not shape:
        raise ValueError("tensor quantisation needs at least one dimension")
    return shape[:-2] + (1, 1)


def alloc_tensor_quantized(
    shapes: Sequence[Sequence[int]], device: torch.device
) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """Uninitialised ``(payload, scales)`` buffers for tensors of ``shapes``
    on ``device``, every buffer contiguous and at least 16 B aligned."""
    pieces = []  # (nbytes, dtype, shape) in output order: payload, scales, ...
    for shape in shapes:
        shape = tuple(shape)
        sshape = tensor_scales_shape(shape)
        pieces.append((_numel(shape), FP8_DTYPE, shape))
        pieces.append((_numel(sshape) * 4, torch.float32, sshape))
    bufs = carve_slabs(pieces, device)
    return [(bufs[2 * j], bufs[2 * j + 1]) for j in range(len(shapes))]


# ---------------------------------------------------------------------------
# pure-torch implementation (CPU tensors)
# ---------------------------------------------------------------------------


def _as_stack(t: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """``t`` as ``[mats, R * C]``, one row per scale."""
    return t.reshape(scales.numel(), -1)


def _quantize_torch(
    x: torch.Tensor, payload: torch.Tensor, scales: torch.Tensor
) -> None:
    if x.numel() == 0:
        return
    xf = _as_stack(x.float(), scales)
    amax = xf.abs().amax(dim=1, keepdim=True).clamp_min(AMAX_FLOOR)
    # tensor / tensor: a division by a python scalar may be computed as a
    # multiplication by its reciprocal, which is not the same rounding
    top = torch.full_like(amax, FP8_MAX)
    q = (xf * (top / amax)).clamp(-FP8_MAX, FP8_MAX)
    payload.copy_(q.to(FP8_DTYPE).reshape(x.shape))
    scales.copy_((amax / top).reshape(scales.shape))


def _dequantize_torch(
    payload: torch.Tensor, scales: torch.Tensor, out: torch.Tensor
) -> None:
    if payload.numel() == 0:
        return
    y = _as_stack(payload.float(), scales) * scales.reshape(-1, 1)
    out.copy_(y.reshape(out.shape))  # f32 -> out.dtype rounds to nearest even


# ---------------------------------------------------------------------------
# public entry points
# ---------------------------------------------------------------------------


def quantize_fp8_tensor(
    tensors: Sequence[torch.Tensor],
) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """Quantise each tensor; returns ``[(payload, scales), ...]`` on the
    tensors' own devices.  All CUDA tensors of one device share the TWO kernel
    launches of a call on the caller's current stream (asynchronous); CPU
    tensors use the torch implementation of the same recipe."""
    tensors = list(tensors)
    for t in tensors:
        _check_wide(t, "quantize_fp8_tensor input")
    out: List[Tuple[torch.Tensor, torch.Tensor]] = [None] * len(tensors)
    by_device: Dict[torch.device, List[int]] = {}
    for i, t in enumerate(tensors):
        by_device.setdefault(t.device, []).append(i)
    launches: Dict[torch.device, list] = {}
    for device, idxs in by_device.items():
        bufs = alloc_tensor_quantized([tensors[i].shape for i in idxs], device)
        for i, (payload, scales) in zip(idxs, bufs):
            out[i] = (payload, scales)
            t = tensors[i]
            if device.type != "cuda":
                _quantize_torch(t, payload, scales)
            elif t.numel():
                tc = t.contiguous()
                launches.setdefault(device, []).append((tc, payload, scales))
    _launch("quant_tensor_batch", launches)
    return out


def dequantize_fp8_tensor_into(
    pairs: Sequence[Tuple[torch.Tensor, torch.Tensor]],
    outs: Sequence[torch.Tensor],
) -> None:
    """``outs[i] <- dequantise(pairs[i])`` in ``outs[i].dtype`` (f32, bf16 or
    f16).  One kernel launch per CUDA device on the caller's current stream;
    a non-contiguous output is written through a scratch buffer."""
    pairs = list(pairs)
    outs = list(outs)
    if len(pairs) != len(outs):
        raise ValueError("dequantize_fp8_tensor_into: pairs/outs length mismatch")
    launches: Dict[torch.device, list] = {}
    scratch = []  # (scratch, out) copied back after the launch
    for (payload, scales), out in zip(pairs, outs):
        _check_wide(out, "dequantize_fp8_tensor_into output")
        if payload.dtype != FP8_DTYPE or scales.dtype != torch.float32:
            raise TypeError("expected a (float8_e4m3fn, float32) pair")
        if payload.shape != out.shape or tuple(
            scales.shape
        ) != tensor_scales_shape(out.shape):
            raise ValueError(
                f"quantised pair {tuple(payload.shape)}/{tuple(scales.shape)} "
                f"does not fit an output of shape {tuple(out.shape)}"
            )
        if out.numel() == 0:
            continue
        payload = payload.to(out.device).contiguous()
        scales = scales.to(out.device).contiguous()
        if out.device.type != "cuda":
            _dequantize_torch(payload, scales, out)
            continue
        dst = out
        if not out.is_contiguous():
            dst = torch.empty(out.shape, dtype=out.dtype, device=out.device)
            scratch.append((dst, out))
        launches.setdefault(out.device, []).append((dst, payload, scales))
    _launch("dequant_tensor_batch", launches)
    for dst, out in scratch:
        out.copy_(dst)
