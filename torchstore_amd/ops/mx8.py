"""MXFP8 quantisation for transfer and storage (K16/K17): OCP E4M3 values
with one E8M0 (power-of-two) scale byte per block of 32, the 8-bit operand of
the scaled matrix instructions of gfx950.

Format, per tensor (OCP Microscaling v1.0, "floor" scale rule): view it as
rows of its last dimension (a 1-D tensor is one row) and cut each row into
blocks of 32 consecutive elements; the last block of a row may be short, and
its missing elements count as +0.  Per block::

    amax  = max |x|
    code  = max(expfield(amax) - 8, 0)     (bits 30..23 of amax as f32; stored)
    X     = 2**(code - 127)                (code 0: the f32 subnormal 2**-127)
    v     = x * 2**(127 - code)            (exact, or both sides zero; |v| < 512)
    q     = rne_to_e4m3fn(clamp(v, -448, 448)), sign of v kept (also on zero)
    y     = to_dst_dtype_rne(float(q) * X) (one fp32 multiply)

8 is emax of E4M3; this is the rule of ``ops/mx.py`` with its 2 replaced.
The payload is ``torch.float8_e4m3fn`` of the source's shape, the scales are
``torch.uint8`` of shape ``[*shape[:-1], ceil(cols / 32)]`` (a consumer may
view them as ``torch.float8_e8m0fnu``): 8.25 bits per element.

The scale rule is the standard one on purpose: a block whose amax lies in
(448 X, 512 X) saturates its top values to 448 X.  Round trip, per element:
``|y - x| <= |x| * 2**-3 + X * 2**-10 + |x| * 2**-8``.  With ``v = x / X``
(exact): where ``448 < |v| < 512`` the result is 448, and ``|v| - 448 <
|v| / 8`` exactly because ``|v| < 512``; elsewhere a normal result (``|v| >=
2**-6``, steps of 2**-3 relative to the power of two below) is within half a
step, at most ``|v| * 2**-4``, and a subnormal one (step 2**-9) within
``2**-10``.  Times ``X`` that is the first two terms.  ``q * X`` is exact in
fp32 unless it is an f32 subnormal; a non-zero ``|q| <= 2 |v|`` (the worst
case is ``|v|`` just above ``2**-10`` becoming ``2**-9``), so the narrowing
to bf16 adds at most ``|q X| * 2**-9 <= |x| * 2**-8`` (f32 adds nothing, f16
less where it neither overflows nor goes subnormal).

Every step is integer work on the bits or one correctly rounded IEEE fp32
operation, so the HIP kernels (``csrc/quant_mx8.h``, one launch per call over
all CUDA tensors of a device) and the pure-torch implementation below (the
path for CPU tensors) produce the same bytes.  Non-finite inputs are outside
the contract (they poison their own block only); finite input never produces
scale code 255 nor the two E4M3 NaN codes.  Dequantising follows IEEE: scale
code 255 makes its block NaN, a NaN code is NaN, code 254 times 448 overflows
to ``inf``, f16 outputs overflow and go subnormal where the product does, and
a zero keeps the sign of its code.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import torch

from torchstore_amd.ops.mx import _scale_values
from torchstore_amd.ops.quant import (
    FP8_DTYPE,
    FP8_MAX,
    QUANT_DTYPES,
    _check_wide,
    _numel,
    carve_slabs,
)

BLOCK = 32
EMAX = 8


@dataclass
class Mxfp8QuantizedTensor:
    """An MXFP8 tensor: what ``get_state_dict(dequantize=False)`` returns per
    entry pushed with ``transfer_quant="mxfp8_e4m3"``, and a valid in-place
    destination for one."""

    payload: torch.Tensor  # float8_e4m3fn, the original shape
    scales: torch.Tensor  # uint8 (e8m0), [*shape[:-1], ceil(shape[-1] / 32)]
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
        dequantize_mxfp8_into([(self.payload, self.scales)], [out])
        return out


def mx8_scales_shape(shape: Sequence[int]) -> Tuple[int, ...]:
    shape = tuple(shape)
    if not shape:
        raise ValueError("block quantisation needs at least one dimension")
    return shape[:-1] + ((shape[-1] + BLOCK - 1) // BLOCK,)


def alloc_mx8(
    shapes: Sequence[Sequence[int]], device: torch.device
) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """Uninitialised ``(payload, scales)`` buffers for tensors of ``shapes``
    on ``device``, carved from shared slabs: every buffer contiguous, every
    non-empty one at least 16 B aligned."""
    pieces = []
    for shape in shapes:
        shape = tuple(shape)
        sshape = mx8_scales_shape(shape)
        pieces.append((_numel(shape), FP8_DTYPE, shape))
        pieces.append((_numel(sshape), torch.uint8, sshape))
    bufs = carve_slabs(pieces, device)
    return [(bufs[2 * j], bufs[2 * j + 1]) for j in range(len(shapes))]


# ---------------------------------------------------------------------------
# pure-torch implementation (CPU tensors)
# ---------------------------------------------------------------------------


def _blocked(x2d: torch.Tensor, nblk: int) -> torch.Tensor:
    """[rows, cols] -> [rows, nblk, 32], padded with +0 on the right."""
    rows, cols = x2d.shape
    pad = nblk * BLOCK - cols
    if pad:
        x2d = torch.nn.functional.pad(x2d, (0, pad))
    return x2d.reshape(rows, nblk, BLOCK).contiguous()


def _quantize_torch(
    x: torch.Tensor, payload: torch.Tensor, scales: torch.Tensor
) -> None:
    if x.numel() == 0:
        return
    cols = x.shape[-1]
    nblk = scales.shape[-1]
    xb = _blocked(x.reshape(-1, cols).float(), nblk)
    amax = (xb.view(torch.int32) & 0x7FFFFFFF).amax(dim=-1)
    code = ((amax >> 23) - EMAX).clamp_min(0)
    inv = ((254 - code) << 23).view(torch.float32)  # 2**(127 - code)
    v = (xb * inv.unsqueeze(-1)).clamp(-FP8_MAX, FP8_MAX)
    v = v.reshape(-1, nblk * BLOCK)[:, :cols]
    payload.copy_(v.to(FP8_DTYPE).reshape(x.shape))  # rne, sign kept on zero
    scales.copy_(code.to(torch.uint8).reshape(scales.shape))


def _dequantize_torch(
    payload: torch.Tensor, scales: torch.Tensor, out: torch.Tensor
) -> None:
    if out.numel() == 0:
        return
    cols = out.shape[-1]
    nblk = scales.shape[-1]
    qb = _blocked(payload.reshape(-1, cols).float(), nblk)
    y = qb * _scale_values(scales).reshape(-1, nblk, 1)
    y = y.reshape(-1, nblk * BLOCK)[:, :cols]
    out.copy_(y.reshape(out.shape))  # f32 -> out.dtype rounds to nearest even


# ---------------------------------------------------------------------------
# public entry points
# ---------------------------------------------------------------------------


def _launch(kind: str, triples_by_device: Dict[torch.device, list]) -> None:
    from torchstore_amd.ops import gpu

    for device, triples in triples_by_device.items():
        getattr(gpu, kind)(triples, device)


def quantize_mxfp8(
    tensors: Sequence[torch.Tensor],
) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """Quantise each tensor; returns ``[(payload, scales), ...]`` on the
    tensors' own devices.  All CUDA tensors of one device share ONE kernel
    launch on the caller's current stream (asynchronous); CPU tensors use
    the torch implementation of the same recipe."""
    tensors = list(tensors)
    for t in tensors:
        _check_wide(t, "quantize_mxfp8 input")
    out: List[Tuple[torch.Tensor, torch.Tensor]] = [None] * len(tensors)
    by_device: Dict[torch.device, List[int]] = {}
    for i, t in enumerate(tensors):
        by_device.setdefault(t.device, []).append(i)
    launches: Dict[torch.device, list] = {}
    for device, idxs in by_device.items():
        bufs = alloc_mx8([tensors[i].shape for i in idxs], device)
        for i, (payload, scales) in zip(idxs, bufs):
            out[i] = (payload, scales)
            t = tensors[i]
            if device.type != "cuda":
                _quantize_torch(t, payload, scales)
            elif t.numel():
                tc = t.contiguous()
                launches.setdefault(device, []).append((tc, payload, scales))
    _launch("quant_mx8_batch", launches)
    return out


def dequantize_mxfp8_into(
    pairs: Sequence[Tuple[torch.Tensor, torch.Tensor]],
    outs: Sequence[torch.Tensor],
) -> None:
    """``outs[i] <- dequantise(pairs[i])`` in ``outs[i].dtype`` (f32, bf16 or
    f16).  One kernel launch per CUDA device on the caller's current stream;
    a non-contiguous output is written through a scratch buffer."""
    pairs = list(pairs)
    outs = list(outs)
    if len(pairs) != len(outs):
        raise ValueError("dequantize_mxfp8_into: pairs/outs length mismatch")
    launches: Dict[torch.device, list] = {}
    scratch = []  # (scratch, out) copied back after the launch
    for (payload, scales), out in zip(pairs, outs):
        _check_wide(out, "dequantize_mxfp8_into output")
        if payload.dtype != FP8_DTYPE or scales.dtype != torch.uint8:
            raise TypeError("expected a (float8_e4m3fn, uint8) pair")
        if payload.shape != out.shape or tuple(
            scales.shape
        ) != mx8_scales_shape(out.shape):
            raise ValueError(
                f"mxfp8 pair {tuple(payload.shape)}/{tuple(scales.shape)} "
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
    _launch("dequant_mx8_batch", launches)
    for dst, out in scratch:
        out.copy_(dst)


__all__ = [
    "BLOCK",
    "QUANT_DTYPES",
    "Mxfp8QuantizedTensor",
    "alloc_mx8",
    "dequantize_mxfp8_into",
    "mx8_scales_shape",
    "quantize_mxfp8",
]
