"""MXFP4 quantisation for transfer and storage (K6/K7): packed OCP E2M1
values with one E8M0 (power-of-two) scale byte per block of 32.

Format, per tensor (OCP Microscaling v1.0, "floor" scale rule): view it as
rows of its last dimension (a 1-D tensor is one row) and cut each row into
blocks of 32 consecutive elements; the last block of a row may be short, and
its missing elements count as +0.  Per block::

    amax  = max |x|
    code  = max(expfield(amax) - 2, 0)     (bits 30..23 of amax as f32; stored)
    X     = 2**(code - 127)
    v     = x * 2**(127 - code)            (one fp32 multiply)
    q     = rne_to_e2m1(v), saturating at +-6, sign of v kept (also on zero)
    y     = to_dst_dtype_rne(float(q) * X) (one fp32 multiply)

E2M1 magnitudes by code 0..7 are 0, 0.5, 1, 1.5, 2, 3, 4, 6; a nibble is
``sign << 3 | code`` and ties go to the even code.  Element ``2j`` of a row
is the low nibble of the row's byte ``j``, element ``2j + 1`` the high one
(the order of ``torch.float4_e2m1fn_x2``); rows never share a byte, and with
an odd row length the last high nibble is 0.  The payload is ``torch.uint8``
of shape ``[*shape[:-1], ceil(cols / 2)]``, the scales are ``torch.uint8`` of
shape ``[*shape[:-1], ceil(cols / 32)]``: 4.25 bits per element.

The scale rule is the standard one on purpose: a block whose amax lies in
(6X, 8X) saturates its top values to 6X.  Round trip:
``|y - x| <= 2 * X + |x| * 2**-8``.

Every step is integer work on the bits or one correctly rounded IEEE fp32
operation, so the HIP kernels (``csrc/quant_mx.h``, one launch per call over
all CUDA tensors of a device) and the pure-torch implementation below (the
path for CPU tensors) produce the same bytes.  Non-finite inputs are outside
the contract (they poison their own block only); finite input never produces
scale code 255.  Dequantising follows IEEE: scale code 255 makes its block
NaN, code 254 times 6 overflows to ``inf``, f16 outputs overflow and go
subnormal where the product does, and a zero keeps the sign of its nibble.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import torch

from torchstore_amd.ops.quant import QUANT_DTYPES, _check_wide, carve_slabs

BLOCK = 32

_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


@dataclass
class MxQuantizedTensor:
    """An MXFP4 tensor: what ``get_state_dict(dequantize=False)`` returns per
    entry pushed with ``transfer_quant="mxfp4"``, and a valid in-place
    destination for one.  ``shape`` is the logical shape: an odd last
    dimension cannot be told from the payload."""

    payload: torch.Tensor  # uint8, [*shape[:-1], ceil(shape[-1] / 2)]
    scales: torch.Tensor  # uint8, [*shape[:-1], ceil(shape[-1] / 32)]
    shape: Tuple[int, ...]
    orig_dtype: torch.dtype

    def __post_init__(self):
        self.shape = torch.Size(self.shape)

    def dequantize(self, dtype: torch.dtype = None) -> torch.Tensor:
        out = torch.empty(
            self.shape,
            dtype=dtype or self.orig_dtype,
            device=self.payload.device,
        )
        dequantize_mxfp4_into([(self.payload, self.scales)], [out])
        return out


def mx_shapes(shape: Sequence[int]) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
    """``(payload_shape, scales_shape)`` of a tensor of ``shape``."""
    shape = tuple(shape)
    if not shape:
        raise ValueError("block quantisation needs at least one dimension")
    cols = shape[-1]
    return (
        shape[:-1] + ((cols + 1) // 2,),
        shape[:-1] + ((cols + BLOCK - 1) // BLOCK,),
    )


def _numel(shape: Sequence[int]) -> int:
    n = 1
    for s in shape:
        n *= s
    return n


def alloc_mx(
    shapes: Sequence[Sequence[int]], device: torch.device
) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """Uninitialised ``(payload, scales)`` buffers for tensors of the logical
    ``shapes`` on ``device``, carved from shared slabs: every buffer
    contiguous, every non-empty one at least 16 B aligned."""
    pieces = []
    for shape in shapes:
        for s in mx_shapes(shape):
            pieces.append((_numel(s), torch.uint8, s))
    bufs = carve_slabs(pieces, device)
    return [(bufs[2 * j], bufs[2 * j + 1]) for j in range(len(shapes))]


# ---------------------------------------------------------------------------
# pure-torch implementation (CPU tensors)
# ---------------------------------------------------------------------------


def _quantize_torch(
    x: torch.Tensor, payload: torch.Tensor, scales: torch.Tensor
) -> None:
    if x.numel() == 0:
        return
    cols = x.shape[-1]
    nblk = scales.shape[-1]
    x2d = x.reshape(-1, cols).float()
    rows = x2d.shape[0]
    pad = nblk * BLOCK - cols
    if pad:
        x2d = torch.nn.functional.pad(x2d, (0, pad))  # +0
    xb = x2d.reshape(rows, nblk, BLOCK).contiguous()
    amax = (xb.view(torch.int32) & 0x7FFFFFFF).amax(dim=-1)
    code = ((amax >> 23) - 2).clamp_min(0)
    inv = ((254 - code) << 23).view(torch.float32)  # 2**(127 - code)
    v = xb * inv.unsqueeze(-1)
    a = v.abs()
    mag = torch.zeros(a.shape, dtype=torch.uint8)
    for t, tie_up in (
        (0.25, False), (0.75, True), (1.25, False), (1.75, True),
        (2.5, False), (3.5, True), (5.0, False),
    ):  # a tie goes up where the code above it is the even one
        mag += (a >= t) if tie_up else (a > t)
    nib = mag | (torch.signbit(v).to(torch.uint8) << 3)
    # an odd row takes one padding element along: +0, so a 0 high nibble
    nib = nib.reshape(rows, nblk * BLOCK)[:, : cols + (cols & 1)]
    packed = nib[:, 0::2] | (nib[:, 1::2] << 4)
    payload.copy_(packed.reshape(payload.shape))
    scales.copy_(code.to(torch.uint8).reshape(scales.shape))


def _scale_values(scales: torch.Tensor) -> torch.Tensor:
    """2**(code - 127) as f32: code 0 is a subnormal, code 255 is NaN."""
    code = scales.to(torch.int32)
    bits = torch.where(code == 0, torch.full_like(code, 0x00400000), code << 23)
    bits = torch.where(code == 255, torch.full_like(code, 0x7FC00000), bits)
    return bits.view(torch.float32)


def _dequantize_torch(
    payload: torch.Tensor, scales: torch.Tensor, out: torch.Tensor
) -> None:
    if out.numel() == 0:
        return
    cols = out.shape[-1]
    nblk = scales.shape[-1]
    p2d = payload.reshape(-1, payload.shape[-1])
    rows = p2d.shape[0]
    nib = torch.stack([p2d & 0xF, p2d >> 4], dim=-1).reshape(rows, -1)
    table = torch.tensor(_E2M1 + tuple(-m for m in _E2M1), dtype=torch.float32)
    q = table[nib.long()]  # -0.0 for nibble 8
    pad = nblk * BLOCK - q.shape[1]
    if pad:
        q = torch.nn.functional.pad(q, (0, pad))
    y = q.reshape(rows, nblk, BLOCK) * _scale_values(scales).reshape(rows, nblk, 1)
    y = y.reshape(rows, nblk * BLOCK)[:, :cols]
    out.copy_(y.reshape(out.shape))  # f32 -> out.dtype rounds to nearest even


# ---------------------------------------------------------------------------
# public entry points
# ---------------------------------------------------------------------------


def _launch(kind: str, triples_by_device: Dict[torch.device, list]) -> None:
    from torchstore_amd.ops import gpu

    for device, triples in triples_by_device.items():
        getattr(gpu, kind)(triples, device)


def quantize_mxfp4(
    tensors: Sequence[torch.Tensor],
) -> List[Tuple[torch.Tensor, torch.Tensor]]:
    """Quantise each tensor; returns ``[(payload, scales), ...]`` on the
    tensors' own devices.  All CUDA tensors of one device share ONE kernel
    launch on the caller's current stream (asynchronous); CPU tensors use
    the torch implementation of the same recipe."""
    tensors = list(tensors)
    for t in tensors:
        _check_wide(t, "quantize_mxfp4 input")
    out: List[Tuple[torch.Tensor, torch.Tensor]] = [None] * len(tensors)
    by_device: Dict[torch.device, List[int]] = {}
    for i, t in enumerate(tensors):
        by_device.setdefault(t.device, []).append(i)
    launches: Dict[torch.device, list] = {}
    for device, idxs in by_device.items():
        bufs = alloc_mx([tensors[i].shape for i in idxs], device)
        for i, (payload, scales) in zip(idxs, bufs):
            out[i] = (payload, scales)
            t = tensors[i]
            if device.type != "cuda":
                _quantize_torch(t, payload, scales)
            elif t.numel():
                tc = t.contiguous()
                launches.setdefault(device, []).append((tc, payload, scales))
    _launch("quant_mx_batch", launches)
    return out


def dequantize_mxfp4_into(
    pairs: Sequence[Tuple[torch.Tensor, torch.Tensor]],
    outs: Sequence[torch.Tensor],
) -> None:
    """``outs[i] <- dequantise(pairs[i])`` in ``outs[i].dtype`` (f32, bf16 or
    f16); ``outs[i].shape`` is the logical shape the pair must belong to.
    One kernel launch per CUDA device on the caller's current stream; a
    non-contiguous output is written through a scratch buffer."""
    pairs = list(pairs)
    outs = list(outs)
    if len(pairs) != len(outs):
        raise ValueError("dequantize_mxfp4_into: pairs/outs length mismatch")
    launches: Dict[torch.device, list] = {}
    scratch = []  # (scratch, out) copied back after the launch
    for (payload, scales), out in zip(pairs, outs):
        _check_wide(out, "dequantize_mxfp4_into output")
        if payload.dtype != torch.uint8 or scales.dtype != torch.uint8:
            raise TypeError("expected a (uint8, uint8) payload/scales pair")
        if (tuple(payload.shape), tuple(scales.shape)) != mx_shapes(out.shape):
            raise ValueError(
                f"mxfp4 pair {tuple(payload.shape)}/{tuple(scales.shape)} "
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
    _launch("dequant_mx_batch", launches)
    for dst, out in scratch:
        out.copy_(dst)


__all__ = [
    "BLOCK",
    "QUANT_DTYPES",
    "MxQuantizedTensor",
    "alloc_mx",
    "dequantize_mxfp4_into",
    "mx_shapes",
    "quantize_mxfp4",
]
