"""The MXFP4 recipe written out independently of ``torchstore_amd.ops.mx``,
and the input grids of its tests.

Scale: integer work on the bits of the block's amax.  E2M1: the nearest of
the eight magnitudes, searched in float64, ties to the even code, saturating
at 6, the sign bit kept.  One fp32 multiply on each side (numpy float32), and
the narrowing into the output dtype by the references of
``tests/value_grids.py``.  ``tests/test_mx.py`` (CPU) and
``tests/test_gpu_mx.py`` (the kernels) check against the same thing.

No test functions and no GPU use in here.
"""

import numpy as np
import torch

from tests.value_grids import (
    BF16,
    F16,
    F32,
    _narrow_bits,
    _step_ulps,
    _widen_bits,
    bits_of,
    from_bits,
)

BLOCK = 32
DTYPES = (F32, BF16, F16)
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
SHAPES = [(1, 1), (3, 32), (3, 33), (3, 128), (5, 200), (4, 7, 130), (257,)]
# scale codes of the dequant grids: the subnormal X, the smallest normal one,
# one that puts f16 outputs into the subnormal range, 1.0, a mild f16
# overflow, 6 * X overflowing f32, and the NaN code
DEQUANT_CODES = (0, 1, 107, 127, 143, 254, 255)


def shapes_of(shape):
    cols = shape[-1]
    return (
        tuple(shape[:-1]) + (-(-cols // 2),),
        tuple(shape[:-1]) + (-(-cols // BLOCK),),
    )


def e2m1_rne(v32):
    """Nibbles (uint8) of f32 values: nearest magnitude in float64, ties to
    the even code, saturating at 6, sign bit of the input kept."""
    v32 = np.asarray(v32, dtype=np.float32)
    a = np.minimum(np.abs(v32.astype(np.float64)), E2M1[-1])
    hi = np.searchsorted(E2M1, a, side="left")  # E2M1[hi] >= a
    lo = np.maximum(hi - 1, 0)
    dlo, dhi = a - E2M1[lo], E2M1[hi] - a  # exact in float64
    code = np.where(dhi < dlo, hi, lo)
    code = np.where(dhi == dlo, np.where(hi % 2 == 0, hi, lo), code)
    return (code | np.where(np.signbit(v32), 8, 0)).astype(np.uint8)


def scale_value(code):
    """2**(code - 127) as float32; code 255 is NaN."""
    code = np.asarray(code, dtype=np.int64)
    with np.errstate(over="ignore"):
        x = np.ldexp(np.float64(1.0), code - 127).astype(np.float32)  # exact
    return np.where(code == 255, np.float32(np.nan), x).astype(np.float32)


def _rows_f32(x):
    """[rows, cols] float32 (exact widening) of a float tensor."""
    cols = x.shape[-1]
    bits = _widen_bits(bits_of(x), x.dtype)
    return bits.view(np.float32).reshape(-1, cols)


def oracle_quant(x):
    """(payload uint8 [*, ceil(cols/2)], scales uint8 [*, ceil(cols/32)])."""
    x = x.detach().cpu()
    cols = x.shape[-1]
    nblk = -(-cols // BLOCK)
    x2d = _rows_f32(x)
    rows = x2d.shape[0]
    padded = np.zeros((rows, nblk * BLOCK), dtype=np.float32)  # +0
    padded[:, :cols] = x2d
    xb = padded.reshape(rows, nblk, BLOCK)
    amax_bits = (xb.view(np.uint32) & 0x7FFFFFFF).max(axis=-1)
    code = np.maximum((amax_bits >> 23).astype(np.int64) - 2, 0)
    inv = ((254 - code).astype(np.uint32) << 23).view(np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        v = (xb * inv[:, :, None]).astype(np.float32)  # one fp32 multiply
    nib = e2m1_rne(v).reshape(rows, nblk * BLOCK)
    even = cols + (cols & 1)
    nib = nib[:, :even].copy()
    if cols & 1:
        nib[:, cols] = 0
    packed = (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)
    pshape, sshape = shapes_of(tuple(x.shape))
    return (
        torch.from_numpy(packed.reshape(pshape)),
        torch.from_numpy(code.astype(np.uint8).reshape(sshape)),
    )


def dequant_bits(payload, scales, shape, dtype):
    """Bits (flat numpy) of the dequantised tensor of logical ``shape``."""
    cols = shape[-1]
    p = payload.detach().cpu().contiguous().numpy()
    p = p.reshape(-1, p.shape[-1])
    rows = p.shape[0]
    nib = np.stack([p & 0xF, p >> 4], axis=-1).reshape(rows, -1)[:, :cols]
    q = np.where(nib & 8, -E2M1[nib & 7], E2M1[nib & 7]).astype(np.float32)
    s = scales.detach().cpu().contiguous().numpy().reshape(rows, -1)
    X = np.repeat(scale_value(s), BLOCK, axis=1)[:, :cols]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        y = (q * X).astype(np.float32)  # one fp32 multiply
    return _narrow_bits(np.ascontiguousarray(y).reshape(-1).view(np.uint32), dtype)


def oracle_dequant(payload, scales, shape, dtype):
    """The dequantised tensor itself (NaN payloads as the references give)."""
    return from_bits(dequant_bits(payload, scales, shape, dtype), dtype).reshape(
        tuple(shape)
    )


def block_scale(scales, cols):
    """X of every element, float64, [..., cols]."""
    X = torch.from_numpy(scale_value(scales.cpu().numpy()).astype(np.float64))
    return X.repeat_interleave(BLOCK, dim=-1)[..., :cols]


# ---------------------------------------------------------------------------
# grids
# ---------------------------------------------------------------------------

TIE_KS = {
    F32: (0, -7, 5, 122, -127),
    BF16: (0, -7, 5, 122, -127),
    F16: (0, -7, 5, 12, -16),
}
TIE_CASES = [(d, k) for d in DTYPES for k in TIE_KS[d]]


def e2m1_tie_grid(dtype, k):
    """[rows, 32] of ``dtype``.  Column 0 of every row is 7 * 2**k: the
    block's X is 2**k and that column saturates to 6.  The other columns
    hold, times 2**k, the seven midpoints between adjacent e2m1 values, their
    neighbours one ulp of ``dtype`` up and down, the eight values and 7.0,
    all with both signs."""
    vals = torch.from_numpy(E2M1.copy())
    mids = (vals[:-1] + vals[1:]) / 2
    s = 2.0 ** k
    mids_t = (mids * s).to(dtype)
    vals_t = (vals * s).to(dtype)
    seven = torch.tensor([7.0 * s], dtype=torch.float64).to(dtype)
    # exact in dtype: the casts above rounded nothing
    assert torch.equal(mids_t.double(), mids * s)
    assert torch.equal(vals_t.double(), vals * s)
    assert seven.double().item() == 7.0 * s
    pos = torch.cat(
        [mids_t, _step_ulps(mids_t, 1), _step_ulps(mids_t, -1), vals_t, seven]
    )
    flat = torch.cat([pos, -pos])
    rows = -(-flat.numel() // (BLOCK - 1))
    body = torch.zeros(rows * (BLOCK - 1), dtype=dtype)
    body[: flat.numel()] = flat
    grid = torch.empty(rows, BLOCK, dtype=dtype)
    grid[:, 0] = seven
    grid[:, 1:] = body.view(rows, BLOCK - 1)
    return grid


def all_bytes_payload():
    """([16, 16] uint8 holding every byte value once, logical shape
    [16, 32]): every pair of nibbles, one block per row."""
    return torch.arange(256, dtype=torch.int32).to(torch.uint8).view(16, 16), (16, 32)


def scales_for(shape, code):
    return torch.full(shapes_of(shape)[1], code, dtype=torch.uint8)
