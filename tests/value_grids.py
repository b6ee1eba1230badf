"""Value grids for the kernels that change bits (cast K3, FP8 K4/K5) and
references for them that are written out here.

The references share no code with the HIP kernels and none with torch's
casts: e4m3 comes from a decoded table searched in float64, f32 -> bf16 is the
integer rounding on the raw bits, and f16 goes through numpy's conversions.
``tests/test_value_grids.py`` proves them (and the grids) on the CPU before
``tests/test_gpu_numerics.py`` judges a kernel by them.

No test functions and no GPU use in here.
"""

import numpy as np
import torch

BLOCK = 128
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DTYPES = (F32, BF16, F16)
CAST_PAIRS = (
    (F32, BF16), (BF16, F32), (F32, F16), (F16, F32), (BF16, F16), (F16, BF16),
)
_INT_VIEW = {F32: torch.int32, F16: torch.int16, BF16: torch.int16}
_NP_UINT = {F32: np.uint32, F16: np.uint16, BF16: np.uint16}


# ---------------------------------------------------------------------------
# raw bits
# ---------------------------------------------------------------------------


def bits_of(t):
    """The bit patterns of a float tensor as a flat unsigned numpy array."""
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view(_INT_VIEW[t.dtype]).numpy().view(_NP_UINT[t.dtype]).copy()


def bits_of_u8(payload):
    """The codes of an e4m3 tensor as a flat uint8 numpy array."""
    return payload.detach().cpu().contiguous().view(torch.uint8).numpy().reshape(-1)


def from_bits(bits, dtype):
    """Flat tensor of ``dtype`` with the given (unsigned) bit patterns."""
    u = np.ascontiguousarray(bits, dtype=_NP_UINT[dtype])
    signed = u.view(np.int32 if dtype == F32 else np.int16)
    return torch.from_numpy(signed.copy()).view(dtype)


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------


def e4m3_values():
    """The 127 finite non-negative e4m3 values, index = code (0x00..0x7E)."""
    code = np.arange(0x7F)
    e, m = code >> 3, (code & 7).astype(np.float64)
    return np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * 2.0 ** (e - 7.0))


def e4m3_decode(codes):
    """float64 value of every e4m3 code; 0x7F and 0xFF are NaN."""
    codes = np.asarray(codes, dtype=np.uint8)
    table = np.append(e4m3_values(), np.nan)
    mag = table[codes & 0x7F]
    return np.where(codes & 0x80, -mag, mag)


def e4m3_rne(x64):
    """Codes (uint8) of the nearest e4m3 values: nearest in float64, ties to
    the even code, the sign bit kept (also on zero), saturating at 448."""
    x64 = np.asarray(x64, dtype=np.float64)
    vals = e4m3_values()
    a = np.minimum(np.abs(x64), vals[-1])
    hi = np.searchsorted(vals, a, side="left")  # vals[hi] >= a
    lo = np.maximum(hi - 1, 0)
    # exact: a and its two neighbours lie within a factor of two of each
    # other, or one of them is zero
    dlo, dhi = a - vals[lo], vals[hi] - a
    code = np.where(dhi < dlo, hi, lo)
    code = np.where(dhi == dlo, np.where(hi % 2 == 0, hi, lo), code)
    code = np.where(np.isnan(x64), 0x7F, code)
    return (code | np.where(np.signbit(x64), 0x80, 0)).astype(np.uint8)


def bf16_rne_bits(f32_bits):
    """f32 -> bf16, round to nearest even, on the raw bits (not for NaN)."""
    u = np.asarray(f32_bits, dtype=np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _widen_bits(bits, dtype):
    """bf16/f16 bits -> f32 bits (exact); f32 bits unchanged."""
    if dtype == F32:
        return np.asarray(bits, dtype=np.uint32)
    if dtype == BF16:
        return np.asarray(bits, dtype=np.uint32) << 16
    f16 = np.asarray(bits, dtype=np.uint16).view(np.float16)
    return f16.astype(np.float32).view(np.uint32)


def _narrow_bits(f32_bits, dtype):
    if dtype == F32:
        return np.asarray(f32_bits, dtype=np.uint32)
    if dtype == BF16:
        return bf16_rne_bits(f32_bits)
    f32 = np.asarray(f32_bits, dtype=np.uint32).view(np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return f32.astype(np.float16).view(np.uint16)


def cast_reference_bits(src, dst_dtype):
    """Bits of ``src`` cast to ``dst_dtype``; through f32, as the kernels go.
    Meaningless where ``src`` is NaN."""
    return _narrow_bits(_widen_bits(bits_of(src), src.dtype), dst_dtype)


def check_cast(src, out, ref=None):
    """``out`` is ``src`` cast: bit for bit wherever ``src`` is not NaN, and
    NaN wherever it is.  ``ref`` may pass in ``cast_reference_bits(src,
    out.dtype)`` computed earlier.  Returns the number of elements compared
    exactly."""
    assert src.numel() == out.numel()
    if ref is None:
        ref = cast_reference_bits(src, out.dtype)
    got = bits_of(out)
    nan_in = np.isnan(_widen_bits(bits_of(src), src.dtype).view(np.float32))
    bad = np.flatnonzero((got != ref) & ~nan_in)
    assert bad.size == 0, (
        f"{src.dtype}->{out.dtype}: {bad.size} wrong, first at {bad[0]}: "
        f"in {bits_of(src)[bad[0]]:#x} got {got[bad[0]]:#x} "
        f"want {ref[bad[0]]:#x}"
    )
    out_nan = np.isnan(_widen_bits(got, out.dtype).view(np.float32))
    assert out_nan[nan_in].all(), f"{src.dtype}->{out.dtype}: NaN in, no NaN out"
    return int((~nan_in).sum())


def dequant_reference_bits(payload, scales, dtype):
    """Bits of the dequantised tensor: decoded table value times the block's
    scale as ONE fp32 multiply, then narrowed by the references above."""
    cols = payload.shape[-1]
    codes = payload.detach().cpu().contiguous().view(torch.uint8).numpy()
    q = e4m3_decode(codes.reshape(-1, cols)).astype(np.float32)  # exact
    s = scales.detach().cpu().contiguous().numpy().reshape(q.shape[0], -1)
    s = np.repeat(s, BLOCK, axis=1)[:, :cols]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        y = (q * s).astype(np.float32)
    return _narrow_bits(y.reshape(-1).view(np.uint32), dtype)


def check_dequant(out, ref_bits):
    """Bytes equal wherever the reference is not NaN; NaN where it is."""
    got = bits_of(out)
    ref_nan = np.isnan(_widen_bits(ref_bits, out.dtype).view(np.float32))
    assert np.array_equal(got[~ref_nan], ref_bits[~ref_nan]), (
        f"dequant into {out.dtype} differs from the reference"
    )
    got_nan = np.isnan(_widen_bits(got, out.dtype).view(np.float32))
    assert got_nan[ref_nan].all(), "a NaN code did not dequantise to NaN"


# ---------------------------------------------------------------------------
# cast inputs
# ---------------------------------------------------------------------------


def all_bits16(dtype):
    """All 65536 bit patterns of float16 / bfloat16, in order."""
    return from_bits(np.arange(65536, dtype=np.uint32), dtype)


def _f32_bits(values):
    return np.asarray(values, dtype=np.float64).astype(np.float32).view(np.uint32)


def f32_rounding_grid(dst_dtype):
    """(grid, nans): f32 inputs around every rounding decision of a cast to
    ``dst_dtype``.  For every finite non-negative destination pattern v: the
    midpoint to its successor, the midpoint's f32 neighbours, v and v plus
    one f32 ulp; all of it negated too; then the overflow/underflow edges."""
    if dst_dtype == BF16:
        v = np.arange(0x7F80, dtype=np.uint32) << 16
        mid = v | 0x8000  # past the largest v this is the tie that goes to inf
        edges = np.concatenate([
            _f32_bits([np.finfo(np.float32).max, np.inf, 0.0]),
            # the largest f32 that still rounds to the bf16 maximum
            np.array([0x7F7F7FFF], dtype=np.uint32),
            # f32 subnormals: below, at and above half a bf16 subnormal step
            np.array([1, 2, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0x10000,
                      0x7FFFFF], dtype=np.uint32),
        ])
    else:
        pat = np.arange(0x7C01, dtype=np.uint16)  # 0x7C00 decodes as 65536
        val = pat.view(np.float16).astype(np.float64)
        val[-1] = 65536.0
        v = _f32_bits(val[:-1])
        mid = _f32_bits((val[:-1] + val[1:]) / 2)
        assert np.array_equal(
            mid.view(np.float32).astype(np.float64), (val[:-1] + val[1:]) / 2
        )
        edges = _f32_bits([
            65504.0, 65519.99, 65520.0, 65536.0, 1e38, 2.0 ** -24, 2.0 ** -25,
            np.nextafter(np.float32(2.0 ** -25), np.float32(1.0)),
            2.0 ** -26, 2.0 ** -149, np.inf, 0.0,
        ])
    pos = np.concatenate([mid, mid + 1, mid - 1, v, v + 1, edges])
    grid = np.concatenate([pos, pos | 0x80000000]).astype(np.uint32)
    nan = np.array([
        0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF,
        0xFFFFFFFF, 0x7FA00000, 0xFFA00000,
        # payload only in the bits a narrowing cast drops: truncation gives inf
        0x7F80FFFF, 0xFF808000, 0x7F801000, 0xFF800FFF,
    ], dtype=np.uint32)
    nans = np.tile(nan, 4)[:41]  # two 16-wide vectors and a tail
    return from_bits(grid, F32), from_bits(nans, F32)


# ---------------------------------------------------------------------------
# FP8 inputs
# ---------------------------------------------------------------------------

TIE_KS = {
    F32: (0, -7, 5, -13, 118, -90),
    BF16: (0, -7, 5, -13, 118, -90),
    F16: (0, -7, 5, 7, -13),
}
TIE_CASES = [(d, k) for d in DTYPES for k in TIE_KS[d]]


def _step_ulps(t, n):
    """Positive finite tensor moved ``n`` ulps of its dtype."""
    return (t.view(_INT_VIEW[t.dtype]) + n).view(t.dtype)


def e4m3_tie_grid(dtype, k):
    """[8, 128] of ``dtype``: column 0 of every row is 448 * 2**k, so the
    block's inv is exactly 2**-k and its scale 2**k; the other columns hold,
    scaled by 2**k, the 126 midpoints between adjacent e4m3 values, their
    neighbours one ulp of ``dtype`` up and down, and the 127 values
    themselves, all of them with both signs."""
    vals = torch.from_numpy(e4m3_values())
    mids = (vals[:-1] + vals[1:]) / 2
    s = 2.0 ** k
    mids_t = (mids * s).to(dtype)
    vals_t = (vals * s).to(dtype)
    # exact in dtype: the casts above rounded nothing
    assert torch.equal(mids_t.double(), mids * s)
    assert torch.equal(vals_t.double(), vals * s)
    pos = torch.cat([
        mids_t, _step_ulps(mids_t, 1), _step_ulps(mids_t[1:], -1), vals_t,
    ])
    flat = torch.cat([pos, -pos])
    rows = -(-flat.numel() // (BLOCK - 1))
    body = torch.zeros(rows * (BLOCK - 1), dtype=dtype)
    body[: flat.numel()] = flat
    grid = torch.empty(rows, BLOCK, dtype=dtype)
    grid[:, 0] = vals_t[-1]
    grid[:, 1:] = body.view(rows, BLOCK - 1)
    return grid


SUBNORMAL_STEP = {F16: 2.0 ** -24, BF16: 2.0 ** -133, F32: 2.0 ** -149}


def subnormal_block(dtype):
    """One [1, 128] block of m * step, m = 0..127 permuted, sign alternating
    (negative at even positions, so the zero is a -0); step is the smallest
    subnormal of ``dtype``, so the bit pattern of |x| is m itself."""
    i = np.arange(BLOCK)
    m = (i * 37) % BLOCK
    sign = 0x80000000 if dtype == F32 else 0x8000
    bits = m | np.where(i % 2 == 0, sign, 0)
    return from_bits(bits.astype(np.uint32), dtype).view(1, BLOCK)


def zero_and_tiny_blocks(dtype):
    """[3, 384]: an all-zero block at [1, 128:256] and a block of +-2**-100
    (below the amax floor; zeros in f16, which cannot hold it) at [2, 0:128]
    among blocks of ordinary data."""
    from tests.test_quant import make_input

    x = make_input((3, 384), torch.float32)
    x[1, 128:256] = 0.0
    tiny = 2.0 ** -100 if dtype != torch.float16 else 0.0
    x[2, 0:128] = tiny
    x[2, 5] = -tiny
    return x.to(dtype)


def all_codes_payload():
    """[3, 128] e4m3: every one of the 256 codes (the first 128 twice)."""
    codes = (np.arange(3 * BLOCK) % 256).astype(np.uint8)
    return torch.from_numpy(codes).view(torch.float8_e4m3fn).view(3, BLOCK)


# a power of two; the floor scale; near the top of f32 (f16 outputs overflow
# to inf); one that puts many f16 outputs into the subnormal range; a mild
# f16 overflow.  Each is the exact value of an f32.
DEQUANT_SCALES = tuple(
    float(np.float32(s))
    for s in (
        1.0,
        np.float32(2.0 ** -96) / np.float32(448.0),
        3e35,
        1.2345e-7,
        200.0,
    )
)


def scales_for(payload, scale):
    return torch.full(
        (*payload.shape[:-1], -(-payload.shape[-1] // BLOCK)), scale,
        dtype=torch.float32,
    )
