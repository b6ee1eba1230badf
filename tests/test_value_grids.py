"""The references and grids of ``tests/value_grids.py`` are right: proved on
the CPU, against torch's CPU casts, the oracle of ``tests/test_quant.py`` and
the CPU path of ``ops.quant``, before any kernel is judged by them
(``tests/test_gpu_numerics.py``)."""

import numpy as np
import pytest
import torch

from tests import value_grids as vg
from tests.test_quant import (
    assert_pair_matches,
    oracle_dequant,
    oracle_quant,
    same_bytes,
)
from tests.value_grids import BF16, DTYPES, F16, F32

FLOOR_SCALE = torch.tensor(2.0 ** -96) / torch.tensor(448.0)


def _ids(value):
    return str(value).replace("torch.", "")


# ---------------------------------------------------------------------------
# the e4m3 table and rounding
# ---------------------------------------------------------------------------


def test_e4m3_table_is_torchs_decode():
    vals = vg.e4m3_values()
    assert vals.shape == (127,) and vals[0] == 0 and vals[-1] == 448.0
    assert vals[1] == 2.0 ** -9 and (np.diff(vals) > 0).all()
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    decoded = codes.view(torch.float8_e4m3fn).double().numpy()
    ours = vg.e4m3_decode(codes.numpy())
    assert np.array_equal(np.isnan(ours), np.isnan(decoded))
    assert np.isnan(ours).sum() == 2
    ok = ~np.isnan(ours)
    assert np.array_equal(ours[ok], decoded[ok])
    assert np.array_equal(np.signbit(ours[ok]), np.signbit(decoded[ok]))


def test_e4m3_rne_by_hand():
    x = [0.0, -0.0, 2.0 ** -10, -(2.0 ** -10), 3 * 2.0 ** -10, 2.0 ** -11,
         1.0, 1.0625, 1.1875, 1.0626, 448.0, 464.0, 1e9, -1e9, 17.0, 19.0]
    want = [0x00, 0x80, 0x00, 0x80, 0x02, 0x00,
            0x38, 0x38, 0x3A, 0x39, 0x7E, 0x7E, 0x7E, 0xFE, 0x58, 0x5A]
    assert vg.e4m3_rne(x).tolist() == want
    codes = np.arange(256, dtype=np.uint8)
    ok = (codes & 0x7F) != 0x7F
    assert np.array_equal(vg.e4m3_rne(vg.e4m3_decode(codes[ok])), codes[ok])


# ---------------------------------------------------------------------------
# cast references against torch's CPU casts
# ---------------------------------------------------------------------------


@pytest.mark.parametrize(
    "src_dtype,dst_dtype",
    [(BF16, F32), (F16, F32), (BF16, F16), (F16, BF16)],
    ids=_ids,
)
def test_cast_reference_all_16bit_sources(src_dtype, dst_dtype):
    src = vg.all_bits16(src_dtype)
    assert np.array_equal(vg.bits_of(src), np.arange(65536))
    n = vg.check_cast(src, src.to(dst_dtype))
    # every pattern but the NaNs (7 / 10 mantissa bits, two signs)
    assert n == 65536 - 2 * ((1 << (7 if src_dtype == BF16 else 10)) - 1)


@pytest.mark.parametrize("dst_dtype", [BF16, F16], ids=_ids)
def test_cast_reference_f32_rounding_grid(dst_dtype):
    grid, nans = vg.f32_rounding_grid(dst_dtype)
    assert grid.dtype == F32 and 300_000 < grid.numel() < 450_000
    assert not torch.isnan(grid).any() and torch.isnan(nans).all()
    assert vg.check_cast(grid, grid.to(dst_dtype)) == grid.numel()
    assert vg.check_cast(nans, nans.to(dst_dtype)) == 0
    out = vg.from_bits(vg.cast_reference_bits(grid, dst_dtype), dst_dtype)
    # the grid reaches every destination pattern that is not a NaN
    n_nan = 2 * ((1 << (7 if dst_dtype == BF16 else 10)) - 1)
    assert np.unique(vg.bits_of(out)).size == 65536 - n_nan
    # and holds real ties: inputs exactly half way between two neighbours
    back = out.double()
    err = (grid.double() - back).abs()
    fin = torch.isfinite(back)
    up = vg.from_bits(vg.bits_of(out) + 1, dst_dtype).double()
    tie = fin & torch.isfinite(up) & (err * 2 == (up - back).abs()) & (err > 0)
    assert tie.sum() > 20_000


def test_check_cast_notices_a_wrong_bit():
    src = vg.all_bits16(F16)
    out = src.to(BF16)
    vg.check_cast(src, out)
    out.view(torch.int16)[12345] ^= 1
    with pytest.raises(AssertionError, match="1 wrong"):
        vg.check_cast(src, out)
    out = src.to(BF16)
    out.view(torch.int16)[0x7C01] = 0x7F80  # a NaN input turned into inf
    with pytest.raises(AssertionError, match="NaN in"):
        vg.check_cast(src, out)


# ---------------------------------------------------------------------------
# quantise on every tie grid
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype,k", vg.TIE_CASES, ids=_ids)
def test_tie_grid_quant(dtype, k):
    from torchstore_amd.ops import quant

    x = vg.e4m3_tie_grid(dtype, k)
    assert x.shape == (8, 128) and x.dtype == dtype
    assert torch.isfinite(x).all()
    assert (x[:, 0].double() == 448.0 * 2.0 ** k).all()
    unit = x.double().numpy() / 2.0 ** k  # exact: a power of two
    vals = vg.e4m3_values()
    mids = (vals[:-1] + vals[1:]) / 2
    assert np.isin(mids, unit).all() and np.isin(-mids, unit).all()
    assert np.isin(vals, unit).all()

    ref_p, ref_s = oracle_quant(x)
    assert ref_s.shape == (8, 1) and (ref_s.double() == 2.0 ** k).all()
    want = torch.from_numpy(vg.e4m3_rne(unit)).view(8, 128)
    assert torch.equal(ref_p.view(torch.uint8), want)
    assert len(np.unique(want.numpy())) == 254  # every code but the NaNs
    (pair,) = quant.quantize_fp8([x])
    assert_pair_matches(pair, x)


# ---------------------------------------------------------------------------
# dequantise
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("out_dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("scale", vg.DEQUANT_SCALES)
def test_dequant_all_codes(scale, out_dtype):
    from torchstore_amd.ops import quant

    payload = vg.all_codes_payload()
    assert payload.shape == (3, 128)
    assert np.unique(vg.bits_of_u8(payload)).size == 256
    scales = vg.scales_for(payload, scale)
    assert scales[0, 0].item() == scale  # the constant is exact in f32
    ref = vg.dequant_reference_bits(payload, scales, out_dtype)
    # the oracle (torch's narrowing) and the written-out reference agree
    vg.check_dequant(oracle_dequant(payload, scales, out_dtype), ref)
    out = torch.empty(3, 128, dtype=out_dtype)
    quant.dequantize_fp8_into([(payload, scales)], [out])
    vg.check_dequant(out, ref)
    assert torch.isnan(out.view(-1)[[0x7F, 0xFF, 256 + 0x7F]]).all()


def test_dequant_scales_cover_what_they_claim():
    payload = vg.all_codes_payload()
    s = vg.DEQUANT_SCALES
    assert s[1] == FLOOR_SCALE.item()

    def f16(scale):
        out = vg.from_bits(vg.dequant_reference_bits(
            payload, vg.scales_for(payload, scale), F16), F16)
        return out[~torch.isnan(out)]

    assert torch.isinf(f16(s[2])).sum() > 300  # all but the zeros
    sub = f16(s[3])
    assert ((sub != 0) & (sub.abs() < 2.0 ** -14)).sum() >= 250
    mild = f16(s[4])
    assert 0 < torch.isinf(mild).sum() < 40
    for scale in s:  # the sign of zero is in every one of them
        z = f16(scale)
        assert (vg.bits_of(z) == 0x8000).any() and (vg.bits_of(z) == 0).any()


@pytest.mark.parametrize("dtype,k", vg.TIE_CASES, ids=_ids)
def test_tie_grid_dequant(dtype, k):
    from torchstore_amd.ops import quant

    pair = oracle_quant(vg.e4m3_tie_grid(dtype, k))
    for out_dtype in DTYPES:
        ref = vg.dequant_reference_bits(*pair, out_dtype)
        vg.check_dequant(oracle_dequant(*pair, out_dtype), ref)
        out = torch.empty(8, 128, dtype=out_dtype)
        quant.dequantize_fp8_into([pair], [out])
        vg.check_dequant(out, ref)
        assert same_bytes(out, oracle_dequant(*pair, out_dtype))
        if k == 118 and out_dtype == F16:  # the recipe's IEEE overflow
            assert torch.equal(torch.isinf(out), pair[0].float() != 0)
        else:
            assert torch.isfinite(out).all()


# ---------------------------------------------------------------------------
# subnormal and zero blocks
# ---------------------------------------------------------------------------


def check_subnormal_pair(pair, dtype):
    """What a quantised ``subnormal_block(dtype)`` has to look like (also
    used on the GPU)."""
    x = vg.subnormal_block(dtype)
    payload = pair[0].cpu().view(torch.uint8).view(-1)
    scale = pair[1].cpu().view(-1)
    if dtype == F16:
        want = torch.tensor(127 * 2.0 ** -24) / torch.tensor(448.0)
        assert scale.item() == want.item()
        assert len(torch.unique(payload & 0x7F)) >= 32
        assert (payload & 0x7F).max() == 0x7E
    else:
        assert scale.item() == FLOOR_SCALE.item()
        assert ((payload & 0x7F) == 0).all()
    neg = torch.from_numpy(np.signbit(x.double().numpy())).view(-1)
    assert torch.equal((payload & 0x80) != 0, neg), "a sign was lost"


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_subnormal_block(dtype):
    from torchstore_amd.ops import quant

    x = vg.subnormal_block(dtype)
    assert x.shape == (1, 128) and x.dtype == dtype
    mag = np.sort(np.abs(x.double().numpy().reshape(-1)))
    assert np.array_equal(mag, np.arange(128) * vg.SUBNORMAL_STEP[dtype])
    assert np.signbit(x.double().numpy()).sum() == 64
    assert vg.bits_of(x)[0] == (0x80000000 if dtype == F32 else 0x8000)  # -0
    check_subnormal_pair(oracle_quant(x), dtype)
    (pair,) = quant.quantize_fp8([x])
    assert_pair_matches(pair, x)
    # the payload is what e4m3_rne makes of x / scale-of-the-block
    amax = max(127 * vg.SUBNORMAL_STEP[dtype], 2.0 ** -96)
    inv = np.float32(448.0) / np.float32(amax)
    q = x.float().numpy().reshape(-1) * inv  # one fp32 multiply each
    assert np.array_equal(vg.bits_of_u8(pair[0]), vg.e4m3_rne(q))


def check_zero_and_tiny_pair(pair):
    payload, scales = pair[0].cpu(), pair[1].cpu()
    assert payload[1, 128:256].view(torch.uint8).eq(0).all()
    assert scales[1, 1] == FLOOR_SCALE and scales[2, 0] == FLOOR_SCALE
    assert payload.float().abs().max() == 448.0
    # 2**-100 * (448 / 2**-96) = 28; f16 holds zeros there.  Element 5 is
    # the negative one either way.
    tiny = payload[2, 0:128].float()
    assert tiny.abs().eq(28.0).all() or tiny.eq(0).all()
    assert torch.equal(torch.signbit(tiny), torch.arange(128) == 5)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_zero_and_tiny_blocks(dtype):
    x = vg.zero_and_tiny_blocks(dtype)
    assert x.shape == (3, 384) and x.dtype == dtype
    assert x[1, 128:256].eq(0).all()
    if dtype != F16:
        assert x[2, 0:128].abs().eq(2.0 ** -100).all() and x[2, 5] < 0
    check_zero_and_tiny_pair(oracle_quant(x))
