"""Tile-scaled FP8 on CPU: ``ops.quant_tile`` against a float64 oracle written out
here, the round-trip bound, and ``transfer_quant="fp8_e4m3_tile"`` through a store."""

import pickle

import pytest
import torch

import torchstore_amd as ts
from tests.test_quant import make_input, same_bytes, signed_zero_input

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(1, 1), (127, 128), (128, 128), (129, 144), (130, 200), (200, 16),
          (3, 129, 130), (257,)]
FLOOR_SCALE = torch.tensor(2.0 ** -96) / torch.tensor(448.0)


def _tiles(shape):
    """(matrix view shape, [(mat, tile row, tile col, row slice, col slice)])."""
    rows, cols = (shape[-2] if len(shape) > 1 else 1), shape[-1]
    mats = torch.Size(shape).numel() // (rows * cols)
    return (mats, rows, cols), [
        (m, i, j, slice(128 * i, 128 * i + 128), slice(128 * j, 128 * j + 128))
        for m in range(mats)
        for i in range(-(-rows // 128))
        for j in range(-(-cols // 128))
    ]


def oracle_amax(x):
    """(per-tile amax [*lead, ntr, ntc], the same per element), in float64."""
    view, tiles = _tiles(x.shape)
    x3 = x.detach().cpu().to(torch.float64).reshape(view)
    lead = tuple(x.shape[:-2])  # none for 1-D: the scales are [1, ntc]
    per_tile = x3.new_zeros(view[0], -(-view[1] // 128), -(-view[2] // 128))
    per_elem = torch.zeros_like(x3)
    for m, i, j, rs, cs in tiles:
        per_tile[m, i, j] = max(x3[m, rs, cs].abs().max().item(), 2.0 ** -96)
        per_elem[m, rs, cs] = per_tile[m, i, j]
    return per_tile.reshape(lead + per_tile.shape[1:]), per_elem.reshape(x.shape)


def oracle_quant(x):
    """(payload e4m3fn of x.shape, scales f32 [*lead, ntr, ntc])."""
    per_tile, per_elem = (a.to(torch.float32) for a in oracle_amax(x))
    xf = x.detach().cpu().to(torch.float32)
    # tensor / tensor on purpose: one IEEE divide each, never x * (1 / 448)
    q = torch.clamp(xf * (torch.full_like(per_elem, 448.0) / per_elem), -448.0, 448.0)
    return q.to(torch.float8_e4m3fn), per_tile / torch.full_like(per_tile, 448.0)


def oracle_dequant(payload, scales, dtype):
    view, tiles = _tiles(payload.shape)
    s3 = scales.cpu().reshape(view[0], *scales.shape[-2:])
    per_elem = torch.zeros(view, dtype=torch.float32)
    for m, i, j, rs, cs in tiles:
        per_elem[m, rs, cs] = s3[m, i, j]
    return (payload.cpu().to(torch.float32) * per_elem.reshape(payload.shape)).to(dtype)


def assert_pair_matches(pair, x):
    payload, scales = pair
    ref_p, ref_s = oracle_quant(x)
    assert payload.dtype == torch.float8_e4m3fn and scales.dtype == torch.float32
    assert same_bytes(payload, ref_p), "payload differs from the oracle"
    assert same_bytes(scales, ref_s), "scales differ from the oracle"


def zero_tile_input(dtype):
    """(130, 384): the middle tile of the first tile row is all zero."""
    x = make_input((130, 384), dtype)
    x[:128, 128:256] = 0.0
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_tile_quant_matches_oracle_and_bound(shape, dtype):
    """The torch path against the oracle, and |dequant - x| <= 16 * scale +
    |x| * 2**-8 with the tile's scale (the bound of tests/test_quant.py)."""
    from torchstore_amd.ops import quant_tile

    x = make_input(shape, dtype)
    (pair,) = quant_tile.quantize_fp8_tile([x])
    assert_pair_matches(pair, x)
    assert tuple(pair[1].shape) == quant_tile.tile_scales_shape(shape)
    for out_dtype in DTYPES:
        out = torch.empty(shape, dtype=out_dtype)
        quant_tile.dequantize_fp8_tile_into([pair], [out])
        assert same_bytes(out, oracle_dequant(*pair, out_dtype))
    out = quant_tile.TileQuantizedTensor(*pair, dtype).dequantize()
    err = (out.double() - x.double()).abs()
    bound = oracle_amax(x)[1] / 448.0 * 16.0 + x.double().abs() * 2.0 ** -8
    assert (err <= bound).all(), f"worst ratio {(err / bound).max().item():.3f}"


def test_cpu_tiles_do_not_cross_leading_index():
    from torchstore_amd.ops import quant_tile

    m = make_input((129, 130), torch.float32)
    x = torch.stack([m, m * 2.0 ** 20, m * 2.0 ** 40])
    (pair,) = quant_tile.quantize_fp8_tile([x])
    assert_pair_matches(pair, x)
    scales = pair[1]
    assert scales.shape == (3, 2, 2)
    assert torch.equal(scales[1:], torch.stack([scales[0] * 2.0 ** 20, scales[0] * 2.0 ** 40]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_tile_zero_and_signed_zero_tiles(dtype):
    from torchstore_amd.ops import quant_tile

    z = zero_tile_input(dtype)
    z[:128:3, 128:256] = -0.0
    sz = signed_zero_input((130, 200), dtype)
    pairs = quant_tile.quantize_fp8_tile([z, sz])
    for pair, x in zip(pairs, (z, sz)):
        assert_pair_matches(pair, x)
        out = torch.empty(x.shape, dtype=dtype)
        quant_tile.dequantize_fp8_tile_into([pair], [out])
        assert same_bytes(out, oracle_dequant(*pair, dtype))
    payload, scales = pairs[0]
    assert scales[0, 0] > FLOOR_SCALE == scales[0, 1] < scales[0, 2]
    tile = payload[:128, 128:256].view(torch.uint8)
    assert tile[::3].eq(0x80).all() and tile[1::3].eq(0).all()  # signs kept


async def test_store_tile_quant_round_trip():
    ws = [make_input((130, 200), torch.bfloat16, seed=1),
          make_input((3, 5, 130), torch.float32, seed=2)]
    sd = {"layers": [{"w": w} for w in ws], "step": 17,
          "norm": make_input((200,), torch.float32, seed=3)}
    await ts.initialize(
        num_storage_volumes=1, strategy=ts.SingletonStrategy(), storage_device="cpu"
    )
    try:
        await ts.put_state_dict(sd, "ck", transfer_quant=ts.Fp8TileQuant(exclude=("*norm*",)))
        assert (await ts.get("ck/norm")).dtype == torch.float32  # excluded
        scales = await ts.get("ck/<FP8_TILE_SCALES>/layers.0.w")
        assert scales.shape == (2, 2) and scales.dtype == torch.float32
        out = await ts.get_state_dict("ck")
        assert same_bytes(out["norm"], sd["norm"]) and out["step"] == 17
        for got, w in zip(out["layers"], ws):
            assert same_bytes(got["w"], oracle_dequant(*oracle_quant(w), w.dtype))
        raw = await ts.get_state_dict("ck", dequantize=False)
        for got, w in zip(raw["layers"], ws):
            assert isinstance(got["w"], ts.TileQuantizedTensor)
            assert_pair_matches((got["w"].payload, got["w"].scales), w)

        leaf = ts.TileQuantizedTensor(
            torch.zeros(3, 5, 130, dtype=torch.float8_e4m3fn),
            torch.zeros(3, 1, 2), torch.float32,
        )
        w0 = torch.zeros(130, 200, dtype=torch.bfloat16)
        dest = {"layers": [{"w": w0}, {"w": leaf}], "norm": torch.zeros(200), "step": 0}
        got = await ts.get_state_dict("ck", dest)
        assert got["layers"][1]["w"] is leaf
        assert_pair_matches((leaf.payload, leaf.scales), ws[1])
        assert same_bytes(w0, oracle_dequant(*oracle_quant(ws[0]), torch.bfloat16))
        await ts.put_state_dict(sd, "ck2", transfer_quant="fp8_e4m3_tile")
        raw = await ts.get_state_dict("ck2", dequantize=False)
        assert isinstance(raw["norm"], ts.TileQuantizedTensor)  # nothing excluded
        assert raw["norm"].scales.shape == (1, 2)
        with pytest.raises(ValueError, match="fp8_e4m3_tile"):
            await ts.put_state_dict(sd, "ck", transfer_quant="fp8_tile")
    finally:
        await ts.shutdown()


def test_marker_tile_field_and_earlier_markers():
    from torchstore_amd.state_dict import QuantMapping

    m = {"a": ("a",)}
    tile = QuantMapping(m, tile={"a": torch.bfloat16})
    back = pickle.loads(pickle.dumps(tile))
    assert dict(back) == m and back.tile == {"a": torch.bfloat16}
    assert back.quant == {} and back.mx == {} and back.mx6 == {} and back.row == {}
    row = {"a": torch.float16}
    assert QuantMapping(m, row=row).__reduce__() == (QuantMapping, (m, {}, {}, {}, row))
    assert QuantMapping(m, row).__reduce__() == (QuantMapping, (m, row))
