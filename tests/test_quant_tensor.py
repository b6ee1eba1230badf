"""Per-tensor FP8 on CPU: ``ops.quant_tensor`` against a float64 oracle written out
here, the round-trip bound, and ``transfer_quant="fp8_e4m3_tensor"`` through a store."""

import pickle

import pytest
import torch

import torchstore_amd as ts
from tests.test_quant import make_input, same_bytes, signed_zero_input

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(1, 1), (257,), (130, 200), (3, 129, 130), (2, 3, 16, 24)]
FLOOR_SCALE = torch.tensor(2.0 ** -96) / torch.tensor(448.0)


def _stack(x):
    """x as [mats, R * C] (a 1-D tensor is one matrix), and the scales shape."""
    lead = tuple(x.shape[:-2])
    return x.reshape(torch.Size(lead).numel(), -1), lead + (1, 1)


def oracle_amax(x):
    """Per-matrix amax with the floor, [mats, 1] in float64."""
    x2, _ = _stack(x.detach().cpu().to(torch.float64))
    return x2.abs().amax(dim=1, keepdim=True).clamp_min(2.0 ** -96)


def oracle_quant(x):
    """(payload e4m3fn of x.shape, scales f32 [*lead, 1, 1])."""
    amax = oracle_amax(x).to(torch.float32)
    x2, sshape = _stack(x.detach().cpu().to(torch.float32))
    top = torch.full_like(amax, 448.0)
    # tensor / tensor on purpose: one IEEE divide each, never x * (1 / 448)
    q = torch.clamp(x2 * (top / amax), -448.0, 448.0)
    return q.to(torch.float8_e4m3fn).reshape(x.shape), (amax / top).reshape(sshape)


def oracle_dequant(payload, scales, dtype):
    p2, _ = _stack(payload.cpu().to(torch.float32))
    return (p2 * scales.cpu().reshape(-1, 1)).reshape(payload.shape).to(dtype)


def assert_pair_matches(pair, x):
    payload, scales = pair
    ref_p, ref_s = oracle_quant(x)
    assert payload.dtype == torch.float8_e4m3fn and scales.dtype == torch.float32
    assert same_bytes(payload, ref_p), "payload differs from the oracle"
    assert same_bytes(scales, ref_s), "scales differ from the oracle"


def zero_matrix_input(dtype):
    """(3, 129, 130): the middle matrix is all zero, every third row of it -0."""
    x = make_input((3, 129, 130), dtype)
    x[1] = 0.0
    x[1, ::3] = -0.0
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_tensor_quant_matches_oracle_and_bound(shape, dtype):
    """The torch path against the oracle, and |dequant - x| <= 16 * scale +
    |x| * 2**-8 with the matrix's scale (the bound of tests/test_quant.py)."""
    from torchstore_amd.ops import quant_tensor

    x = make_input(shape, dtype)
    (pair,) = quant_tensor.quantize_fp8_tensor([x])
    assert_pair_matches(pair, x)
    assert tuple(pair[1].shape) == quant_tensor.tensor_scales_shape(shape)
    assert tuple(pair[1].shape) == tuple(shape[:-2]) + (1, 1)
    for out_dtype in DTYPES:
        out = torch.empty(shape, dtype=out_dtype)
        quant_tensor.dequantize_fp8_tensor_into([pair], [out])
        assert same_bytes(out, oracle_dequant(*pair, out_dtype))
    out = quant_tensor.TensorQuantizedTensor(*pair, dtype).dequantize()
    err, _ = _stack((out.double() - x.double()).abs())
    bound = oracle_amax(x) / 448.0 * 16.0 + _stack(x.double().abs())[0] * 2.0 ** -8
    assert (err <= bound).all(), f"worst ratio {(err / bound).max().item():.3f}"


def test_cpu_scales_do_not_leak_across_leading_index():
    from torchstore_amd.ops import quant_tensor

    m = make_input((129, 130), torch.float32)
    x = torch.stack([m, m * 2.0 ** 20, m * 2.0 ** 40])
    (pair,) = quant_tensor.quantize_fp8_tensor([x])
    assert_pair_matches(pair, x)
    scales = pair[1]
    assert scales.shape == (3, 1, 1)
    assert torch.equal(scales[1:], torch.stack([scales[0] * 2.0 ** 20, scales[0] * 2.0 ** 40]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_zero_matrix_and_signed_zeros(dtype):
    from torchstore_amd.ops import quant_tensor

    z = zero_matrix_input(dtype)
    sz = signed_zero_input((130, 200), dtype)
    pairs = quant_tensor.quantize_fp8_tensor([z, sz])
    for pair, x in zip(pairs, (z, sz)):
        assert_pair_matches(pair, x)
        out = torch.empty(x.shape, dtype=dtype)
        quant_tensor.dequantize_fp8_tensor_into([pair], [out])
        assert same_bytes(out, oracle_dequant(*pair, dtype))
    payload, scales = pairs[0]
    assert scales[0, 0, 0] > FLOOR_SCALE == scales[1, 0, 0] < scales[2, 0, 0]
    mid = payload[1].view(torch.uint8)
    assert mid[::3].eq(0x80).all() and mid[1::3].eq(0).all()  # signs kept


async def test_store_tensor_quant_round_trip():
    from torchstore_amd.state_dict import QuantMapping

    ws = [make_input((130, 200), torch.bfloat16, seed=1),
          make_input((3, 5, 130), torch.float32, seed=2)]
    sd = {"layers": [{"w": w} for w in ws], "step": 17,
          "norm": make_input((200,), torch.float32, seed=3)}
    await ts.initialize(
        num_storage_volumes=1, strategy=ts.SingletonStrategy(), storage_device="cpu"
    )
    try:
        await ts.put_state_dict(sd, "ck", transfer_quant=ts.Fp8TensorQuant(exclude=("*norm*",)))
        assert (await ts.get("ck/norm")).dtype == torch.float32  # excluded
        scales = await ts.get("ck/<FP8_TENSOR_SCALES>/layers.1.w")
        assert scales.shape == (3, 1, 1) and scales.dtype == torch.float32
        raw = await ts.get_state_dict("ck", dequantize=False)
        assert same_bytes(raw["norm"], sd["norm"]) and raw["step"] == 17
        for got, w in zip(raw["layers"], ws):
            assert isinstance(got["w"], ts.TensorQuantizedTensor)
            assert_pair_matches((got["w"].payload, got["w"].scales), w)

        w0 = torch.zeros(130, 200, dtype=torch.bfloat16)
        dest = {"layers": [{"w": w0}, {"w": torch.zeros(3, 5, 130)}],
                "norm": torch.zeros(200), "step": 0}
        got = await ts.get_state_dict("ck", dest)
        assert got["layers"][0]["w"] is w0
        assert same_bytes(w0, oracle_dequant(*oracle_quant(ws[0]), torch.bfloat16))
        assert same_bytes(dest["layers"][1]["w"], oracle_dequant(*oracle_quant(ws[1]), torch.float32))
        marker = await ts.get("ck/<MAPPING>")
        assert set(marker.whole) == {"layers.0.w", "layers.1.w"} and not marker.tile

        # markers of the earlier kinds are on the wire what they were
        await ts.put_state_dict(sd, "plain")
        assert type(await ts.get("plain/<MAPPING>")) is dict
        await ts.put_state_dict(sd, "tile", transfer_quant="fp8_e4m3_tile")
        tile = await ts.get("tile/<MAPPING>")
        assert tile.__reduce__() == (
            QuantMapping, (dict(tile), {}, {}, {}, {}, tile.tile))
        assert pickle.loads(pickle.dumps(marker)).whole == marker.whole
        with pytest.raises(ValueError, match="fp8_e4m3_tensor"):
            await ts.put_state_dict(sd, "ck", transfer_quant="fp8_tensor")
        with pytest.raises(ValueError, match="direct=True"):
            await ts.put_state_dict(sd, "ck", transfer_quant="fp8_e4m3_tensor", direct=True)
    finally:
        await ts.shutdown()
