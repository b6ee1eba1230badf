"""Row-scaled FP8 transfer format on CPU: ``ops.quant_row`` against an oracle
written out here (``tests/test_gpu_quant_row.py`` shares it), the round-trip
bound, and ``transfer_quant="fp8_e4m3_row"`` through a CPU store."""

import pickle

import pytest
import torch

import torchstore_amd as ts
from tests.test_quant import make_input, same_bytes, signed_zero_input

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(1, 1), (3, 128), (5, 200), (4, 7, 130), (257,)]
FLOOR_SCALE = torch.tensor(2.0 ** -96) / torch.tensor(448.0)


def oracle_quant(x):
    """(payload e4m3fn of x.shape, scales f32 [*x.shape[:-1], 1])."""
    xf = x.detach().cpu().to(torch.float32)
    amax = xf.abs().amax(-1, keepdim=True)
    amax = torch.maximum(amax, torch.full_like(amax, 2.0 ** -96))
    # tensor / tensor on purpose: one IEEE divide each, never x * (1 / 448)
    c448 = torch.full_like(amax, 448.0)
    q = torch.clamp(xf * (c448 / amax), -448.0, 448.0)
    return q.to(torch.float8_e4m3fn), amax / c448


def oracle_dequant(payload, scales, dtype):
    return (payload.cpu().to(torch.float32) * scales.cpu()).to(dtype)


def assert_pair_matches(pair, x):
    payload, scales = pair
    ref_p, ref_s = oracle_quant(x)
    assert payload.dtype == torch.float8_e4m3fn and scales.dtype == torch.float32
    assert same_bytes(payload, ref_p), "payload differs from the oracle"
    assert same_bytes(scales, ref_s), "scales differ from the oracle"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_row_quant_matches_oracle_and_bound(shape, dtype):
    """The torch path against the oracle, and |dequant - x| <= 16 * scale +
    |x| * 2**-8: half the step of e4m3's top binade, plus the rounding into
    the output dtype."""
    from torchstore_amd.ops import quant_row

    x = make_input(shape, dtype)
    (pair,) = quant_row.quantize_fp8_row([x])
    assert_pair_matches(pair, x)
    assert tuple(pair[1].shape) == quant_row.row_scales_shape(shape)
    for out_dtype in DTYPES:
        out = torch.empty(shape, dtype=out_dtype)
        quant_row.dequantize_fp8_row_into([pair], [out])
        assert same_bytes(out, oracle_dequant(*pair, out_dtype))
    out = quant_row.RowQuantizedTensor(*pair, dtype).dequantize()
    err = (out.double() - x.double()).abs()
    bound = 16.0 * pair[1].double() + x.double().abs() * 2.0 ** -8
    assert (err <= bound).all(), f"worst ratio {(err / bound).max().item():.3f}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_row_zero_and_signed_zero_rows(dtype):
    from torchstore_amd.ops import quant_row

    x = signed_zero_input((3, 200), dtype)
    x[1] = 0.0
    x[1, ::3] = -0.0
    (pair,) = quant_row.quantize_fp8_row([x])
    assert_pair_matches(pair, x)
    payload, scales = pair
    assert scales[1, 0] == FLOOR_SCALE and scales[0, 0] > FLOOR_SCALE
    assert payload[1].view(torch.uint8)[::3].eq(0x80).all()
    assert payload[1].view(torch.uint8)[1::3].eq(0).all()
    out = torch.empty(3, 200, dtype=dtype)
    quant_row.dequantize_fp8_row_into([pair], [out])
    assert same_bytes(out, oracle_dequant(*pair, dtype))
    assert same_bytes(out[1], x[1])  # zeros keep their signs


async def test_store_row_quant_round_trip():
    sd = {
        "layers": [
            {"w": make_input((12, 200), torch.bfloat16, seed=1)},
            {"w": make_input((3, 5, 130), torch.float32, seed=2)},
        ],
        "norm": make_input((200,), torch.float32, seed=3),
        "step": 17,
    }
    ws = [layer["w"] for layer in sd["layers"]]
    await ts.initialize(
        num_storage_volumes=1, strategy=ts.SingletonStrategy(),
        storage_device="cpu",
    )
    try:
        await ts.put_state_dict(sd, "ck", transfer_quant=ts.Fp8RowQuant(exclude=("*norm*",)))
        assert (await ts.get("ck/norm")).dtype == torch.float32  # excluded
        scales = await ts.get("ck/<FP8_ROW_SCALES>/layers.0.w")
        assert scales.shape == (12, 1) and scales.dtype == torch.float32

        out = await ts.get_state_dict("ck")
        assert same_bytes(out["norm"], sd["norm"]) and out["step"] == 17
        for got, w in zip(out["layers"], ws):
            assert same_bytes(
                got["w"], oracle_dequant(*oracle_quant(w), w.dtype)
            )
        raw = await ts.get_state_dict("ck", dequantize=False)
        for got, w in zip(raw["layers"], ws):
            assert isinstance(got["w"], ts.RowQuantizedTensor)
            assert_pair_matches((got["w"].payload, got["w"].scales), w)

        leaf = ts.RowQuantizedTensor(
            torch.zeros(3, 5, 130, dtype=torch.float8_e4m3fn),
            torch.zeros(3, 5, 1),
            torch.float32,
        )
        dest = {
            "layers": [{"w": torch.zeros(12, 200, dtype=torch.float16)}, {"w": leaf}],
            "norm": torch.zeros(200),
            "step": 0,
        }
        got = await ts.get_state_dict("ck", dest)
        assert got["layers"][1]["w"] is leaf
        assert_pair_matches((leaf.payload, leaf.scales), ws[1])
        assert same_bytes(
            dest["layers"][0]["w"],
            oracle_dequant(*oracle_quant(ws[0]), torch.float16),
        )

        # a plain re-push afterwards: the marker decides, not the stale scales
        await ts.put_state_dict(sd, "ck")
        out = await ts.get_state_dict("ck")
        for got, w in zip(out["layers"], ws):
            assert same_bytes(got["w"], w)
        with pytest.raises(ValueError, match="fp8_e4m3_row"):
            await ts.put_state_dict(sd, "ck", transfer_quant="fp8_row")
    finally:
        await ts.shutdown()


def test_marker_row_field_survives_pickling():
    from torchstore_amd.state_dict import QuantMapping

    m = QuantMapping({"a": ("a",)}, row={"a": torch.bfloat16})
    back = pickle.loads(pickle.dumps(m))
    assert dict(back) == dict(m) and back.row == {"a": torch.bfloat16}
    assert back.quant == {} and back.mx == {} and back.mx6 == {}
