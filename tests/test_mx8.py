"""MXFP8 (``ops/mx8.py``) on the CPU against a reference put together here
from the helpers of ``tests/value_grids.py`` and ``tests/mx_oracle.py``, and
``transfer_quant="mxfp8_e4m3"`` through a CPU store."""

import pickle

import numpy as np
import pytest
import torch

import torchstore_amd as ts
from tests.mx_oracle import scale_value
from tests.test_quant import make_input, same_bytes
from tests.value_grids import (
    _narrow_bits, _widen_bits, bits_of, bits_of_u8, check_dequant, e4m3_decode,
    e4m3_rne,
)
from torchstore_amd.ops import mx8

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(1, 1), (3, 32), (3, 33), (5, 200), (4, 7, 130), (257,)]
# one block at X = 1 (500 fixes code 127), by position: the band (464, 512)
# saturates, 464 is the tie that goes to 448, 17 / 19 are ties whose even
# neighbour lies below / above, both zeros, an e4m3 subnormal, a subnormal
# tie, half the smallest subnormal (a tie, to zero) and a quarter of it
TIE_VALUES = [500.0, -496.0, 480.0, 464.0, -464.0, 17.0, -17.0, 19.0, -19.0,
              0.0, -0.0, 3 * 2.0**-9, 5 * 2.0**-10, -(2.0**-10), 2.0**-11,
              -(2.0**-11)]
TIE_CODES = [0x7E, 0xFE, 0x7E, 0x7E, 0xFE, 0x58, 0xD8, 0x5A, 0xDA,
             0x00, 0x80, 0x03, 0x02, 0x80, 0x00, 0x80]


def tie_block(dtype):
    vals = torch.tensor(TIE_VALUES + [1.5] * 16, dtype=torch.float64)
    x = vals.to(dtype).view(1, 32)
    assert torch.equal(x.double().view(-1), vals)  # nothing was rounded
    return x


def inputs(dtype):
    """Every shape, the tie block, a row whose middle block is all zeros."""
    zeros = make_input((1, 96), dtype)
    zeros[0, 32:64] = 0.0
    return [make_input(s, dtype) for s in SHAPES] + [tie_block(dtype), zeros]


def _blocks_f32(x):
    """([rows, nblk, 32] float32 with +0 padding, cols) of a float tensor."""
    cols = x.shape[-1]
    x2d = _widen_bits(bits_of(x), x.dtype).view(np.float32).reshape(-1, cols)
    nblk = -(-cols // 32)
    padded = np.zeros((x2d.shape[0], nblk * 32), dtype=np.float32)
    padded[:, :cols] = x2d
    return padded.reshape(-1, nblk, 32), cols


def ref_quant(x):
    """(payload, scales): integer work on the bits, one numpy float32
    multiply, the float64 table search after the clamp."""
    xb, cols = _blocks_f32(x.detach().cpu())
    amax_bits = (xb.view(np.uint32) & 0x7FFFFFFF).max(axis=-1)
    code = np.maximum((amax_bits >> 23).astype(np.int64) - 8, 0)
    inv = ((254 - code).astype(np.uint32) << 23).view(np.float32)
    with np.errstate(under="ignore"):
        v = (xb * inv[:, :, None]).astype(np.float32)
    q = e4m3_rne(np.clip(v.astype(np.float64), -448.0, 448.0))
    q = q.reshape(xb.shape[0], -1)[:, :cols].copy()
    code = torch.from_numpy(code.astype(np.uint8))
    return (torch.from_numpy(q).view(torch.float8_e4m3fn).reshape(x.shape),
            code.reshape(mx8.mx8_scales_shape(x.shape)))


def ref_dequant_bits(payload, scales, dtype):
    """Table value times X as ONE numpy float32 multiply, narrowed."""
    cols = payload.shape[-1]
    q = e4m3_decode(bits_of_u8(payload).reshape(-1, cols)).astype(np.float32)
    s = scales.detach().cpu().contiguous().numpy().reshape(q.shape[0], -1)
    X = np.repeat(scale_value(s), 32, axis=1)[:, :cols]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        y = (q * X).astype(np.float32)
    return _narrow_bits(np.ascontiguousarray(y).reshape(-1).view(np.uint32), dtype)


def assert_pair_matches(pair, x):
    for got, want, what in zip(pair, ref_quant(x), ("payload", "scales")):
        assert same_bytes(got, want), f"{what} differs from the reference"


def assert_dequant_matches(out, pair):
    check_dequant(out, ref_dequant_bits(pair[0], pair[1], out.dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_mx8_matches_reference_and_bound(dtype):
    xs = inputs(dtype)
    pairs = mx8.quantize_mxfp8(xs)
    for x, pair in zip(xs, pairs):
        assert_pair_matches(pair, x)
        for out_dtype in DTYPES:
            out = torch.empty(x.shape, dtype=out_dtype)
            mx8.dequantize_mxfp8_into([pair], [out])
            assert_dequant_matches(out, pair)
        # round trip into bf16: |x| 2^-3 + X 2^-10 + |x| 2^-8 per element
        y = mx8.Mxfp8QuantizedTensor(*pair, dtype).dequantize(torch.bfloat16)
        v, _ = _blocks_f32(x)
        v = v.astype(np.float64)
        X = scale_value(pair[1].numpy().reshape(v.shape[:2])).astype(np.float64)
        bound = np.abs(v) * (2.0**-3 + 2.0**-8) + X[..., None] * 2.0**-10
        err = np.abs(_blocks_f32(y)[0] - v)
        assert (err <= bound).all(), float((err - bound).max())
    tie, zeros = pairs[-2], pairs[-1]
    assert tie[1].item() == 127
    assert bits_of_u8(tie[0])[: len(TIE_CODES)].tolist() == TIE_CODES
    assert zeros[1].view(-1)[1] == 0 and not bits_of_u8(zeros[0])[32:64].any()


def test_marker_without_mx8_pickles_as_before():
    from torchstore_amd.state_dict import QuantMapping

    flat = {"a.w": ("a", "w")}
    dt = {"a.w": torch.bfloat16}
    olds = [(flat, dt), (flat, {}, {}, {}, dt), (flat, {}, {}, {}, {}, {}, dt)]
    for args in olds:  # built the old way: the same arguments come back
        assert QuantMapping(*args).__reduce__() == (QuantMapping, args)
    m = pickle.loads(pickle.dumps(QuantMapping(flat, mx8=dt)))
    assert m == flat and m.mx8 == dt and m.quant == {} and m.whole == {}


async def test_store_mx8_cpu():
    ws = [make_input((12, 200), torch.bfloat16, seed=1),
          make_input((3, 5, 131), torch.float32, seed=2)]
    sd = {"layers": [{"w": w} for w in ws], "step": 17,
          "norm": make_input((200,), torch.float32, seed=3)}
    await ts.initialize(
        num_storage_volumes=1, strategy=ts.SingletonStrategy(), storage_device="cpu"
    )
    try:
        policy = ts.Mxfp8BlockQuant(exclude=("*norm*",))
        await ts.put_state_dict(sd, "ck", transfer_quant=policy)
        # dtype, shape and bytes of what the volume holds
        assert same_bytes(await ts.get("ck/layers.0.w"), ref_quant(ws[0])[0])
        stored = await ts.get("ck/<MX8_SCALES>/layers.1.w")
        assert same_bytes(stored, ref_quant(ws[1])[1])
        out = await ts.get_state_dict("ck")
        assert same_bytes(out["norm"], sd["norm"]) and out["step"] == 17
        raw = await ts.get_state_dict("ck", dequantize=False)
        p, s = mx8.alloc_mx8([ws[1].shape], torch.device("cpu"))[0]
        leaf = ts.Mxfp8QuantizedTensor(p, s, torch.float32)
        bf16 = torch.zeros(12, 200, dtype=torch.bfloat16)
        dest = {"layers": [{"w": bf16}, {"w": leaf}], "norm": torch.zeros(200),
                "step": 0}
        got = await ts.get_state_dict("ck", dest)
        assert got["layers"][1]["w"] is leaf
        assert_pair_matches((p, s), ws[1])
        assert_dequant_matches(bf16, ref_quant(ws[0]))
        for i in (0, 1):
            assert out["layers"][i]["w"].dtype == ws[i].dtype
            assert_dequant_matches(out["layers"][i]["w"], ref_quant(ws[i]))
            q = raw["layers"][i]["w"]
            assert isinstance(q, ts.Mxfp8QuantizedTensor) and q.shape == ws[i].shape
            assert_pair_matches((q.payload, q.scales), ws[i])
        with pytest.raises(ValueError, match="unknown transfer_quant"):
            await ts.put_state_dict(sd, "ck", transfer_quant="mxfp8_e5m2")
        with pytest.raises(ValueError, match="direct"):
            await ts.put_state_dict(sd, "ck", direct=True, transfer_quant="mxfp8_e4m3")
    finally:
        await ts.shutdown()
