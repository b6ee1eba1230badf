"""MXFP6 (``ops/mx6.py``) on the CPU against a float64 reference written
here from the format's definition, and ``transfer_quant="mxfp6_e2m3"``
through a CPU store."""

import pickle

import numpy as np
import pytest
import torch

import torchstore_amd as ts
from tests.test_quant import make_input, same_bytes
from torchstore_amd.ops import mx6

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(1, 1), (3, 32), (3, 33), (5, 200), (3, 5), (4, 7, 130), (257,)]
MAGS = np.array([m / 8 for m in range(16)] + [2 + m / 4 for m in range(8)]
                + [4 + m / 2 for m in range(8)])  # by code: 0, 0.125, ..., 7.5


def _blocked(x):
    """(rows, nblk, 32) float64 with +0 padding, and cols."""
    cols = x.shape[-1]
    x2d = x.reshape(-1, cols).double().numpy()
    nblk = -(-cols // 32)
    v = np.zeros((x2d.shape[0], nblk * 32))
    v[:, :cols] = x2d
    return v.reshape(x2d.shape[0], nblk, 32), cols


def _scale(code):
    """2**(code - 127) in float64; NaN for code 255."""
    return np.where(code == 255, np.nan, 2.0 ** (code.astype(np.float64) - 127))


def ref_quant(x):
    """(payload, scales) of the format's definition, evaluated in float64."""
    v, cols = _blocked(x)
    amax = np.abs(v).max(-1).astype(np.float32)
    code = np.maximum((amax.view(np.int32) >> 23) - 2, 0)
    d = np.abs(np.abs(v / _scale(code)[..., None])[..., None] - MAGS)
    lo, hi = d.argmin(-1), 31 - d[..., ::-1].argmin(-1)  # differ on a tie
    c6 = np.where(lo % 2 == 0, lo, hi) | (np.signbit(v) << 5)
    bits = (c6[..., None] >> np.arange(6)) & 1
    packed = np.packbits(
        bits.reshape(v.shape[0], -1).astype(np.uint8), axis=1, bitorder="little"
    )[:, : (3 * cols + 3) // 4]
    pshape, sshape = mx6.mx6_shapes(x.shape)
    scales = torch.from_numpy(code.astype(np.uint8)).reshape(sshape)
    return torch.from_numpy(packed.copy()).reshape(pshape), scales


def ref_dequant(payload, scales, shape, dtype):
    rows, nblk = scales.numel() // scales.shape[-1], scales.shape[-1]
    bits = np.unpackbits(
        payload.reshape(rows, -1).numpy(), axis=1, count=nblk * 192, bitorder="little"
    )
    c6 = (bits.reshape(rows, nblk, 32, 6) << np.arange(6)).sum(-1)
    q = np.where(c6 & 32, -1.0, 1.0) * MAGS[c6 & 31]
    with np.errstate(invalid="ignore"):
        y = q * _scale(scales.reshape(rows, nblk).numpy())[..., None]
    y = torch.from_numpy(y.reshape(rows, -1)[:, : shape[-1]].copy())
    return y.to(torch.float32).reshape(shape).to(dtype)  # exact, then one rne


def tie_block(dtype):
    """Rows of one block each at X = 1/8: every tie midpoint of e2m3 with
    both signs, the saturation band (7.5 X, 8 X) and both zeros."""
    mids = (MAGS[:-1] + MAGS[1:]) / 2
    vals = np.concatenate([mids, -mids, mids])[: 3 * 28].reshape(3, 28)
    head = np.tile([7.75, -7.875, 0.0, -0.0], (3, 1))  # 7.75 fixes the scale
    return torch.from_numpy(np.concatenate([head, vals], 1) / 8).to(dtype)


def assert_matches_ref(pair, x):
    want = ref_quant(x.cpu())
    assert same_bytes(pair[0], want[0]), "payload"
    assert same_bytes(pair[1], want[1]), "scales"


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_mx6_matches_reference_and_bound(dtype):
    xs = [make_input(s, dtype) for s in SHAPES] + [tie_block(dtype)]
    pairs = mx6.quantize_mxfp6(xs)
    for x, pair in zip(xs, pairs):
        assert_matches_ref(pair, x)
        for out_dtype in DTYPES:
            out = torch.empty(x.shape, dtype=out_dtype)
            mx6.dequantize_mxfp6_into([pair], [out])
            assert same_bytes(out, ref_dequant(*pair, x.shape, out_dtype))
        # round trip in the input's own dtype: X / 2 + |x| 2^-8 per element
        y = mx6.Mxfp6QuantizedTensor(*pair, x.shape, dtype).dequantize()
        v, cols = _blocked(x)
        bound = _scale(pair[1].reshape(v.shape[:2]).numpy())[..., None] / 2
        bound = bound + np.abs(v) * 2.0**-8
        err = np.abs(_blocked(y)[0] - v)
        assert (err <= bound).all(), float((err - bound).max())
    # y is the tie block's: 7.75 X and -7.875 X saturate to +-7.5 X, -0 stays
    assert y[0, :2].tolist() == [7.5 / 8, -7.5 / 8] and torch.signbit(y[0, 3])


def test_mx6_errors():
    x = make_input((4, 40), torch.bfloat16)
    (pair,) = mx6.quantize_mxfp6([x])
    with pytest.raises(ValueError, match="does not fit"):
        mx6.dequantize_mxfp6_into([pair], [torch.empty(4, 41)])
    with pytest.raises(TypeError):
        mx6.quantize_mxfp6([torch.zeros(4, 4, dtype=torch.int32)])
    with pytest.raises(ValueError, match="mxfp6_e2m3"):
        ts.state_dict._resolve_quant("mxfp6")


def test_marker_without_mx6_pickles_as_before():
    from torchstore_amd.state_dict import QuantMapping

    flat = {"a.w": ("a", "w")}
    mx = {"a.w": (torch.bfloat16, (3, 5))}
    for args in ((flat, {"a.w": torch.float16}), (flat, {}, mx)):  # as before
        assert QuantMapping(*args).__reduce__() == (QuantMapping, args)
    m = pickle.loads(pickle.dumps(QuantMapping(flat, mx6=mx)))
    assert m == flat and m.mx6 == mx and m.mx == {} and m.quant == {}


async def test_store_mx6_cpu():
    sd = {
        "layers": [
            {"w": make_input((12, 200), torch.bfloat16, seed=1)},
            {"w": make_input((3, 5, 131), torch.float32, seed=2)},
        ],
        "norm": make_input((200,), torch.float32, seed=3),
        "step": 17,
    }
    ws = [layer["w"] for layer in sd["layers"]]
    want = [ref_dequant(*ref_quant(w), w.shape, w.dtype) for w in ws]
    await ts.initialize(
        num_storage_volumes=1, strategy=ts.SingletonStrategy(), storage_device="cpu"
    )
    try:
        policy = ts.Mxfp6BlockQuant(exclude=("*norm*",))
        await ts.put_state_dict(sd, "ck", transfer_quant=policy)
        stored = await ts.get("ck/layers.0.w")
        assert stored.dtype == torch.uint8 and stored.shape == (12, 150)
        assert (await ts.get("ck/<MX6_SCALES>/layers.1.w")).shape == (3, 5, 5)
        out = await ts.get_state_dict("ck")
        assert same_bytes(out["norm"], sd["norm"]) and out["step"] == 17
        raw = await ts.get_state_dict("ck", dequantize=False)
        dest = {
            "layers": [{"w": torch.zeros_like(ws[0])}, {"w": None}],
            "norm": torch.zeros(200),
            "step": 0,
        }
        p, s = mx6.alloc_mx6([ws[1].shape], torch.device("cpu"))[0]
        leaf = ts.Mxfp6QuantizedTensor(p, s, ws[1].shape, torch.float32)
        dest["layers"][1]["w"] = leaf
        got = await ts.get_state_dict("ck", dest)
        assert got["layers"][1]["w"] is leaf and same_bytes(p, ref_quant(ws[1])[0])
        assert same_bytes(dest["layers"][0]["w"], want[0])
        for i in (0, 1):
            assert same_bytes(out["layers"][i]["w"], want[i])
            q = raw["layers"][i]["w"]
            assert isinstance(q, ts.Mxfp6QuantizedTensor) and q.shape == ws[i].shape
            assert_matches_ref((q.payload, q.scales), ws[i])
        dest["layers"][0]["w"] = torch.zeros(12, 201, dtype=torch.bfloat16)
        with pytest.raises(ValueError, match="MXFP6"):
            await ts.get_state_dict("ck", dest)
        with pytest.raises(ValueError, match="direct"):
            await ts.put_state_dict(sd, "ck", direct=True, transfer_quant="mxfp6_e2m3")
    finally:
        await ts.shutdown()
