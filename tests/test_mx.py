"""MXFP4 transfer format on CPU: ``ops.mx`` byte for byte against the oracle
of ``tests/mx_oracle.py``, the round-trip error bound, and
``transfer_quant="mxfp4"`` through a CPU store."""

from pathlib import Path

import numpy as np
import pytest
import torch

import torchstore_amd as ts
from tests import mx_oracle as oracle
from tests.mx_oracle import DEQUANT_CODES, SHAPES, TIE_CASES
from tests.test_quant import make_input, same_bytes, signed_zero_input
from tests.value_grids import check_dequant, subnormal_block
from torchstore_amd.strategy import SingletonStrategy

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
GOLDEN = Path(__file__).resolve().parent / "golden"


def assert_pair_matches(pair, x):
    payload, scales = pair
    ref_p, ref_s = oracle.oracle_quant(x)
    assert payload.dtype == torch.uint8 and scales.dtype == torch.uint8
    assert same_bytes(scales, ref_s), "scale codes differ from the oracle"
    assert same_bytes(payload, ref_p), "payload differs from the oracle"


def assert_dequant_matches(out, pair):
    check_dequant(out, oracle.dequant_bits(*pair, tuple(out.shape), out.dtype))


# ---------------------------------------------------------------------------
# ops.mx on CPU
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_mx_matches_oracle(shape, dtype):
    from torchstore_amd.ops import mx

    x = make_input(shape, dtype)
    (pair,) = mx.quantize_mxfp4([x])
    assert_pair_matches(pair, x)
    payload, scales = pair
    assert (tuple(payload.shape), tuple(scales.shape)) == mx.mx_shapes(shape)
    assert mx.mx_shapes(shape) == oracle.shapes_of(shape)
    assert payload.data_ptr() % 16 == 0 and scales.data_ptr() % 16 == 0
    assert scales.max() < 255
    for out_dtype in DTYPES:
        out = torch.empty(shape, dtype=out_dtype)
        mx.dequantize_mxfp4_into([pair], [out])
        assert_dequant_matches(out, pair)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_roundtrip_error_bound(shape, dtype):
    """|dequant - x| <= 2 * X + |x| * 2**-8: the larger of half the widest
    e2m1 step (4 to 6, so X) and the clipping error (below 8 X down to 6 X,
    so 2 X), plus the rounding into the output dtype."""
    from torchstore_amd.ops import mx

    x = make_input(shape, dtype)
    (pair,) = mx.quantize_mxfp4([x])
    out = torch.empty(shape, dtype=dtype)
    mx.dequantize_mxfp4_into([pair], [out])
    X = oracle.block_scale(pair[1], shape[-1])
    err = (out.double() - x.double()).abs()
    bound = 2.0 * X + x.double().abs() * 2.0 ** -8
    assert (err <= bound).all(), f"worst ratio {(err / bound).max().item():.3f}"


@pytest.mark.parametrize("dtype,k", TIE_CASES)
def test_cpu_tie_grid(dtype, k):
    from torchstore_amd.ops import mx

    x = oracle.e2m1_tie_grid(dtype, k)
    (pair,) = mx.quantize_mxfp4([x])
    assert_pair_matches(pair, x)
    payload, scales = pair
    assert scales.eq(max(k + 127, 0)).all()  # X = 2**k in every block
    assert (payload[:, 0] & 0xF).eq(7).all()  # 7 X saturates to 6 X
    # columns 1..7 of row 0 hold the midpoints in order; they round to the
    # even code, i.e. to 0 1 1 2 2 4 4 times X
    nib = torch.stack([payload & 0xF, payload >> 4], dim=-1).reshape(-1, 32)
    assert nib[0, 1:8].tolist() == [0, 2, 2, 4, 4, 6, 6]
    for out_dtype in DTYPES:
        out = torch.empty(x.shape, dtype=out_dtype)
        mx.dequantize_mxfp4_into([pair], [out])
        assert_dequant_matches(out, pair)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_subnormal_block_and_signed_zeros(dtype):
    """Blocks of subnormals take code 0 (X = 2**-127, itself a subnormal),
    and -0 survives both directions."""
    from torchstore_amd.ops import mx

    sub = subnormal_block(dtype)[:, :96].contiguous()  # three blocks
    zeros = signed_zero_input((3, 200), dtype)
    pairs = mx.quantize_mxfp4([sub, zeros])
    assert_pair_matches(pairs[0], sub)
    assert_pair_matches(pairs[1], zeros)
    if dtype != torch.float16:  # f16 subnormals are normal f32 numbers
        assert pairs[0][1].eq(0).all()
    nib = torch.stack([pairs[1][0] & 0xF, pairs[1][0] >> 4], dim=-1)
    assert nib.eq(8).any()  # -0 is in the payload
    for pair, x in zip(pairs, (sub, zeros)):
        for out_dtype in DTYPES:
            out = torch.empty(x.shape, dtype=out_dtype)
            mx.dequantize_mxfp4_into([pair], [out])
            assert_dequant_matches(out, pair)
    out = torch.empty(3, 200, dtype=dtype)
    mx.dequantize_mxfp4_into([pairs[1]], [out])
    was_neg_zero = (zeros == 0) & torch.signbit(zeros)
    assert (torch.signbit(out) & (out == 0))[was_neg_zero].all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_zero_block_and_short_last_block(dtype):
    from torchstore_amd.ops import mx

    x = make_input((3, 75), dtype)  # blocks of 32, 32 and 11; odd cols
    x[1, 32:64] = 0.0
    x[1, 40] = -0.0
    (pair,) = mx.quantize_mxfp4([x])
    assert_pair_matches(pair, x)
    payload, scales = pair
    assert payload.shape == (3, 38) and scales.shape == (3, 3)
    assert scales[1, 1] == 0
    assert payload[1, 16:32].tolist() == [0] * 4 + [0x08] + [0] * 11
    assert (payload[:, 37] >> 4).eq(0).all()  # odd cols: high nibble is 0


@pytest.mark.parametrize("out_dtype", DTYPES)
def test_cpu_dequant_all_bytes(out_dtype):
    """All 256 payload bytes under scale codes that reach f16 subnormals,
    f16 overflow, inf in f32 and the NaN code."""
    from torchstore_amd.ops import mx

    payload, shape = oracle.all_bytes_payload()
    for code in DEQUANT_CODES:
        scales = oracle.scales_for(shape, code)
        out = torch.empty(shape, dtype=out_dtype)
        mx.dequantize_mxfp4_into([(payload, scales)], [out])
        assert_dequant_matches(out, (payload, scales))
        if code == 255:
            assert torch.isnan(out).all()
        if code == 254:  # 2 X and more overflow, also in f32
            assert torch.isinf(out.float()).any() and not torch.isnan(out).any()
        # a zero keeps the sign of its nibble whatever the finite scale:
        # byte 0x08 is element 16 (-0) and 17 (+0) of row 0
        if code != 255:
            assert out[0, 16] == 0 and torch.signbit(out[0, 16])
            assert out[0, 17] == 0 and not torch.signbit(out[0, 17])


def test_cpu_mx_batch_and_layouts():
    """Several tensors per call, an empty one, a non-contiguous input and a
    non-contiguous output; the error cases."""
    from torchstore_amd.ops import mx

    xs = [
        make_input((6, 130), torch.bfloat16),
        torch.empty(0, 5),
        make_input((130, 6), torch.float32).t(),
        make_input((301,), torch.float16),
    ]
    pairs = mx.quantize_mxfp4(xs)
    assert pairs[1][0].shape == (0, 3) and pairs[1][1].shape == (0, 1)
    for i in (0, 2, 3):
        assert_pair_matches(pairs[i], xs[i])
    wide = torch.zeros(6, 260, dtype=torch.bfloat16)
    out = wide[:, ::2]
    mx.dequantize_mxfp4_into([pairs[0], pairs[1]], [out, torch.empty(0, 5)])
    assert_dequant_matches(out, pairs[0])
    assert wide[:, 1::2].eq(0).all()
    leaf = mx.MxQuantizedTensor(*pairs[3], (301,), torch.float16)
    assert leaf.shape == (301,)
    assert_dequant_matches(leaf.dequantize(), pairs[3])
    assert leaf.dequantize(torch.float32).dtype == torch.float32
    with pytest.raises(TypeError):
        mx.quantize_mxfp4([torch.zeros(4, dtype=torch.int32)])
    with pytest.raises(ValueError):
        mx.quantize_mxfp4([torch.tensor(1.0)])
    with pytest.raises(ValueError):  # 131 columns need 66 payload bytes
        mx.dequantize_mxfp4_into([pairs[0]], [torch.zeros(6, 131)])
    with pytest.raises(ValueError):  # same payload shape, one block more
        mx.dequantize_mxfp4_into(
            [(torch.zeros(2, 32, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.uint8))],
            [torch.zeros(2, 65)],
        )
    with pytest.raises(TypeError):
        mx.dequantize_mxfp4_into(
            [(pairs[0][0].view(torch.int8), pairs[0][1])], [torch.zeros(6, 130)]
        )
    with pytest.raises(ValueError):
        mx.dequantize_mxfp4_into([pairs[0]], [])
    with pytest.raises(ValueError):
        mx.mx_shapes(())


def test_alloc_quantized_is_unchanged():
    """The slab carving that ``ops.mx`` shares returns what it always did."""
    from torchstore_amd.ops import quant

    bufs = quant.alloc_quantized([(3, 200), (0, 4), (257,)], torch.device("cpu"))
    assert [tuple(p.shape) for p, _ in bufs] == [(3, 200), (0, 4), (257,)]
    assert [tuple(s.shape) for _, s in bufs] == [(3, 2), (0, 1), (3,)]
    (p0, s0), _, (p2, s2) = bufs
    assert p0.dtype == torch.float8_e4m3fn and s0.dtype == torch.float32
    base = p0.data_ptr()
    # 600 B, 24 B, 257 B and 12 B pieces of one slab, 256 B apart at least
    assert [t.data_ptr() - base for t in (s0, p2, s2)] == [768, 1024, 1536]


# ---------------------------------------------------------------------------
# the commit marker on the wire
# ---------------------------------------------------------------------------


def _marker_mapping():
    return {
        "model.layers.0.w": ("model", "layers", 0, "w"),
        "model.norm": ("model", "norm"),
        "step": ("step",),
    }


def test_fp8_marker_pickles_as_before():
    """The marker of an FP8 push serialises to the bytes recorded before the
    ``mx`` field existed (tests/golden/fp8_marker_pickle.bin)."""
    from torchstore_amd.runtime import serde
    from torchstore_amd.state_dict import QuantMapping

    marker = QuantMapping(_marker_mapping(), {"model.layers.0.w": torch.bfloat16})
    header, buffers = serde.dumps(marker)
    assert not buffers
    assert header == (GOLDEN / "fp8_marker_pickle.bin").read_bytes()
    back = serde.loads(header, [])
    assert back == _marker_mapping() and back.mx == {}
    assert back.quant == {"model.layers.0.w": torch.bfloat16}


def test_mx_marker_roundtrip():
    from torchstore_amd.runtime import serde
    from torchstore_amd.state_dict import QuantMapping

    mx = {"model.layers.0.w": (torch.bfloat16, (12, 201))}
    header, _ = serde.dumps(QuantMapping(_marker_mapping(), mx=mx))
    back = serde.loads(header, [])
    assert isinstance(back, QuantMapping) and back == _marker_mapping()
    assert back.mx == mx and back.quant == {}


# ---------------------------------------------------------------------------
# through a CPU store
# ---------------------------------------------------------------------------


async def _with_store(body):
    await ts.initialize(
        num_storage_volumes=1,
        strategy=SingletonStrategy(),
        storage_device="cpu",
    )
    try:
        await body()
    finally:
        await ts.shutdown()


_SHAPES = [(12, 200), (3, 5, 131)]  # the second has odd rows


def _state_dict():
    return {
        "model": {
            "layers": [
                {"w": make_input(_SHAPES[0], torch.bfloat16, seed=1)},
                {"w": make_input(_SHAPES[1], torch.float32, seed=2)},
            ],
            "final_norm": make_input((200,), torch.float32, seed=3),
            "small": make_input((8,), torch.float16, seed=4),
            "ids": torch.arange(300, dtype=torch.int32),
            "temp": torch.tensor(0.75),
        },
        "step": 17,
        "tag": "run-a",
    }


_POLICY = ts.Mxfp4BlockQuant(min_numel=64, exclude=("*norm*",))


def _expect(x, dtype=None):
    p, s = oracle.oracle_quant(x)
    return oracle.oracle_dequant(p, s, tuple(x.shape), dtype or x.dtype)


def _check_untouched(out, sd, norm_dtype=torch.float32):
    m, ref = out["model"], sd["model"]
    assert out["step"] == 17 and out["tag"] == "run-a"
    assert same_bytes(m["ids"], ref["ids"])
    assert same_bytes(m["temp"], ref["temp"])
    assert same_bytes(m["small"], ref["small"])
    assert same_bytes(m["final_norm"], ref["final_norm"].to(norm_dtype))


async def _store_mx_allocating_get_and_stored_bytes(ck):
    async def body():
        sd = _state_dict()
        await ts.put_state_dict(sd, ck, transfer_quant=_POLICY)
        for i, shape in enumerate(_SHAPES):
            rows, cols = int(np.prod(shape[:-1])), shape[-1]
            payload = await ts.get(f"{ck}/model.layers.{i}.w")
            scales = await ts.get(f"{ck}/<MX_SCALES>/model.layers.{i}.w")
            assert payload.dtype == torch.uint8 and scales.dtype == torch.uint8
            assert (tuple(payload.shape), tuple(scales.shape)) == oracle.shapes_of(shape)
            stored = payload.numel() + scales.numel()
            assert stored == rows * (-(-cols // 2) + -(-cols // 32))
            assert_pair_matches((payload, scales), sd["model"]["layers"][i]["w"])
        assert (await ts.get(f"{ck}/model.final_norm")).dtype == torch.float32
        out = await ts.get_state_dict(ck)
        _check_untouched(out, sd)
        for i in (0, 1):
            x = sd["model"]["layers"][i]["w"]
            got = out["model"]["layers"][i]["w"]
            assert got.shape == x.shape
            assert same_bytes(got, _expect(x))

    await body()


async def _store_mx_inplace_get_and_transfer_dtype(ck):
    async def body():
        sd = _state_dict()
        await ts.put_state_dict(
            sd, ck, transfer_dtype=torch.bfloat16, transfer_quant=_POLICY
        )
        # transfer_dtype still governs the floating entries left alone
        assert (await ts.get(f"{ck}/model.final_norm")).dtype == torch.bfloat16
        assert (await ts.get(f"{ck}/model.small")).dtype == torch.bfloat16
        assert (await ts.get(f"{ck}/model.layers.1.w")).dtype == torch.uint8
        dest = {
            "model": {
                "layers": [
                    # the destination dtype governs the dequant
                    {"w": torch.zeros(_SHAPES[0], dtype=torch.float16)},
                    {"w": torch.zeros(_SHAPES[1], dtype=torch.float32)},
                ],
                "final_norm": torch.zeros(200, dtype=torch.bfloat16),
                "small": torch.zeros(8, dtype=torch.bfloat16),
                "ids": torch.zeros(300, dtype=torch.int32),
                "temp": torch.zeros((), dtype=torch.bfloat16),
            },
            "step": 0,
            "tag": "",
        }
        w0 = dest["model"]["layers"][0]["w"]
        out = await ts.get_state_dict(ck, dest)
        assert out["model"]["layers"][0]["w"] is w0  # landed in place
        for i in (0, 1):
            d = dest["model"]["layers"][i]["w"]
            assert same_bytes(d, _expect(sd["model"]["layers"][i]["w"], d.dtype))
        assert same_bytes(
            dest["model"]["final_norm"],
            sd["model"]["final_norm"].to(torch.bfloat16),
        )
        assert same_bytes(dest["model"]["ids"], sd["model"]["ids"])
        assert out["step"] == 17 and out["tag"] == "run-a"

    await body()


async def _store_mx_string_policy_quantises_every_float_tensor(ck):
    async def body():
        sd = _state_dict()
        await ts.put_state_dict(sd, ck, transfer_quant="mxfp4")
        for k in ("model.final_norm", "model.small", "model.layers.0.w"):
            assert (await ts.get(f"{ck}/{k}")).dtype == torch.uint8
        assert (await ts.get(f"{ck}/model.small")).shape == (4,)
        # 0-dim and integer tensors never are
        assert (await ts.get(f"{ck}/model.temp")).dtype == torch.float32
        assert (await ts.get(f"{ck}/model.ids")).dtype == torch.int32
        out = await ts.get_state_dict(ck)
        assert same_bytes(out["model"]["temp"], sd["model"]["temp"])
        assert same_bytes(out["model"]["ids"], sd["model"]["ids"])
        assert same_bytes(out["model"]["small"], _expect(sd["model"]["small"]))

    await body()


async def _store_mx_raw_leaves(ck):
    """dequantize=False hands out MxQuantizedTensor leaves; such
    destinations are filled in place, without a dequant."""

    async def body():
        sd = _state_dict()
        await ts.put_state_dict(sd, ck, transfer_quant=_POLICY)
        out = await ts.get_state_dict(ck, dequantize=False)
        _check_untouched(out, sd)
        for i in (0, 1):
            x = sd["model"]["layers"][i]["w"]
            leaf = out["model"]["layers"][i]["w"]
            assert isinstance(leaf, ts.MxQuantizedTensor)
            assert leaf.orig_dtype == x.dtype and leaf.shape == x.shape
            assert_pair_matches((leaf.payload, leaf.scales), x)
            assert same_bytes(leaf.dequantize(), _expect(x))

        dest = _state_dict()
        leaves = []
        for i, shape in enumerate(_SHAPES):
            pshape, sshape = oracle.shapes_of(shape)
            leaf = ts.MxQuantizedTensor(
                torch.zeros(pshape, dtype=torch.uint8),
                torch.zeros(sshape, dtype=torch.uint8),
                shape,
                torch.bfloat16,
            )
            dest["model"]["layers"][i]["w"] = leaf
            leaves.append(leaf)
        payload0 = leaves[0].payload
        got = await ts.get_state_dict(ck, dest)
        for i in (0, 1):
            assert got["model"]["layers"][i]["w"] is leaves[i]
            assert_pair_matches(
                (leaves[i].payload, leaves[i].scales),
                sd["model"]["layers"][i]["w"],
            )
        assert leaves[0].payload is payload0

        bad = _state_dict()
        bad["model"]["layers"][0]["w"] = torch.zeros(12, 200, dtype=torch.int32)
        with pytest.raises(TypeError, match="pushed quantised"):
            await ts.get_state_dict(ck, bad)
        # an FP8 leaf is no destination for an MXFP4 entry
        bad["model"]["layers"][0]["w"] = ts.QuantizedTensor(
            torch.zeros(12, 200, dtype=torch.float8_e4m3fn),
            torch.zeros(12, 2),
            torch.bfloat16,
        )
        with pytest.raises(TypeError, match="pushed quantised"):
            await ts.get_state_dict(ck, bad)
        # 130 and 131 columns pack into the same payload shape
        bad = _state_dict()
        bad["model"]["layers"][1]["w"] = torch.zeros(3, 5, 132)
        with pytest.raises(ValueError, match="shape"):
            await ts.get_state_dict(ck, bad)

    await body()


async def _store_mx_strict_mismatch(ck):
    async def body():
        await ts.put_state_dict(
            {"a": make_input((4, 130), torch.float32)}, ck,
            transfer_quant="mxfp4",
        )
        with pytest.raises(KeyError, match="mapping mismatch"):
            await ts.get_state_dict(ck, {"zz": torch.zeros(4, 130)})
        await ts.put_state_dict(
            {
                "a": make_input((4, 130), torch.float32),
                "b": make_input((4, 130), torch.float32),
            },
            ck + "2",
            transfer_quant="mxfp4",
        )
        with pytest.raises(KeyError, match="mapping mismatch"):
            await ts.get_state_dict(ck + "2", {"a": torch.zeros(4, 130)})
        # the reserved scales entries are not state_dict entries
        out = await ts.get_state_dict(
            ck + "2", {"a": torch.zeros(4, 130)}, strict=False
        )
        assert out["a"].abs().sum() > 0

    await body()


async def _store_mx_overwrites(ck):
    """Every order between plain, FP8 and MXFP4 pushes under one key."""
    from tests.test_quant import oracle_dequant as fp8_dequant
    from tests.test_quant import oracle_quant as fp8_quant

    async def body():
        def expect(w, mode):
            if mode is None:
                return w
            if mode == "mxfp4":
                return _expect(w)
            p, s = fp8_quant(w)
            return fp8_dequant(p, s, torch.float32)

        # every ordered pair of the three modes occurs as a transition
        order = [None, "mxfp4", "fp8_e4m3", "mxfp4", None, "fp8_e4m3", None]
        for n, mode in enumerate(order):
            w = make_input((9, 201), torch.float32, seed=5 + n)
            await ts.put_state_dict({"w": w}, ck, transfer_quant=mode)
            want = expect(w, mode)
            assert same_bytes((await ts.get_state_dict(ck))["w"], want)
            dest = {"w": torch.zeros(9, 201)}
            await ts.get_state_dict(ck, dest)
            assert same_bytes(dest["w"], want)

    await body()


async def test_store_mx():
    """One CPU store for all the scenarios above (starting a store costs far
    more than any of them), each under a key of its own."""

    async def body():
        for n, scenario in enumerate((
            _store_mx_allocating_get_and_stored_bytes,
            _store_mx_inplace_get_and_transfer_dtype,
            _store_mx_string_policy_quantises_every_float_tensor,
            _store_mx_raw_leaves,
            _store_mx_strict_mismatch,
            _store_mx_overwrites,
        )):
            await scenario(f"ck{n}")

    await _with_store(body)


async def test_direct_with_mxfp4_raises():
    """Refused before anything is sent, so no store is needed."""
    from torchstore_amd.state_dict import put_state_dict

    for policy in ("mxfp4", ts.Mxfp4BlockQuant()):
        with pytest.raises(ValueError, match="direct"):
            await put_state_dict(
                None, {"w": torch.zeros(4, 130)}, "ck",
                direct=True, transfer_quant=policy,
            )
