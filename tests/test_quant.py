"""Block-scaled FP8 transfer format on CPU: ``ops.quant`` against an oracle
written out here, the round-trip error bound, and ``transfer_quant`` through
a CPU store.

The oracle is the recipe of the format, in plain torch, independent of
``torchstore_amd.ops.quant``.  ``tests/test_gpu_quant.py`` imports it from
here so both files check against the same thing.
"""

import pytest
import torch

import torchstore_amd as ts
from torchstore_amd.strategy import SingletonStrategy

BLOCK = 128
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(1, 1), (3, 128), (5, 200), (4, 7, 130), (257,)]


# ---------------------------------------------------------------------------
# oracle
# ---------------------------------------------------------------------------


def _blocks(x2d, nblk):
    rows, cols = x2d.shape
    padded = torch.zeros(rows, nblk * BLOCK, dtype=torch.float32)
    padded[:, :cols] = x2d
    return padded.reshape(rows, nblk, BLOCK)


def oracle_quant(x):
    """(payload e4m3fn of x.shape, scales f32 [*x.shape[:-1], nblk])."""
    x = x.detach().cpu()
    cols = x.shape[-1]
    nblk = -(-cols // BLOCK)
    xb = _blocks(x.reshape(-1, cols).to(torch.float32), nblk)
    amax = xb.abs().amax(dim=-1)
    amax = torch.maximum(amax, torch.full_like(amax, 2.0 ** -96))
    # tensor / tensor on purpose: one IEEE divide each, never x * (1 / 448)
    c448 = torch.full_like(amax, 448.0)
    scale = amax / c448
    inv = c448 / amax
    q = torch.clamp(xb * inv[:, :, None], -448.0, 448.0)
    q = q.reshape(-1, nblk * BLOCK)[:, :cols].reshape(x.shape)
    return q.to(torch.float8_e4m3fn), scale.reshape(*x.shape[:-1], nblk)


def oracle_dequant(payload, scales, dtype):
    payload, scales = payload.cpu(), scales.cpu()
    cols = payload.shape[-1]
    nblk = scales.shape[-1]
    qb = _blocks(payload.reshape(-1, cols).to(torch.float32), nblk)
    y = qb * scales.reshape(-1, nblk, 1)
    y = y.reshape(-1, nblk * BLOCK)[:, :cols].reshape(payload.shape)
    return y.to(dtype)


def make_input(shape, dtype, seed=0):
    """randn scaled columnwise by logspace(-3, 2): every block of a row sees
    another magnitude, and the data spans five decades."""
    g = torch.Generator().manual_seed(seed + 17 * len(shape) + shape[-1])
    x = torch.randn(shape, generator=g)
    return (x * torch.logspace(-3, 2, shape[-1])).to(dtype)


def signed_zero_input(shape, dtype):
    """-0.0 inputs, and values small enough to quantise to +-0: the sign of a
    zero has to survive the multiply on both sides of the format."""
    x = make_input(shape, torch.float32, seed=9)
    x[..., ::3] = -0.0
    x[..., 1::7] *= 1e-6
    return x.to(dtype)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(
        a.cpu().contiguous().reshape(-1).view(torch.uint8),
        b.cpu().contiguous().reshape(-1).view(torch.uint8),
    )


def assert_pair_matches(pair, x):
    payload, scales = pair
    ref_p, ref_s = oracle_quant(x)
    assert payload.dtype == torch.float8_e4m3fn and scales.dtype == torch.float32
    assert same_bytes(payload, ref_p), "payload differs from the oracle"
    assert scales.shape == ref_s.shape and torch.equal(scales.cpu(), ref_s)


# ---------------------------------------------------------------------------
# ops.quant on CPU
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_cpu_quant_matches_oracle(shape, dtype):
    from torchstore_amd.ops import quant

    x = make_input(shape, dtype)
    (pair,) = quant.quantize_fp8([x])
    assert_pair_matches(pair, x)
    payload, scales = pair
    assert payload.data_ptr() % 16 == 0 and scales.data_ptr() % 16 == 0
    assert not torch.isnan(payload.float()).any()
    for out_dtype in DTYPES:
        out = torch.empty(shape, dtype=out_dtype)
        quant.dequantize_fp8_into([pair], [out])
        assert same_bytes(out, oracle_dequant(payload, scales, out_dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_zero_and_tiny_blocks(dtype):
    """An all-zero block quantises to zeros with the floor scale; a block
    whose amax lies below 2**-96 is scaled by the floor, not by its amax."""
    from tests.value_grids import zero_and_tiny_blocks
    from torchstore_amd.ops import quant

    x = zero_and_tiny_blocks(dtype)
    (pair,) = quant.quantize_fp8([x])
    assert_pair_matches(pair, x)
    payload, scales = pair
    floor_scale = torch.tensor(2.0 ** -96) / torch.tensor(448.0)
    assert payload[1, 128:256].view(torch.uint8).eq(0).all()
    assert scales[1, 1] == floor_scale and scales[2, 0] == floor_scale
    assert payload.float().abs().max() == 448.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_signed_zeros(dtype):
    from torchstore_amd.ops import quant

    x = signed_zero_input((3, 200), dtype)
    (pair,) = quant.quantize_fp8([x])
    assert_pair_matches(pair, x)
    assert pair[0].view(torch.uint8).eq(0x80).any()  # -0 is in the payload
    for out_dtype in DTYPES:
        out = torch.empty(3, 200, dtype=out_dtype)
        quant.dequantize_fp8_into([pair], [out])
        assert same_bytes(out, oracle_dequant(*pair, out_dtype))


def test_cpu_quant_batch_and_layouts():
    """Several tensors per call, an empty one, a non-contiguous input and a
    non-contiguous output."""
    from torchstore_amd.ops import quant

    xs = [
        make_input((6, 130), torch.bfloat16),
        torch.empty(0, 4),
        make_input((130, 6), torch.float32).t(),
        make_input((300,), torch.float16),
    ]
    pairs = quant.quantize_fp8(xs)
    assert pairs[1][0].shape == (0, 4) and pairs[1][1].shape == (0, 1)
    for i in (0, 2, 3):
        assert_pair_matches(pairs[i], xs[i])
    wide = torch.zeros(6, 260, dtype=torch.bfloat16)
    out = wide[:, ::2]
    quant.dequantize_fp8_into([pairs[0]], [out])
    assert same_bytes(out, oracle_dequant(*pairs[0], torch.bfloat16))
    assert wide[:, 1::2].eq(0).all()
    with pytest.raises(TypeError):
        quant.quantize_fp8([torch.zeros(4, dtype=torch.int32)])
    with pytest.raises(ValueError):
        quant.dequantize_fp8_into([pairs[0]], [torch.zeros(6, 131)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_roundtrip_error_bound(shape, dtype):
    """|dequant - x| <= 16 * scale_of_block + |x| * 2**-8: half the step of
    e4m3's top binade, plus the rounding into the output dtype."""
    from torchstore_amd.ops import quant

    x = make_input(shape, dtype)
    (pair,) = quant.quantize_fp8([x])
    out = torch.empty(shape, dtype=dtype)
    quant.dequantize_fp8_into([pair], [out])
    cols = shape[-1]
    scale = pair[1].repeat_interleave(BLOCK, dim=-1)[..., :cols]
    err = (out.double() - x.double()).abs()
    bound = 16.0 * scale.double() + x.double().abs() * 2.0 ** -8
    assert (err <= bound).all(), f"worst ratio {(err / bound).max().item():.3f}"


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


def _state_dict():
    return {
        "model": {
            "layers": [
                {"w": make_input((12, 200), torch.bfloat16, seed=1)},
                {"w": make_input((3, 5, 130), torch.float32, seed=2)},
            ],
            "final_norm": make_input((200,), torch.float32, seed=3),
            "small": make_input((8,), torch.float16, seed=4),
            "ids": torch.arange(300, dtype=torch.int32),
            "temp": torch.tensor(0.75),
        },
        "step": 17,
        "tag": "run-a",
    }


_POLICY = ts.Fp8BlockQuant(min_numel=64, exclude=("*norm*",))
_QUANTISED = ("model.layers.0.w", "model.layers.1.w")


def _check_untouched(out, sd, norm_dtype=torch.float32):
    m, ref = out["model"], sd["model"]
    assert out["step"] == 17 and out["tag"] == "run-a"
    assert same_bytes(m["ids"], ref["ids"])
    assert same_bytes(m["temp"], ref["temp"])
    assert same_bytes(m["small"], ref["small"])
    assert same_bytes(m["final_norm"], ref["final_norm"].to(norm_dtype))


async def test_store_quant_allocating_get():
    async def body():
        sd = _state_dict()
        await ts.put_state_dict(sd, "ck", transfer_quant=_POLICY)
        # payload under the entry's own key as fp8, scales beside the marker
        stored = await ts.get("ck/model.layers.0.w")
        assert stored.dtype == torch.float8_e4m3fn
        assert stored.shape == (12, 200)
        assert (await ts.get("ck/model.final_norm")).dtype == torch.float32
        out = await ts.get_state_dict("ck")
        _check_untouched(out, sd)
        for i in (0, 1):
            x = sd["model"]["layers"][i]["w"]
            p, s = oracle_quant(x)
            got = out["model"]["layers"][i]["w"]
            assert same_bytes(got, oracle_dequant(p, s, x.dtype))

    await _with_store(body)


async def test_store_quant_inplace_get_and_transfer_dtype():
    async def body():
        sd = _state_dict()
        await ts.put_state_dict(
            sd, "ck", transfer_dtype=torch.bfloat16, transfer_quant=_POLICY
        )
        # transfer_dtype still governs the floating entries left alone
        assert (await ts.get("ck/model.final_norm")).dtype == torch.bfloat16
        assert (await ts.get("ck/model.small")).dtype == torch.bfloat16
        assert (await ts.get("ck/model.layers.1.w")).dtype == torch.float8_e4m3fn
        dest = {
            "model": {
                "layers": [
                    # the destination dtype governs the dequant
                    {"w": torch.zeros(12, 200, dtype=torch.float16)},
                    {"w": torch.zeros(3, 5, 130, dtype=torch.float32)},
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
        out = await ts.get_state_dict("ck", dest)
        assert out["model"]["layers"][0]["w"] is w0  # landed in place
        for i in (0, 1):
            p, s = oracle_quant(sd["model"]["layers"][i]["w"])
            d = dest["model"]["layers"][i]["w"]
            assert same_bytes(d, oracle_dequant(p, s, d.dtype))
        assert same_bytes(
            dest["model"]["final_norm"],
            sd["model"]["final_norm"].to(torch.bfloat16),
        )
        assert same_bytes(dest["model"]["ids"], sd["model"]["ids"])
        assert out["step"] == 17 and out["tag"] == "run-a"

    await _with_store(body)


async def test_store_quant_string_policy_quantises_every_float_tensor():
    async def body():
        sd = _state_dict()
        await ts.put_state_dict(sd, "ck", transfer_quant="fp8_e4m3")
        for k in ("model.final_norm", "model.small", *_QUANTISED):
            assert (await ts.get(f"ck/{k}")).dtype == torch.float8_e4m3fn
        # 0-dim and integer tensors never are
        assert (await ts.get("ck/model.temp")).dtype == torch.float32
        assert (await ts.get("ck/model.ids")).dtype == torch.int32
        out = await ts.get_state_dict("ck")
        assert same_bytes(out["model"]["temp"], sd["model"]["temp"])
        assert same_bytes(out["model"]["ids"], sd["model"]["ids"])
        p, s = oracle_quant(sd["model"]["small"])
        assert same_bytes(
            out["model"]["small"], oracle_dequant(p, s, torch.float16)
        )
        with pytest.raises(ValueError, match="transfer_quant"):
            await ts.put_state_dict(sd, "ck", transfer_quant="int4")

    await _with_store(body)


async def test_store_quant_raw_leaves():
    """dequantize=False hands out QuantizedTensor leaves; QuantizedTensor
    destinations are filled in place, without a dequant."""

    async def body():
        sd = _state_dict()
        await ts.put_state_dict(sd, "ck", transfer_quant=_POLICY)
        out = await ts.get_state_dict("ck", dequantize=False)
        _check_untouched(out, sd)
        for i in (0, 1):
            x = sd["model"]["layers"][i]["w"]
            leaf = out["model"]["layers"][i]["w"]
            assert isinstance(leaf, ts.QuantizedTensor)
            assert leaf.orig_dtype == x.dtype
            assert_pair_matches((leaf.payload, leaf.scales), x)
            p, s = oracle_quant(x)
            assert same_bytes(leaf.dequantize(), oracle_dequant(p, s, x.dtype))

        dest = _state_dict()
        leaves = []
        for i, shape in enumerate([(12, 200), (3, 5, 130)]):
            leaf = ts.QuantizedTensor(
                torch.zeros(shape, dtype=torch.float8_e4m3fn),
                torch.zeros(*shape[:-1], 2),
                torch.bfloat16,
            )
            dest["model"]["layers"][i]["w"] = leaf
            leaves.append(leaf)
        payload0 = leaves[0].payload
        got = await ts.get_state_dict("ck", dest)
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
            await ts.get_state_dict("ck", bad)

    await _with_store(body)


async def test_store_quant_strict_mismatch():
    async def body():
        await ts.put_state_dict(
            {"a": make_input((4, 130), torch.float32)}, "ck",
            transfer_quant="fp8_e4m3",
        )
        with pytest.raises(KeyError, match="mapping mismatch"):
            await ts.get_state_dict("ck", {"zz": torch.zeros(4, 130)})
        await ts.put_state_dict(
            {
                "a": make_input((4, 130), torch.float32),
                "b": make_input((4, 130), torch.float32),
            },
            "ck2",
            transfer_quant="fp8_e4m3",
        )
        with pytest.raises(KeyError, match="mapping mismatch"):
            await ts.get_state_dict("ck2", {"a": torch.zeros(4, 130)})
        # the reserved scales entries are not state_dict entries
        out = await ts.get_state_dict(
            "ck2", {"a": torch.zeros(4, 130)}, strict=False
        )
        assert out["a"].abs().sum() > 0

    await _with_store(body)


async def test_store_quant_overwrites():
    async def body():
        a = {"w": make_input((9, 200), torch.float32, seed=5)}
        b = {"w": make_input((9, 200), torch.float32, seed=6)}
        # quantised after plain
        await ts.put_state_dict(a, "ck")
        await ts.put_state_dict(b, "ck", transfer_quant="fp8_e4m3")
        p, s = oracle_quant(b["w"])
        expect = oracle_dequant(p, s, torch.float32)
        assert same_bytes((await ts.get_state_dict("ck"))["w"], expect)
        dest = {"w": torch.zeros(9, 200)}
        await ts.get_state_dict("ck", dest)
        assert same_bytes(dest["w"], expect)
        # plain after quantised
        await ts.put_state_dict(a, "ck")
        assert same_bytes((await ts.get_state_dict("ck"))["w"], a["w"])
        dest = {"w": torch.zeros(9, 200)}
        await ts.get_state_dict("ck", dest)
        assert same_bytes(dest["w"], a["w"])
        # and quantised again, with new values
        await ts.put_state_dict(a, "ck", transfer_quant="fp8_e4m3")
        p, s = oracle_quant(a["w"])
        assert same_bytes(
            (await ts.get_state_dict("ck"))["w"],
            oracle_dequant(p, s, torch.float32),
        )

    await _with_store(body)


async def test_direct_with_transfer_quant_raises():
    """Refused before anything is sent, so no store is needed."""
    from torchstore_amd.state_dict import put_state_dict

    with pytest.raises(ValueError, match="direct"):
        await put_state_dict(
            None, {"w": torch.zeros(4, 130)}, "ck",
            direct=True, transfer_quant="fp8_e4m3",
        )
