"""Row-scaled FP8 kernels (K10/K11) on the GPU, byte for byte against the
oracle of ``tests/test_quant_row.py`` (evaluated on the CPU), and
``transfer_quant="fp8_e4m3_row"`` through a GPU-resident store."""

import pytest
import torch

import torchstore_amd as ts
from tests.test_quant import make_input, same_bytes, signed_zero_input
from tests.test_quant_row import (
    FLOOR_SCALE, assert_pair_matches, oracle_dequant, oracle_quant,
)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an AMD GPU"
)

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
CANARY = 0x5A
GUARD = 256


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for knob in ("HIPSTORE_ROW_GRID", "HIPSTORE_ROW_WAVE", "HIPSTORE_ROW_WG"):
        monkeypatch.delenv(knob, raising=False)


def _dev():
    return torch.device("cuda", 0)


def _shapes():
    """The smallest shapes on each regime boundary from both sides, in fast
    and generic form; no row count is a multiple of the rows per unit."""
    from torchstore_amd.ops import gpu

    W, R = gpu.row_limits()
    return [(1, 1), (9, 16), (5, 200), (4, 7, 130), (257,), (5, W),
            (5, W + 16), (3, R), (3, R + 16), (2, 2 * R + 24)]


def _inputs(dtype):
    """Each tensor as it is (largest magnitudes in the last columns) and
    flipped (largest first), the last one also one element into its storage,
    then signed zeros and an all-zero row between two others."""
    from torchstore_amd.ops import gpu

    W, _ = gpu.row_limits()
    xs = []
    for shape in _shapes() + [(64, 1024)]:
        x = make_input(shape, dtype)
        xs += [x, x.flip(-1).contiguous()]
    xs = [x.to(_dev()) for x in xs]
    base = torch.zeros(64 * 1024 + 1, dtype=dtype, device=_dev())
    base[1:] = xs[-1].reshape(-1)
    shifted = base[1:].view(64, 1024)
    assert shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
    xs.append(shifted)
    xs += [signed_zero_input(s, dtype).to(_dev()) for s in [(3, 200), (3, W + 16)]]
    z = make_input((3, 4096), dtype).to(_dev())
    z[1] = 0.0
    return xs + [z]


def _canaried(nbytes):
    """(arena, view of its first nbytes): the rest holds the canary."""
    arena = torch.full((nbytes + GUARD,), CANARY, dtype=torch.uint8, device=_dev())
    return arena, arena[:nbytes]


def _intact(arena, nbytes):
    return bool(arena[nbytes:].eq(CANARY).all())


@requires_gpu
@pytest.mark.parametrize("grid", [None, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_row_quant_kernel_matches_oracle(dtype, grid, monkeypatch):
    """At the default grid cap a workgroup takes one unit; at 64 each takes
    several, in turn of different tensors and regimes, and alternates the
    two LDS slots."""
    from torchstore_amd.ops import gpu, quant_row

    if grid:
        monkeypatch.setenv("HIPSTORE_ROW_GRID", str(grid))
    xs = _inputs(dtype)
    triples, arenas = [], []
    for x in xs:
        sshape = quant_row.row_scales_shape(x.shape)
        ns = torch.Size(sshape).numel() * 4
        pa, pv = _canaried(x.numel())
        sa, sv = _canaried(ns)
        triples.append(
            (x, pv.view(torch.float8_e4m3fn).view(x.shape),
             sv.view(torch.float32).view(sshape))
        )
        arenas.append((pa, x.numel(), sa, ns))
    before, quant_before = gpu.row_launches(), gpu.quant_launches()
    gpu.quant_row_batch(triples, _dev())
    assert gpu.row_launches() == before + 1
    assert gpu.quant_launches() == quant_before  # a counter of its own
    torch.cuda.synchronize()
    for (x, payload, scales), (pa, np_, sa, ns) in zip(triples, arenas):
        assert_pair_matches((payload, scales), x)
        assert _intact(pa, np_), f"wrote past a payload {tuple(x.shape)}"
        assert _intact(sa, ns), f"wrote past the scales {tuple(x.shape)}"
    assert triples[-1][2][1, 0].cpu() == FLOOR_SCALE
    with pytest.raises(ValueError, match="contiguous"):
        gpu.quant_row_batch([(xs[2].t(), triples[2][1], triples[2][2])], _dev())


@requires_gpu
@pytest.mark.parametrize("out_dtype", DTYPES)
def test_row_dequant_kernel_matches_oracle(out_dtype):
    """One launch over every shape into canaried destinations; then a
    non-contiguous destination and an unaligned one."""
    from torchstore_amd.ops import gpu, quant_row

    xs = [make_input(s, torch.float32) for s in _shapes() + [(64, 1024)]]
    pairs = [oracle_quant(x) for x in xs]
    es = torch.empty((), dtype=out_dtype).element_size()
    dev_pairs, outs, arenas = [], [], []
    for x, (p, s) in zip(xs, pairs):
        dev_pairs.append((p.to(_dev()), s.to(_dev())))
        arena, view = _canaried(x.numel() * es)
        outs.append(view.view(out_dtype).view(x.shape))
        arenas.append((arena, x.numel() * es))
    before = gpu.row_launches()
    quant_row.dequantize_fp8_row_into(dev_pairs, outs)
    assert gpu.row_launches() == before + 1
    torch.cuda.synchronize()
    for pair, out, (arena, nb) in zip(pairs, outs, arenas):
        assert same_bytes(out, oracle_dequant(*pair, out_dtype))
        assert _intact(arena, nb), "wrote past a destination"

    wide = torch.zeros(64, 2048, dtype=out_dtype, device=_dev())
    base = torch.zeros(64 * 1024 + 1, dtype=out_dtype, device=_dev())
    strided, shifted = wide[:, ::2], base[1:].view(64, 1024)
    quant_row.dequantize_fp8_row_into([dev_pairs[-1]] * 2, [strided, shifted])
    torch.cuda.synchronize()
    for out in (strided, shifted):
        assert same_bytes(out, oracle_dequant(*pairs[-1], out_dtype))
    assert wide[:, 1::2].eq(0).all() and base[0] == 0


@requires_gpu
@pytest.mark.parametrize("out_dtype", DTYPES)
def test_row_dequant_all_bytes(out_dtype):
    """All 256 payload bytes as (1, 256) and (16, 16) under a tiny, a unit
    and a huge scale: NaN exactly at the two NaN codes (its payload is
    unspecified), every other byte as the oracle has it."""
    from torchstore_amd.ops import quant_row

    codes = torch.arange(256, dtype=torch.uint8)
    pairs = []
    for scale in (2.0 ** -96 / 448.0, 1.0, 2.0 ** 100):
        for shape in ((1, 256), (16, 16)):
            payload = codes.view(torch.float8_e4m3fn).view(shape)
            pairs.append((payload, torch.full((shape[0], 1), scale)))
    dev_pairs = [(p.to(_dev()), s.to(_dev())) for p, s in pairs]
    outs = [torch.empty(p.shape, dtype=out_dtype, device=_dev()) for p, _ in pairs]
    quant_row.dequantize_fp8_row_into(dev_pairs, outs)
    torch.cuda.synchronize()
    for pair, out in zip(pairs, outs):
        ref, got = oracle_dequant(*pair, out_dtype), out.cpu()
        nan = torch.isnan(ref)
        assert nan.reshape(-1).nonzero().reshape(-1).tolist() == [0x7F, 0xFF]
        assert torch.equal(torch.isnan(got), nan)
        assert same_bytes(got.masked_fill(nan, 0), ref.masked_fill(nan, 0))
    if out_dtype == torch.float16:
        assert torch.isinf(outs[4]).any()  # 2**100: IEEE overflow


@requires_gpu
async def test_row_state_dict_through_gpu_store():
    from torchstore_amd.ops import gpu

    W, _ = gpu.row_limits()

    def weights(seed):
        return {
            "layers": [
                {"w": make_input((256, 384), torch.bfloat16, seed).to(_dev())},
                {"w": make_input((6, W + 24), torch.bfloat16, seed + 1).to(_dev())},
            ],
            "norm": make_input((384,), torch.bfloat16, seed + 2).to(_dev()),
            "step": seed,
        }

    def expect(w):
        return oracle_dequant(*oracle_quant(w), torch.bfloat16)

    policy = ts.Fp8RowQuant(exclude=("*norm*",))
    await ts.initialize(
        num_storage_volumes=1, strategy=ts.SingletonStrategy(),
        storage_device="auto",
    )
    try:
        dest = weights(0)
        for t in (dest["layers"][0]["w"], dest["layers"][1]["w"], dest["norm"]):
            t.zero_()
        src = weights(10)
        for seed in (10, 20):
            if seed == 20:  # the second push sees the source mutated in place
                new = weights(20)
                for i in (0, 1):
                    src["layers"][i]["w"].copy_(new["layers"][i]["w"])
                src["norm"].copy_(new["norm"])
                src["step"] = 20
            await ts.put_state_dict(src, "ck", transfer_quant=policy)
            stored = await ts.get("ck/layers.0.w")
            assert same_bytes(stored, oracle_quant(src["layers"][0]["w"])[0])
            scales = await ts.get("ck/<FP8_ROW_SCALES>/layers.0.w")
            assert same_bytes(scales, oracle_quant(src["layers"][0]["w"])[1])
            out = await ts.get_state_dict("ck", dest)
            torch.cuda.synchronize()
            for i in (0, 1):
                assert out["layers"][i]["w"] is dest["layers"][i]["w"]
                assert same_bytes(
                    dest["layers"][i]["w"], expect(src["layers"][i]["w"])
                )
            assert same_bytes(dest["norm"], src["norm"])  # excluded: exact
            assert out["step"] == seed
    finally:
        await ts.shutdown()
