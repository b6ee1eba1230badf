"""Tile-scaled FP8 kernels (K12/K13) on the GPU, byte for byte against the oracle of
``tests/test_quant_tile.py``, and the format through a GPU-resident store."""

import functools

import pytest
import torch

import torchstore_amd as ts
from tests.test_quant import make_input, same_bytes, signed_zero_input
from tests.test_quant_tile import (
    DTYPES, FLOOR_SCALE, SHAPES, assert_pair_matches, oracle_dequant,
    oracle_quant, zero_tile_input,
)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an AMD GPU")

# (1152, 1408) is 99 tiles: at a grid of 64 every workgroup takes several
GPU_SHAPES = SHAPES + [(256, 384), (1152, 1408)]
CANARY = 0x5A
GUARD = 256


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    monkeypatch.delenv("HIPSTORE_TILE_GRID", raising=False)


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _cases(dtype):
    """[(CPU input, its oracle pair, placed one element into its storage)]:
    each tensor as it is and flipped along either axis (the tile maximum
    moves between the first and last pass and lane group), one off a 16 B
    boundary, signed zeros and, last, an all-zero tile between two others."""
    xs = []
    for shape in GPU_SHAPES:
        x = make_input(shape, dtype)
        xs += [(x, False), (x.flip(-1).contiguous(), False)]
        if len(shape) > 1:
            xs.append((x.flip(-2).contiguous(), False))
    xs.append((make_input((130, 208), dtype), True))
    xs.append((signed_zero_input((130, 200), dtype), False))
    xs.append((signed_zero_input((130, 208), dtype), False))
    xs.append((zero_tile_input(dtype), False))
    return [(x, oracle_quant(x), shift) for x, shift in xs]


def _on_device(x, shift):
    if not shift:
        return x.to(_dev())
    base = torch.zeros(x.numel() + 1, dtype=x.dtype, device=_dev())
    base[1:] = x.to(_dev()).reshape(-1)
    shifted = base[1:].view(x.shape)
    assert shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
    return shifted


def _canaried(nbytes):  # (arena, its first nbytes): the rest holds the canary
    arena = torch.full((nbytes + GUARD,), CANARY, dtype=torch.uint8, device=_dev())
    return arena, arena[:nbytes]


def _intact(arena, nbytes):
    return bool(arena[nbytes:].eq(CANARY).all())


@requires_gpu
@pytest.mark.parametrize("grid", [None, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tile_quant_kernel_matches_oracle(dtype, grid, monkeypatch):
    """At the default grid cap a workgroup takes one tile; at 64 each takes
    several, of different tensors and paths, and alternates the LDS slots."""
    from torchstore_amd.ops import gpu, quant_tile

    if grid:
        monkeypatch.setenv("HIPSTORE_TILE_GRID", str(grid))
    cases = _cases(dtype)
    triples, arenas = [], []
    for x, _, shift in cases:
        x = _on_device(x, shift)
        sshape = quant_tile.tile_scales_shape(x.shape)
        ns = torch.Size(sshape).numel() * 4
        pa, pv = _canaried(x.numel())
        sa, sv = _canaried(ns)
        payload = pv.view(torch.float8_e4m3fn).view(x.shape)
        triples.append((x, payload, sv.view(torch.float32).view(sshape)))
        arenas.append((pa, x.numel(), sa, ns))
    before = gpu.tile_launches(), gpu.quant_launches(), gpu.row_launches()
    gpu.quant_tile_batch(triples, _dev())
    after = gpu.tile_launches(), gpu.quant_launches(), gpu.row_launches()
    assert after == (before[0] + 1, before[1], before[2])  # a counter of its own
    torch.cuda.synchronize()
    for (x, payload, scales), (_, ref, _), (pa, np_, sa, ns) in zip(triples, cases, arenas):
        assert same_bytes(payload, ref[0]), f"payload differs {tuple(x.shape)}"
        assert same_bytes(scales, ref[1]), f"scales differ {tuple(x.shape)}"
        assert _intact(pa, np_) and _intact(sa, ns), f"wrote past {tuple(x.shape)}"
    assert triples[-1][2][0, 1].cpu() == FLOOR_SCALE
    with pytest.raises(ValueError, match="contiguous"):
        gpu.quant_tile_batch([(triples[-1][0].t(),) + triples[-1][1:]], _dev())


@requires_gpu
@pytest.mark.parametrize("out_dtype", DTYPES)
def test_tile_dequant_kernel_matches_oracle(out_dtype):
    """One launch into canaried destinations; then a strided and an unaligned one."""
    from torchstore_amd.ops import gpu, quant_tile

    xs = [make_input(s, torch.float32) for s in GPU_SHAPES]
    pairs = [oracle_quant(x) for x in xs]
    es = torch.empty((), dtype=out_dtype).element_size()
    dev_pairs, outs, arenas = [], [], []
    for x, (p, s) in zip(xs, pairs):
        dev_pairs.append((p.to(_dev()), s.to(_dev())))
        arena, view = _canaried(x.numel() * es)
        outs.append(view.view(out_dtype).view(x.shape))
        arenas.append((arena, x.numel() * es))
    before = gpu.tile_launches()
    quant_tile.dequantize_fp8_tile_into(dev_pairs, outs)
    assert gpu.tile_launches() == before + 1
    torch.cuda.synchronize()
    for pair, out, (arena, nb) in zip(pairs, outs, arenas):
        assert same_bytes(out, oracle_dequant(*pair, out_dtype))
        assert _intact(arena, nb), "wrote past a destination"

    i = GPU_SHAPES.index((256, 384))
    wide = torch.zeros(256, 768, dtype=out_dtype, device=_dev())
    base = torch.zeros(256 * 384 + 1, dtype=out_dtype, device=_dev())
    strided, shifted = wide[:, ::2], base[1:].view(256, 384)
    quant_tile.dequantize_fp8_tile_into([dev_pairs[i]] * 2, [strided, shifted])
    torch.cuda.synchronize()
    for out in (strided, shifted):
        assert same_bytes(out, oracle_dequant(*pairs[i], out_dtype))
    assert wide[:, 1::2].eq(0).all() and base[0] == 0


@requires_gpu
async def test_tile_state_dict_through_gpu_store():
    def weights(seed):
        ws = [make_input((256, 384), torch.bfloat16, seed),
              make_input((2, 130, 200), torch.bfloat16, seed + 1)]
        return {"layers": [{"w": w.to(_dev())} for w in ws], "step": seed,
                "norm": make_input((384,), torch.bfloat16, seed + 2).to(_dev())}

    src, dest = weights(10), weights(0)
    ws = [layer["w"] for layer in src["layers"]]
    await ts.initialize(
        num_storage_volumes=1, strategy=ts.SingletonStrategy(), storage_device="auto"
    )
    try:
        await ts.put_state_dict(src, "ck", transfer_quant=ts.Fp8TileQuant(exclude=("*norm*",)))
        out = await ts.get_state_dict("ck", dest)
        raw = await ts.get_state_dict("ck", dequantize=False)
        torch.cuda.synchronize()
        for i, w in enumerate(ws):
            assert out["layers"][i]["w"] is dest["layers"][i]["w"]
            ref = oracle_dequant(*oracle_quant(w), torch.bfloat16)
            assert same_bytes(dest["layers"][i]["w"], ref)
            leaf = raw["layers"][i]["w"]
            assert isinstance(leaf, ts.TileQuantizedTensor)
            assert_pair_matches((leaf.payload, leaf.scales), w)
        assert same_bytes(dest["norm"], src["norm"]) and out["step"] == 10  # excluded
    finally:
        await ts.shutdown()
