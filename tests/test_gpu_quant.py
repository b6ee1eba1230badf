"""Block-scaled FP8 kernels on the GPU, byte for byte against the oracle of
``tests/test_quant.py`` (the recipe in plain torch, evaluated on the CPU),
and ``transfer_quant`` through a GPU-resident store."""

import pytest
import torch

import torchstore_amd as ts
from tests.test_quant import (
    assert_pair_matches,
    make_input,
    oracle_dequant,
    oracle_quant,
    same_bytes,
    signed_zero_input,
)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an AMD GPU"
)

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [
    (1, 1),
    (3, 128),
    (257,),
    (5, 200),  # rows 16 B aligned, cols % 16 != 0: generic path
    (4, 7, 130),
    (2, 4112),  # fast path with a short (16-element) last block
    (64, 1024),  # several waves, blocks and units
]
CANARY = 0x5A
GUARD = 256


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    monkeypatch.delenv("HIPSTORE_QUANT_GRID", raising=False)


def _dev():
    return torch.device("cuda", 0)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_quant_kernel_matches_oracle(dtype):
    from torchstore_amd.ops import gpu, quant

    xs = [make_input(s, dtype).to(_dev()) for s in SHAPES]
    # unaligned base: the same data one element into its storage
    base = torch.zeros(64 * 1024 + 1, dtype=dtype, device=_dev())
    base[1:] = xs[-1].reshape(-1)
    shifted = base[1:].view(64, 1024)
    assert shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
    zeros = [signed_zero_input(s, dtype).to(_dev()) for s in [(3, 200), (3, 256)]]
    for x in xs + [shifted] + zeros:
        before = gpu.quant_launches()
        (pair,) = quant.quantize_fp8([x])
        assert gpu.quant_launches() == before + 1
        torch.cuda.synchronize()
        assert pair[0].device == x.device and pair[0].data_ptr() % 16 == 0
        assert_pair_matches(pair, x)


@requires_gpu
def test_quant_batch_one_launch_and_canaries():
    """Four tensors of mixed dtype and shape plus an empty one in ONE launch,
    into buffers with a canary region behind every payload and scales."""
    from torchstore_amd.ops import gpu

    xs = [
        make_input((64, 1024), torch.bfloat16),
        make_input((5, 200), torch.float32),  # generic among fast ones
        make_input((2, 4112), torch.float16),
        make_input((257,), torch.bfloat16),
    ]
    xs = [x.to(_dev()) for x in xs]
    triples, arenas = [], []
    for x in xs:
        n = x.numel()
        nsc = x.numel() // x.shape[-1] * (-(-x.shape[-1] // 128))
        pa = torch.full((n + GUARD,), CANARY, dtype=torch.uint8, device=_dev())
        sa = torch.full(
            (nsc * 4 + GUARD,), CANARY, dtype=torch.uint8, device=_dev()
        )
        payload = pa[:n].view(torch.float8_e4m3fn).view(x.shape)
        scales = sa[: nsc * 4].view(torch.float32).view(*x.shape[:-1], -1)
        triples.append((x, payload, scales))
        arenas.append((pa, n, sa, nsc * 4))
    empty = torch.empty(0, 8, dtype=torch.bfloat16, device=_dev())
    triples.append(
        (
            empty,
            torch.empty(0, 8, dtype=torch.float8_e4m3fn, device=_dev()),
            torch.empty(0, 1, dtype=torch.float32, device=_dev()),
        )
    )
    before = gpu.quant_launches()
    gpu.quant_fp8_batch(triples, _dev())
    assert gpu.quant_launches() == before + 1
    torch.cuda.synchronize()
    for (x, payload, scales), (pa, n, sa, nb) in zip(triples, arenas):
        assert_pair_matches((payload, scales), x)
        assert pa[n:].eq(CANARY).all(), "wrote past a payload"
        assert sa[nb:].eq(CANARY).all(), "wrote past the scales"

    # the public entry point batches the same way
    from torchstore_amd.ops import quant

    before = gpu.quant_launches()
    pairs = quant.quantize_fp8(xs + [empty])
    assert gpu.quant_launches() == before + 1
    torch.cuda.synchronize()
    for pair, x in zip(pairs, xs):
        assert_pair_matches(pair, x)
    assert pairs[-1][0].shape == (0, 8) and pairs[-1][1].shape == (0, 1)


@requires_gpu
@pytest.mark.parametrize("out_dtype", DTYPES)
def test_dequant_kernel_matches_oracle(out_dtype):
    """One launch over every shape, into canaried destinations, plus a
    non-contiguous destination and an unaligned one."""
    from torchstore_amd.ops import gpu, quant

    pairs = [oracle_quant(make_input(s, torch.float32)) for s in SHAPES]
    pairs += [
        oracle_quant(signed_zero_input(s, torch.float32))
        for s in [(3, 200), (3, 256)]
    ]
    es = torch.empty((), dtype=out_dtype).element_size()
    dev_pairs, outs, arenas = [], [], []
    for p, s in pairs:
        dev_pairs.append((p.to(_dev()), s.to(_dev())))
        nb = p.numel() * es
        arena = torch.full((nb + GUARD,), CANARY, dtype=torch.uint8, device=_dev())
        outs.append(arena[:nb].view(out_dtype).view(p.shape))
        arenas.append((arena, nb))
    before = gpu.quant_launches()
    quant.dequantize_fp8_into(dev_pairs, outs)
    assert gpu.quant_launches() == before + 1
    torch.cuda.synchronize()
    for (p, s), out, (arena, nb) in zip(pairs, outs, arenas):
        assert same_bytes(out, oracle_dequant(p, s, out_dtype))
        assert arena[nb:].eq(CANARY).all(), "wrote past a destination"

    p, s = pairs[len(SHAPES) - 1]  # (64, 1024)
    wide = torch.zeros(64, 2048, dtype=out_dtype, device=_dev())
    strided = wide[:, ::2]
    base = torch.zeros(64 * 1024 + 1, dtype=out_dtype, device=_dev())
    shifted = base[1:].view(64, 1024)
    big = dev_pairs[len(SHAPES) - 1]
    quant.dequantize_fp8_into([big, big], [strided, shifted])
    torch.cuda.synchronize()
    ref = oracle_dequant(p, s, out_dtype)
    assert same_bytes(strided, ref) and same_bytes(shifted, ref)
    assert wide[:, 1::2].eq(0).all() and base[0] == 0


@requires_gpu
async def test_quantised_state_dict_through_gpu_store():
    def weights(seed):
        return {
            "layers": [
                {"w": make_input((256, 384), torch.bfloat16, seed).to(_dev())},
                {"w": make_input((256, 384), torch.bfloat16, seed + 1).to(_dev())},
            ],
            "norm": make_input((384,), torch.bfloat16, seed + 2).to(_dev()),
            "step": seed,
        }

    def expect(w):
        p, s = oracle_quant(w)
        return oracle_dequant(p, s, torch.bfloat16)

    policy = ts.Fp8BlockQuant(exclude=("*norm*",))
    await ts.initialize(
        num_storage_volumes=1,
        strategy=ts.SingletonStrategy(),
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
            assert stored.dtype == torch.float8_e4m3fn
            assert same_bytes(stored, oracle_quant(src["layers"][0]["w"])[0])
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
