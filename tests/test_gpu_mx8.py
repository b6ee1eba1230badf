"""MXFP8 kernels (K16/K17) on the GPU, byte for byte against the reference of
``tests/test_mx8.py`` (evaluated on the CPU) and the torch implementation, and
``transfer_quant="mxfp8_e4m3"`` through a GPU-resident store."""

import numpy as np
import pytest
import torch

import torchstore_amd as ts
from tests.mx_oracle import DEQUANT_CODES
from tests.test_gpu_mx import _canaried, _dev, _intact, requires_gpu
from tests.test_mx8 import (
    DTYPES, assert_dequant_matches, assert_pair_matches, inputs, ref_quant,
)
from tests.test_quant import make_input, same_bytes

pytestmark = pytest.mark.gpu

OTHER_COUNTERS = ("quant_launches", "mx_launches", "mx6_launches", "row_launches",
                  "tile_launches", "tensor_launches")
FP8 = torch.float8_e4m3fn


def _shifted(x):
    """The same data one element into its storage: the generic path."""
    base = torch.zeros(x.numel() + 1, dtype=x.dtype, device=x.device)
    base[1:] = x.reshape(-1)
    out = base[1:].view(x.shape)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_mx8_quant_kernel_matches_cpu_and_reference(dtype):
    from torchstore_amd.ops import gpu, mx8

    xs = inputs(dtype) + [
        make_input((2, 4128), dtype),  # fast, 129 blocks a row: a unit
        # straddles the rows and the last group of four scales is partial
        make_input((64, 1024), dtype),  # eight units
    ]
    xs = [x.to(_dev()) for x in xs]
    xs.append(_shifted(xs[-1]))
    for x in xs:
        others = [getattr(gpu, c)() for c in OTHER_COUNTERS]
        before = gpu.mx8_launches()
        (pair,) = mx8.quantize_mxfp8([x])
        assert gpu.mx8_launches() == before + 1
        assert [getattr(gpu, c)() for c in OTHER_COUNTERS] == others
        torch.cuda.synchronize()
        assert pair[0].device == x.device and pair[0].data_ptr() % 16 == 0
        assert_pair_matches(pair, x)
        (cpu_pair,) = mx8.quantize_mxfp8([x.cpu()])
        assert same_bytes(pair[0], cpu_pair[0]) and same_bytes(pair[1], cpu_pair[1])


@requires_gpu
@pytest.mark.parametrize("grid", [None, "64"])
def test_mx8_batch_one_launch_and_canaries(grid, monkeypatch):
    """Mixed dtypes and shapes, a generic tensor among fast ones and an empty
    one in ONE launch, into canaried buffers; one scales view starts 2 bytes
    into its arena (byte stores instead of dwords).  77 units: under a grid
    of 64 workgroups walk from the first descriptor into the later ones."""
    from torchstore_amd.ops import gpu, mx8

    if grid is None:
        monkeypatch.delenv("HIPSTORE_MX8_GRID", raising=False)
    else:
        monkeypatch.setenv("HIPSTORE_MX8_GRID", grid)
    xs = [
        make_input((520, 1024), torch.bfloat16),  # 65 units
        make_input((5, 201), torch.float32),  # generic among fast ones
        make_input((2, 4128), torch.float16),
        make_input((64, 1024), torch.float32),
        make_input((257,), torch.bfloat16),
    ]
    xs = [x.to(_dev()) for x in xs]
    triples, arenas = [], []
    for i, x in enumerate(xs):
        sshape = mx8.mx8_scales_shape(x.shape)
        ns, off = torch.Size(sshape).numel(), 2 if i == 3 else 0
        pa, pv = _canaried(x.numel())
        sa, sv = _canaried(off + ns)
        triples.append((x, pv.view(FP8).view(x.shape), sv[off:].view(sshape)))
        arenas.append((pa, x.numel(), sa, off + ns))
    assert triples[3][2].data_ptr() % 4 == 2
    empty = torch.empty(0, 8, dtype=torch.bfloat16, device=_dev())
    triples.append((empty, torch.empty(0, 8, dtype=FP8, device=_dev()),
                    torch.empty(0, 1, dtype=torch.uint8, device=_dev())))
    before = gpu.mx8_launches()
    gpu.quant_mx8_batch(triples, _dev())
    assert gpu.mx8_launches() == before + 1
    torch.cuda.synchronize()
    for (x, payload, scales), (pa, np_, sa, ns) in zip(triples, arenas):
        assert_pair_matches((payload, scales), x)
        assert _intact(pa, np_), "wrote past a payload"
        assert _intact(sa, ns), "wrote past the scales"
    assert arenas[3][2][:2].eq(0x5A).all(), "wrote before the scales"


@requires_gpu
@pytest.mark.parametrize("out_dtype", DTYPES)
def test_mx8_dequant_kernel_matches_reference(out_dtype):
    """The reference pairs of every shape in one launch, into canaried
    destinations; then an unaligned payload, a strided and an unaligned
    destination."""
    from torchstore_amd.ops import gpu, mx8

    xs = inputs(torch.float32) + [
        make_input(s, torch.float32) for s in [(2, 4128), (64, 1024)]
    ]
    pairs = [ref_quant(x) for x in xs]
    dev_pairs = [(p.to(_dev()), s.to(_dev())) for p, s in pairs]
    es = torch.empty((), dtype=out_dtype).element_size()
    outs, arenas = [], []
    for x in xs:
        arena, view = _canaried(x.numel() * es)
        outs.append(view.view(out_dtype).view(x.shape))
        arenas.append((arena, x.numel() * es))
    before = gpu.mx8_launches()
    mx8.dequantize_mxfp8_into(dev_pairs, outs)
    assert gpu.mx8_launches() == before + 1
    torch.cuda.synchronize()
    for pair, out, (arena, nb) in zip(pairs, outs, arenas):
        assert_dequant_matches(out, pair)
        assert _intact(arena, nb), "wrote past a destination"

    big = dev_pairs[-1]  # (64, 1024)
    pshift = _shifted(big[0].view(torch.uint8)).view(FP8)
    wide = torch.zeros(64, 2048, dtype=out_dtype, device=_dev())
    base = torch.zeros(64 * 1024 + 1, dtype=out_dtype, device=_dev())
    dests = [torch.empty(64, 1024, dtype=out_dtype, device=_dev()),
             wide[:, ::2], base[1:].view(64, 1024)]
    mx8.dequantize_mxfp8_into([(pshift, big[1]), big, big], dests)
    torch.cuda.synchronize()
    for out in dests:
        assert_dequant_matches(out, pairs[-1])
    assert wide[:, 1::2].eq(0).all() and base[0] == 0


@requires_gpu
@pytest.mark.parametrize("out_dtype", DTYPES)
def test_mx8_dequant_all_codes(out_dtype):
    """All 256 payload codes under every scale code of the grid, as rows of
    32 (fast) and of 31 (generic), in one launch."""
    from torchstore_amd.ops import mx8

    pairs = []
    for shape in [(8, 32), (9, 31)]:
        codes = (np.arange(shape[0] * shape[1]) % 256).astype(np.uint8)
        payload = torch.from_numpy(codes).view(FP8).view(shape)
        pairs += [(payload, torch.full((shape[0], 1), c, dtype=torch.uint8))
                  for c in DEQUANT_CODES]
    outs = [torch.empty(p.shape, dtype=out_dtype, device=_dev()) for p, _ in pairs]
    mx8.dequantize_mxfp8_into([(p.to(_dev()), s.to(_dev())) for p, s in pairs], outs)
    torch.cuda.synchronize()
    for pair, out in zip(pairs, outs):
        assert_dequant_matches(out, pair)  # NaN where the reference is NaN
        if pair[1][0, 0] == 255:
            assert torch.isnan(out).all()
        else:  # 0x7F and 0xFF, wherever they sit
            assert torch.isnan(out.view(-1)[127]) and torch.isnan(out.view(-1)[255])


@requires_gpu
async def test_mx8_state_dict_through_gpu_store():
    def weights(seed):
        shapes = [(256, 384), (96, 131), (384,)]
        a, b, norm = (make_input(s, torch.bfloat16, seed + i).to(_dev())
                      for i, s in enumerate(shapes))
        return {"layers": [{"w": a}, {"w": b}], "norm": norm, "step": seed}

    await ts.initialize(
        num_storage_volumes=1, strategy=ts.SingletonStrategy(), storage_device="auto"
    )
    try:
        dest, src = weights(0), weights(10)
        for seed in (10, 20):
            if seed == 20:  # the second push sees the source mutated in place
                new = weights(20)
                for i in (0, 1):
                    src["layers"][i]["w"].copy_(new["layers"][i]["w"])
                src["norm"].copy_(new["norm"])
                src["step"] = 20
            policy = ts.Mxfp8BlockQuant(exclude=("*norm*",))
            await ts.put_state_dict(src, "ck", transfer_quant=policy)
            want = [ref_quant(src["layers"][i]["w"]) for i in (0, 1)]
            assert same_bytes(await ts.get("ck/layers.0.w"), want[0][0])
            assert same_bytes(await ts.get("ck/<MX8_SCALES>/layers.1.w"), want[1][1])
            out = await ts.get_state_dict("ck", dest)
            torch.cuda.synchronize()
            for i in (0, 1):
                assert out["layers"][i]["w"] is dest["layers"][i]["w"]
                assert_dequant_matches(dest["layers"][i]["w"], want[i])
            assert same_bytes(dest["norm"], src["norm"])  # excluded: exact
            assert out["step"] == seed
    finally:
        await ts.shutdown()
