"""MXFP6 kernels on the GPU, byte for byte against the CPU implementation and
the float64 reference of ``tests/test_mx6.py``, and
``transfer_quant="mxfp6_e2m3"`` through a GPU-resident store."""

import pytest
import torch

import torchstore_amd as ts
from tests.test_gpu_mx import DTYPES, _canaried, _dev, _intact, requires_gpu
from tests.test_mx6 import SHAPES as CPU_SHAPES
from tests.test_mx6 import assert_matches_ref, ref_dequant, ref_quant, tie_block
from tests.test_quant import make_input, same_bytes

pytestmark = pytest.mark.gpu

SHAPES = CPU_SHAPES + [
    (2, 4128),  # fast path, 129 blocks per row: units straddle the rows
    (64, 1024),  # several units
]


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    monkeypatch.delenv("HIPSTORE_MX6_GRID", raising=False)


def _shifted(t):
    """The same data one element into a storage of its own: unaligned base."""
    base = torch.zeros(t.numel() + 1, dtype=t.dtype, device=_dev())
    base[1:] = t.reshape(-1)
    out = base[1:].view(t.shape)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_mx6_quant_kernel_matches_cpu(dtype):
    from torchstore_amd.ops import gpu, mx6

    cpu = [make_input(s, dtype) for s in SHAPES] + [tie_block(dtype)]
    xs = [x.to(_dev()) for x in cpu]
    cpu.append(cpu[len(SHAPES) - 1])  # (64, 1024) again, on the generic path
    xs.append(_shifted(xs[len(SHAPES) - 1]))
    want = mx6.quantize_mxfp6(cpu)
    for x, w in zip(xs, want):
        counts = gpu.mx6_launches(), gpu.mx_launches(), gpu.quant_launches()
        (pair,) = mx6.quantize_mxfp6([x])
        assert (gpu.mx6_launches(), gpu.mx_launches(), gpu.quant_launches()) == (
            counts[0] + 1, counts[1], counts[2]
        )
        torch.cuda.synchronize()
        assert pair[0].device == x.device and pair[0].data_ptr() % 16 == 0
        assert same_bytes(pair[0], w[0]) and same_bytes(pair[1], w[1])


@requires_gpu
def test_mx6_batch_one_launch_and_canaries():
    """Four tensors of mixed dtype and shape plus an empty one in ONE launch,
    into buffers with a canary region behind every payload and scales."""
    from torchstore_amd.ops import gpu, mx6

    xs = [
        make_input((64, 1024), torch.bfloat16),
        make_input((5, 201), torch.float32),  # generic among fast ones
        make_input((2, 4128), torch.float16),
        make_input((257,), torch.bfloat16),
    ]
    xs = [x.to(_dev()) for x in xs]
    triples, arenas = [], []
    for x in xs:
        pshape, sshape = mx6.mx6_shapes(x.shape)
        np_, ns = torch.Size(pshape).numel(), torch.Size(sshape).numel()
        pa, pv = _canaried(np_)
        sa, sv = _canaried(ns)
        triples.append((x, pv.view(pshape), sv.view(sshape)))
        arenas.append((pa, np_, sa, ns))
    empty = torch.empty(0, 8, dtype=torch.bfloat16, device=_dev())
    triples.append((empty,) + tuple(mx6.alloc_mx6([empty.shape], _dev())[0]))
    before = gpu.mx6_launches()
    gpu.quant_mx6_batch(triples, _dev())
    assert gpu.mx6_launches() == before + 1
    torch.cuda.synchronize()
    for (x, payload, scales), (pa, np_, sa, ns) in zip(triples, arenas):
        assert_matches_ref((payload, scales), x)
        assert _intact(pa, np_), "wrote past a payload"
        assert _intact(sa, ns), "wrote past the scales"
    with pytest.raises(ValueError, match="contiguous"):
        gpu.quant_mx6_batch([(xs[0].t(), triples[0][1], triples[0][2])], _dev())


@requires_gpu
@pytest.mark.parametrize("out_dtype", DTYPES)
def test_mx6_dequant_kernel_matches_reference(out_dtype):
    """One launch over every shape, into canaried destinations; then a
    payload one byte into its storage, a non-contiguous destination and an
    unaligned one."""
    from torchstore_amd.ops import gpu, mx6

    xs = [make_input(s, torch.float32) for s in SHAPES]
    pairs = [ref_quant(x) for x in xs]
    es = torch.empty((), dtype=out_dtype).element_size()
    dev_pairs, outs, arenas = [], [], []
    for x, (p, s) in zip(xs, pairs):
        dev_pairs.append((p.to(_dev()), s.to(_dev())))
        arena, view = _canaried(x.numel() * es)
        outs.append(view.view(out_dtype).view(x.shape))
        arenas.append((arena, x.numel() * es))
    before = gpu.mx6_launches()
    mx6.dequantize_mxfp6_into(dev_pairs, outs)
    assert gpu.mx6_launches() == before + 1
    torch.cuda.synchronize()
    for x, pair, out, (arena, nb) in zip(xs, pairs, outs, arenas):
        assert same_bytes(out, ref_dequant(*pair, x.shape, out_dtype))
        assert _intact(arena, nb), "wrote past a destination"

    big, (p, s) = dev_pairs[-1], pairs[-1]  # (64, 1024)
    pshift = _shifted(big[0])
    wide = torch.zeros(64, 2048, dtype=out_dtype, device=_dev())
    strided = wide[:, ::2]
    shifted = _shifted(torch.zeros(64, 1024, dtype=out_dtype, device=_dev()))
    plain = torch.empty(64, 1024, dtype=out_dtype, device=_dev())
    mx6.dequantize_mxfp6_into(
        [(pshift, big[1]), big, big], [plain, strided, shifted]
    )
    torch.cuda.synchronize()
    for out in (plain, strided, shifted):
        assert same_bytes(out.contiguous(), ref_dequant(p, s, (64, 1024), out_dtype))
    assert wide[:, 1::2].eq(0).all()


@requires_gpu
@pytest.mark.parametrize("out_dtype", DTYPES)
def test_mx6_dequant_all_codes(out_dtype):
    """All 64 codes under the extreme scale codes, as one full block per row
    (fast) and as rows of 31 (generic), in one launch."""
    from torchstore_amd.ops import mx6

    # every code of both signs: the 64 six-bit patterns in wire order
    bits = (torch.arange(64).reshape(-1, 1) >> torch.arange(6)) & 1
    by = bits.reshape(-1, 8).mul(1 << torch.arange(8)).sum(-1).to(torch.uint8)
    payload = by.reshape(2, 24)
    pairs, outs, shapes = [], [], []
    for code in (0, 1, 127, 254, 255):
        scales = torch.full((2, 1), code, dtype=torch.uint8)
        for shape in ((2, 32), (2, 31)):  # 31 columns are 24 bytes too
            pairs.append((payload, scales))
            shapes.append(shape)
            outs.append(torch.empty(shape, dtype=out_dtype, device=_dev()))
    mx6.dequantize_mxfp6_into([(p.to(_dev()), s.to(_dev())) for p, s in pairs], outs)
    torch.cuda.synchronize()
    for (p, s), shape, out in zip(pairs[:-2], shapes, outs):
        assert same_bytes(out, ref_dequant(p, s, shape, out_dtype))
    assert torch.isnan(outs[-1]).all() and torch.isnan(outs[-2]).all()  # 255


@requires_gpu
async def test_mx6_state_dict_through_gpu_store():
    def weights(seed):
        return {
            "layers": [
                {"w": make_input((256, 384), torch.bfloat16, seed).to(_dev())},
                {"w": make_input((96, 131), torch.bfloat16, seed + 1).to(_dev())},
            ],
            "norm": make_input((384,), torch.bfloat16, seed + 2).to(_dev()),
            "step": seed,
        }

    def expect(w):
        return ref_dequant(*ref_quant(w.cpu()), tuple(w.shape), torch.bfloat16)

    policy = ts.Mxfp6BlockQuant(exclude=("*norm*",))
    await ts.initialize(
        num_storage_volumes=1, strategy=ts.SingletonStrategy(), storage_device="auto"
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
            assert stored.dtype == torch.uint8 and stored.shape == (256, 288)
            assert same_bytes(stored, ref_quant(src["layers"][0]["w"].cpu())[0])
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
