"""MXFP4 kernels on the GPU, byte for byte against the oracle of
``tests/mx_oracle.py`` (evaluated on the CPU), and ``transfer_quant="mxfp4"``
through a GPU-resident store."""

import pytest
import torch

import torchstore_amd as ts
from tests import mx_oracle as oracle
from tests.mx_oracle import DEQUANT_CODES, TIE_CASES
from tests.test_mx import assert_dequant_matches, assert_pair_matches
from tests.test_quant import make_input, same_bytes, signed_zero_input
from tests.value_grids import subnormal_block

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an AMD GPU"
)

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = oracle.SHAPES + [
    (2, 4128),  # fast path, 129 blocks per row: units straddle the rows
    (64, 1024),  # several units
]
CANARY = 0x5A
GUARD = 256


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    monkeypatch.delenv("HIPSTORE_MX_GRID", raising=False)


def _dev():
    return torch.device("cuda", 0)


def _canaried(nbytes):
    """(arena, view of its first nbytes): the rest holds the canary."""
    arena = torch.full((nbytes + GUARD,), CANARY, dtype=torch.uint8, device=_dev())
    return arena, arena[:nbytes]


def _intact(arena, nbytes):
    return bool(arena[nbytes:].eq(CANARY).all())


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_mx_quant_kernel_matches_oracle(dtype):
    from torchstore_amd.ops import gpu, mx

    xs = [make_input(s, dtype).to(_dev()) for s in SHAPES]
    # unaligned wide base: the same data one element into its storage
    base = torch.zeros(64 * 1024 + 1, dtype=dtype, device=_dev())
    base[1:] = xs[-1].reshape(-1)
    shifted = base[1:].view(64, 1024)
    assert shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
    xs += [shifted]
    xs += [signed_zero_input(s, dtype).to(_dev()) for s in [(3, 200), (3, 256)]]
    xs += [subnormal_block(dtype).to(_dev())]
    for x in xs:
        before = gpu.mx_launches()
        (pair,) = mx.quantize_mxfp4([x])
        assert gpu.mx_launches() == before + 1
        torch.cuda.synchronize()
        assert pair[0].device == x.device and pair[0].data_ptr() % 16 == 0
        assert_pair_matches(pair, x)


@requires_gpu
def test_mx_tie_grids():
    """Every rounding decision of e2m1, at five block scales per dtype, in
    one launch; and the way back."""
    from torchstore_amd.ops import gpu, mx

    grids = [oracle.e2m1_tie_grid(dtype, k) for dtype, k in TIE_CASES]
    before = gpu.mx_launches()
    pairs = mx.quantize_mxfp4([g.to(_dev()) for g in grids])
    assert gpu.mx_launches() == before + 1
    torch.cuda.synchronize()
    for pair, g, (_, k) in zip(pairs, grids, TIE_CASES):
        assert_pair_matches(pair, g)
        assert pair[1].eq(max(k + 127, 0)).all()
    for out_dtype in DTYPES:
        outs = [torch.empty(g.shape, dtype=out_dtype, device=_dev()) for g in grids]
        mx.dequantize_mxfp4_into(pairs, outs)
        torch.cuda.synchronize()
        for out, pair in zip(outs, pairs):
            assert_dequant_matches(out, pair)


@requires_gpu
def test_mx_batch_one_launch_and_canaries():
    """Four tensors of mixed dtype and shape plus an empty one in ONE launch,
    into buffers with a canary region behind every payload and scales."""
    from torchstore_amd.ops import gpu, mx

    xs = [
        make_input((64, 1024), torch.bfloat16),
        make_input((5, 201), torch.float32),  # generic among fast ones
        make_input((2, 4128), torch.float16),
        make_input((257,), torch.bfloat16),
    ]
    xs = [x.to(_dev()) for x in xs]
    triples, arenas = [], []
    for x in xs:
        pshape, sshape = mx.mx_shapes(x.shape)
        np_, ns = torch.Size(pshape).numel(), torch.Size(sshape).numel()
        pa, pv = _canaried(np_)
        sa, sv = _canaried(ns)
        triples.append((x, pv.view(pshape), sv.view(sshape)))
        arenas.append((pa, np_, sa, ns))
    empty = torch.empty(0, 8, dtype=torch.bfloat16, device=_dev())
    triples.append(
        (
            empty,
            torch.empty(0, 4, dtype=torch.uint8, device=_dev()),
            torch.empty(0, 1, dtype=torch.uint8, device=_dev()),
        )
    )
    before = gpu.mx_launches()
    quant_before = gpu.quant_launches()
    gpu.quant_mx_batch(triples, _dev())
    assert gpu.mx_launches() == before + 1
    assert gpu.quant_launches() == quant_before  # a counter of its own
    torch.cuda.synchronize()
    for (x, payload, scales), (pa, np_, sa, ns) in zip(triples, arenas):
        assert_pair_matches((payload, scales), x)
        assert _intact(pa, np_), "wrote past a payload"
        assert _intact(sa, ns), "wrote past the scales"

    # the public entry point batches the same way
    before = gpu.mx_launches()
    pairs = mx.quantize_mxfp4(xs + [empty])
    assert gpu.mx_launches() == before + 1
    torch.cuda.synchronize()
    for pair, x in zip(pairs, xs):
        assert_pair_matches(pair, x)
    assert pairs[-1][0].shape == (0, 4) and pairs[-1][1].shape == (0, 1)
    with pytest.raises(ValueError, match="contiguous"):
        gpu.quant_mx_batch([(xs[0].t(), triples[0][1], triples[0][2])], _dev())


@requires_gpu
@pytest.mark.parametrize("out_dtype", DTYPES)
def test_mx_dequant_kernel_matches_oracle(out_dtype):
    """One launch over every shape, into canaried destinations; then a
    payload one byte into its storage, a non-contiguous destination and an
    unaligned one."""
    from torchstore_amd.ops import gpu, mx

    xs = [make_input(s, torch.float32) for s in SHAPES]
    xs += [signed_zero_input(s, torch.float32) for s in [(3, 200), (3, 256)]]
    pairs = [oracle.oracle_quant(x) for x in xs]
    es = torch.empty((), dtype=out_dtype).element_size()
    dev_pairs, outs, arenas = [], [], []
    for x, (p, s) in zip(xs, pairs):
        dev_pairs.append((p.to(_dev()), s.to(_dev())))
        nb = x.numel() * es
        arena, view = _canaried(nb)
        outs.append(view.view(out_dtype).view(x.shape))
        arenas.append((arena, nb))
    before = gpu.mx_launches()
    mx.dequantize_mxfp4_into(dev_pairs, outs)
    assert gpu.mx_launches() == before + 1
    torch.cuda.synchronize()
    for pair, out, (arena, nb) in zip(pairs, outs, arenas):
        assert_dequant_matches(out, pair)
        assert _intact(arena, nb), "wrote past a destination"

    i = len(SHAPES) - 1  # (64, 1024)
    p, s = pairs[i]
    pbase = torch.zeros(p.numel() + 1, dtype=torch.uint8, device=_dev())
    pbase[1:] = dev_pairs[i][0].reshape(-1)
    pshift = pbase[1:].view(p.shape)
    assert pshift.data_ptr() % 16 == 1
    wide = torch.zeros(64, 2048, dtype=out_dtype, device=_dev())
    strided = wide[:, ::2]
    base = torch.zeros(64 * 1024 + 1, dtype=out_dtype, device=_dev())
    shifted = base[1:].view(64, 1024)
    plain = torch.empty(64, 1024, dtype=out_dtype, device=_dev())
    big = dev_pairs[i]
    mx.dequantize_mxfp4_into(
        [(pshift, big[1]), big, big], [plain, strided, shifted]
    )
    torch.cuda.synchronize()
    for out in (plain, strided, shifted):
        assert_dequant_matches(out, (p, s))
    assert wide[:, 1::2].eq(0).all() and base[0] == 0


@requires_gpu
@pytest.mark.parametrize("out_dtype", DTYPES)
def test_mx_dequant_all_bytes(out_dtype):
    """All 256 payload bytes under every scale code of the grid, fast and
    generic path, in one launch."""
    from torchstore_amd.ops import mx

    payload, shape = oracle.all_bytes_payload()
    pairs, outs = [], []
    for code in DEQUANT_CODES:
        scales = oracle.scales_for(shape, code)
        pairs.append((payload, scales))
        outs.append(torch.empty(shape, dtype=out_dtype, device=_dev()))
        # the same bytes as rows of 31: short blocks on the generic path
        pairs.append((payload, scales))
        outs.append(torch.empty(16, 31, dtype=out_dtype, device=_dev()))
    mx.dequantize_mxfp4_into(
        [(p.to(_dev()), s.to(_dev())) for p, s in pairs], outs
    )
    torch.cuda.synchronize()
    for pair, out in zip(pairs, outs):
        assert_dequant_matches(out, pair)
    assert torch.isnan(outs[-2]).all()  # scale code 255


@requires_gpu
async def test_mx_state_dict_through_gpu_store():
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
        p, s = oracle.oracle_quant(w)
        return oracle.oracle_dequant(p, s, tuple(w.shape), torch.bfloat16)

    policy = ts.Mxfp4BlockQuant(exclude=("*norm*",))
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
            assert stored.dtype == torch.uint8 and stored.shape == (256, 192)
            assert same_bytes(stored, oracle.oracle_quant(src["layers"][0]["w"])[0])
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
