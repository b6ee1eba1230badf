"""Per-tensor FP8 kernels (K14/K15) on the GPU, byte for byte against the oracle of
``tests/test_quant_tensor.py``, and the format through a GPU-resident store."""

import functools

import pytest
import torch

import torchstore_amd as ts
from tests.test_quant import make_input, same_bytes, signed_zero_input
from tests.test_quant_tensor import (
    DTYPES, FLOOR_SCALE, SHAPES, assert_pair_matches, oracle_dequant,
    oracle_quant, zero_matrix_input,
)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an AMD GPU")

# a unit is 16384 elements.  (1152, 1408) is 99 units of one matrix: at a grid
# of 64 a workgroup keeps a running maximum over several.  (40, 129, 128) is
# two units per matrix on the fast path, (5, 129, 130) the same on the generic
# one: workgroups cross matrix boundaries mid-walk and publish on the change.
GPU_SHAPES = SHAPES + [(1152, 1408), (40, 129, 128), (5, 129, 130)]
CANARY = 0x5A
GUARD = 256


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    monkeypatch.delenv("HIPSTORE_TENSOR_GRID", raising=False)


def _dev():
    return torch.device("cuda", 0)


def _max_last(x):
    """x in reverse order, and the maximum of every matrix in its last element:
    pass A's last workgroups publish what pass B's first ones need."""
    y = x.flip(tuple(range(x.dim()))).contiguous()
    y2 = y.view(torch.Size(x.shape[:-2]).numel(), -1)
    y2[:, -1] = y2.abs().amax(dim=1) * 2
    return y


@functools.lru_cache(maxsize=None)
def _cases(dtype):
    """[(CPU input, oracle pair, oracle pair of half the input, placed one
    element into its storage)]; the last case has an all-zero matrix."""
    xs = []
    for shape in GPU_SHAPES:
        x = make_input(shape, dtype)
        xs += [(x, False), (_max_last(x), False)]
    shifted = make_input((130, 208), dtype)
    xs += [(shifted, True), (_max_last(shifted), True)]
    xs.append((signed_zero_input((130, 200), dtype), False))
    xs.append((zero_matrix_input(dtype), False))
    return [(x, oracle_quant(x), oracle_quant(x * 0.5), shift) for x, shift in xs]


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


def _launch_counts(gpu):
    return (gpu.tensor_launches(), gpu.tile_launches(), gpu.quant_launches(),
            gpu.row_launches())


@requires_gpu
@pytest.mark.parametrize("grid", [None, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tensor_quant_kernel_matches_oracle(dtype, grid, monkeypatch):
    """Two launches per call; the second call quantises half the data into
    the same buffers, which a stale amax slot would give the first scales."""
    from torchstore_amd.ops import gpu, quant_tensor

    if grid:
        monkeypatch.setenv("HIPSTORE_TENSOR_GRID", str(grid))
    cases = _cases(dtype)
    triples, arenas = [], []
    for x, _, _, shift in cases:
        x = _on_device(x, shift)
        sshape = quant_tensor.tensor_scales_shape(x.shape)
        ns = torch.Size(sshape).numel() * 4
        pa, pv = _canaried(x.numel())
        sa, sv = _canaried(ns)
        payload = pv.view(torch.float8_e4m3fn).view(x.shape)
        triples.append((x, payload, sv.view(torch.float32).view(sshape)))
        arenas.append((pa, x.numel(), sa, ns))
    for call in (1, 2):
        before = _launch_counts(gpu)
        gpu.quant_tensor_batch(triples, _dev())
        assert _launch_counts(gpu) == (before[0] + 2,) + before[1:]
        torch.cuda.synchronize()
        for (x, payload, scales), case, (pa, np_, sa, ns) in zip(triples, cases, arenas):
            what = f"{tuple(x.shape)} call {call}"
            assert same_bytes(payload, case[call][0]), f"payload differs {what}"
            assert same_bytes(scales, case[call][1]), f"scales differ {what}"
            assert _intact(pa, np_) and _intact(sa, ns), f"wrote past {what}"
        assert triples[-1][2][1, 0, 0].cpu() == FLOOR_SCALE
        for (x, _, _), case in zip(triples, cases):
            x.copy_(case[0] * 0.5)
    with pytest.raises(ValueError, match="contiguous"):
        gpu.quant_tensor_batch([(triples[-1][0].transpose(1, 2),) + triples[-1][1:]], _dev())


@requires_gpu
@pytest.mark.parametrize("out_dtype", DTYPES)
def test_tensor_dequant_kernel_matches_oracle(out_dtype):
    """One launch into canaried destinations; then a strided and an unaligned one."""
    from torchstore_amd.ops import gpu, quant_tensor

    xs = [make_input(s, torch.float32) for s in GPU_SHAPES]
    pairs = [oracle_quant(x) for x in xs]
    es = torch.empty((), dtype=out_dtype).element_size()
    dev_pairs, outs, arenas = [], [], []
    for x, (p, s) in zip(xs, pairs):
        dev_pairs.append((p.to(_dev()), s.to(_dev())))
        arena, view = _canaried(x.numel() * es)
        outs.append(view.view(out_dtype).view(x.shape))
        arenas.append((arena, x.numel() * es))
    before = gpu.tensor_launches()
    quant_tensor.dequantize_fp8_tensor_into(dev_pairs, outs)
    assert gpu.tensor_launches() == before + 1
    torch.cuda.synchronize()
    for pair, out, (arena, nb) in zip(pairs, outs, arenas):
        assert same_bytes(out, oracle_dequant(*pair, out_dtype))
        assert _intact(arena, nb), "wrote past a destination"

    i = GPU_SHAPES.index((40, 129, 128))
    wide = torch.zeros(40, 129, 256, dtype=out_dtype, device=_dev())
    base = torch.zeros(40 * 129 * 128 + 1, dtype=out_dtype, device=_dev())
    strided, shifted = wide[..., ::2], base[1:].view(40, 129, 128)
    quant_tensor.dequantize_fp8_tensor_into([dev_pairs[i]] * 2, [strided, shifted])
    torch.cuda.synchronize()
    for out in (strided, shifted):
        assert same_bytes(out, oracle_dequant(*pairs[i], out_dtype))
    assert wide[..., 1::2].eq(0).all() and base[0] == 0


@requires_gpu
async def test_tensor_state_dict_through_gpu_store():
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
        await ts.put_state_dict(src, "ck", transfer_quant=ts.Fp8TensorQuant(exclude=("*norm*",)))
        out = await ts.get_state_dict("ck", dest)
        raw = await ts.get_state_dict("ck", dequantize=False)
        torch.cuda.synchronize()
        for i, w in enumerate(ws):
            assert out["layers"][i]["w"] is dest["layers"][i]["w"]
            ref = oracle_dequant(*oracle_quant(w), torch.bfloat16)
            assert same_bytes(dest["layers"][i]["w"], ref)
            leaf = raw["layers"][i]["w"]
            assert isinstance(leaf, ts.TensorQuantizedTensor)
            assert_pair_matches((leaf.payload, leaf.scales), w)
        assert same_bytes(dest["norm"], src["norm"]) and out["step"] == 10  # excluded
    finally:
        await ts.shutdown()
