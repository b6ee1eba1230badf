"""The value space of the kernels that change bits, bit for bit: the cast
kernel (K3) on every 16-bit pattern and around every rounding decision of an
f32 source, the FP8 kernels (K4/K5) on exact e4m3 ties, subnormal and tiny
blocks and all 256 payload codes, and the quant kernel's unit walk under a
small grid.

The references are the ones written out in ``tests/value_grids.py`` (proved
on the CPU by ``tests/test_value_grids.py``) and the oracle of
``tests/test_quant.py``.  Every comparison is bit-exact; a NaN input only has
to give a NaN.  Every destination lies in a ``uint8`` arena with a canary
behind it.
"""

import functools
import os

import numpy as np
import pytest
import torch

from tests import value_grids as vg
from tests.test_quant import (
    assert_pair_matches,
    make_input,
    oracle_dequant,
    oracle_quant,
    same_bytes,
)
from tests.test_value_grids import (
    check_subnormal_pair,
    check_zero_and_tiny_pair,
)
from tests.value_grids import BF16, CAST_PAIRS, DTYPES, F16, F32

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an AMD GPU"
)

CANARY = 0x5A
GUARD = 256
UNIT_BLOCKS = 64  # kQuantUnitBlocks


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in [k for k in os.environ if k.startswith("HIPSTORE_")]:
        monkeypatch.delenv(k, raising=False)


def _ids(value):
    return str(value).replace("torch.", "")


def _dev():
    return torch.device("cuda", 0)


def _es(dtype):
    return torch.empty((), dtype=dtype).element_size()


class Arena:
    """``shape`` elements of ``dtype`` inside a uint8 buffer filled with the
    canary, ``lead`` bytes in (16 B aligned when 0) and GUARD bytes short of
    its end."""

    def __init__(self, dtype, shape, lead=0):
        self.nbytes = torch.Size(shape).numel() * _es(dtype)
        self.lead = lead
        self.buf = torch.full(
            (lead + self.nbytes + GUARD,), CANARY, dtype=torch.uint8,
            device=_dev(),
        )
        self.t = self.buf[lead : lead + self.nbytes].view(dtype).view(shape)

    def check(self):
        assert self.buf[: self.lead].eq(CANARY).all(), "wrote before a buffer"
        assert self.buf[self.lead + self.nbytes :].eq(CANARY).all(), (
            "wrote past a buffer"
        )


def _set_knobs(monkeypatch, **knobs):
    for name, value in knobs.items():
        if value is not None:
            monkeypatch.setenv(name, str(value))


# ---------------------------------------------------------------------------
# cast (K3)
# ---------------------------------------------------------------------------

CAST_VS = [None, 16, 1, 32]
CAST_GRIDS = [None, 64]


def cast_trips(numel, v_knob, grid_knob):
    """Trips of thread 0 through the vector loop, by launch_cast's sizing:
    the grid is sized for HIPSTORE_CAST_V elements a thread, the kernel takes
    8 or 16."""
    v = v_knob or 8
    kernel_v = 16 if v >= 16 else 8
    work = -(-numel // v)
    grid = max(1, min(-(-work // 256), grid_knob or 1024))
    return -(-(numel // kernel_v * kernel_v) // (grid * 256 * kernel_v))


@functools.lru_cache(maxsize=None)
def _cast_case(src_dtype, dst_dtype):
    """(source on the CPU, NaN source or None, reference bits): computed
    once, shared by every test of the pair."""
    if src_dtype == F32:
        src, nans = vg.f32_rounding_grid(dst_dtype)
    else:
        # four times over: two trips of the loop at a grid of 64 and V = 8
        src, nans = vg.all_bits16(src_dtype).repeat(4), None
    return src, nans, vg.cast_reference_bits(src, dst_dtype)


def _cast_and_check(src, dst_dtype, ref=None):
    from torchstore_amd.ops import gpu

    s = src.to(_dev())
    assert s.data_ptr() % 16 == 0
    out = Arena(dst_dtype, (src.numel(),))
    gpu.cast_copy(s, out.t)
    torch.cuda.synchronize()
    out.check()
    return vg.check_cast(src, out.t.cpu(), ref)


@requires_gpu
@pytest.mark.parametrize("grid", CAST_GRIDS)
@pytest.mark.parametrize("v", CAST_VS)
@pytest.mark.parametrize(
    "src_dtype,dst_dtype", [p for p in CAST_PAIRS if p[0] != F32], ids=_ids
)
def test_cast_every_16bit_pattern(src_dtype, dst_dtype, v, grid, monkeypatch):
    """All 65536 source patterns (+-0, +-inf and the subnormals among them),
    under both kernel widths and with the grid-stride loop taken."""
    src, _, ref = _cast_case(src_dtype, dst_dtype)
    assert src.numel() == 4 * 65536
    if grid == 64 and v is None:
        assert cast_trips(src.numel(), v, grid) == 2
    if grid is None and v != 32:
        assert cast_trips(src.numel(), v, grid) == 1
    _set_knobs(monkeypatch, HIPSTORE_CAST_V=v, HIPSTORE_CAST_GRID=grid)
    n = _cast_and_check(src, dst_dtype, ref)
    n_nan = 2 * ((1 << (7 if src_dtype == BF16 else 10)) - 1)
    assert n == 4 * (65536 - n_nan)


@requires_gpu
@pytest.mark.parametrize("grid", CAST_GRIDS)
@pytest.mark.parametrize("v", CAST_VS)
@pytest.mark.parametrize("dst_dtype", [BF16, F16], ids=_ids)
def test_cast_f32_rounding_grid(dst_dtype, v, grid, monkeypatch):
    """Every tie, every neighbour of a tie, overflow to inf, underflow to a
    subnormal and to zero; the NaNs separately."""
    src, nans, ref = _cast_case(F32, dst_dtype)
    if grid == 64 and v is None:
        assert cast_trips(src.numel(), v, grid) == 3
    if grid == 64:
        assert cast_trips(src.numel(), v, grid) >= 2
    _set_knobs(monkeypatch, HIPSTORE_CAST_V=v, HIPSTORE_CAST_GRID=grid)
    assert _cast_and_check(src, dst_dtype, ref) == src.numel()
    assert _cast_and_check(nans, dst_dtype) == 0


TAIL_NUMELS = [0, 1, 7, 8, 9, 15, 16, 17, 2048 + 15, 64 * 256 * 8 + 8 * 5 + 7]


@requires_gpu
@pytest.mark.parametrize("v", [8, 16])
@pytest.mark.parametrize("src_dtype,dst_dtype", CAST_PAIRS, ids=_ids)
def test_cast_tails(src_dtype, dst_dtype, v, monkeypatch):
    """Lengths around the vector width: the canary directly behind the last
    element shows that the tail writes numel % V elements and no more."""
    src, _, ref = _cast_case(src_dtype, dst_dtype)
    _set_knobs(monkeypatch, HIPSTORE_CAST_V=v, HIPSTORE_CAST_GRID=64)
    assert cast_trips(TAIL_NUMELS[-1], v, 64) == (2 if v == 8 else 1)
    for numel in TAIL_NUMELS:
        assert numel <= src.numel()
        n = _cast_and_check(src[:numel], dst_dtype, ref[:numel])
        assert n <= numel


@requires_gpu
@pytest.mark.parametrize("src_dtype,dst_dtype", CAST_PAIRS, ids=_ids)
def test_cast_fallbacks_and_wrappers(src_dtype, dst_dtype):
    """A source or destination off 16 B alignment (cast_copy defers to
    torch), cast_tensor on a non-contiguous input and cast_into: the same
    rule holds for all of them."""
    from torchstore_amd.ops import gpu
    from torchstore_amd.ops.cast import cast_into, cast_tensor

    src, nans, ref = _cast_case(src_dtype, dst_dtype)
    n = 40_000 + 13
    src, ref = src[:n], ref[:n]
    if nans is not None:
        nan_ref = vg.cast_reference_bits(nans, dst_dtype)
        src, ref = torch.cat([src, nans]), np.concatenate([ref, nan_ref])
        n = src.numel()

    # source one element off
    base = torch.zeros(n + 1, dtype=src_dtype, device=_dev())
    base[1:] = src.to(_dev())
    shifted = base[1:]
    assert shifted.data_ptr() % 16 != 0
    out = Arena(dst_dtype, (n,))
    gpu.cast_copy(shifted, out.t)
    torch.cuda.synchronize()
    out.check()
    vg.check_cast(src, out.t.cpu(), ref)

    # destination one element off
    out = Arena(dst_dtype, (n,), lead=_es(dst_dtype))
    assert out.t.data_ptr() % 16 != 0
    gpu.cast_copy(src.to(_dev()), out.t)
    torch.cuda.synchronize()
    out.check()
    vg.check_cast(src, out.t.cpu(), ref)

    # cast_tensor packs a non-contiguous input first
    wide = torch.zeros(n, 2, dtype=src_dtype, device=_dev())
    wide[:, 0] = src.to(_dev())
    view = wide[:, 0]
    assert not view.is_contiguous()
    got = cast_tensor(view, dst_dtype)
    torch.cuda.synchronize()
    assert got.dtype == dst_dtype and got.shape == (n,)
    vg.check_cast(src, got.cpu(), ref)

    # cast_into a preallocated buffer
    out = Arena(dst_dtype, (n,))
    cast_into(src.to(_dev()), out.t)
    torch.cuda.synchronize()
    out.check()
    vg.check_cast(src, out.t.cpu(), ref)


# ---------------------------------------------------------------------------
# FP8 (K4/K5)
# ---------------------------------------------------------------------------


def _shifted(x):
    """The same data one element into its storage: the generic path."""
    base = torch.zeros(x.numel() + 1, dtype=x.dtype, device=_dev())
    base[1:] = x.reshape(-1).to(_dev())
    s = base[1:].view(x.shape)
    assert s.data_ptr() % 16 != 0 and s.is_contiguous()
    return s


def _quant_into_arenas(xs):
    """One launch over ``xs`` (on the device) into canaried payload and
    scales buffers; returns the pairs after checking the canaries."""
    from torchstore_amd.ops import gpu

    triples, arenas = [], []
    for x in xs:
        pa = Arena(torch.float8_e4m3fn, tuple(x.shape))
        sa = Arena(F32, (*x.shape[:-1], -(-x.shape[-1] // 128)))
        triples.append((x, pa.t, sa.t))
        arenas += [pa, sa]
    before = gpu.quant_launches()
    gpu.quant_fp8_batch(triples, _dev())
    assert gpu.quant_launches() == before + 1
    torch.cuda.synchronize()
    for a in arenas:
        a.check()
    return [(p, s) for _, p, s in triples]


def _dequant_into_arenas(pairs, out_dtype, leads=None):
    """One launch over ``pairs`` into canaried destinations of ``out_dtype``
    (``leads[i]`` bytes into their arenas); returns the outputs."""
    from torchstore_amd.ops import gpu, quant

    leads = leads or [0] * len(pairs)
    arenas = [
        Arena(out_dtype, tuple(p.shape), lead) for (p, _), lead in zip(pairs, leads)
    ]
    dev_pairs = [(p.to(_dev()), s.to(_dev())) for p, s in pairs]
    before = gpu.quant_launches()
    quant.dequantize_fp8_into(dev_pairs, [a.t for a in arenas])
    assert gpu.quant_launches() == before + 1
    torch.cuda.synchronize()
    for a in arenas:
        a.check()
    return [a.t for a in arenas]


@requires_gpu
@pytest.mark.parametrize("dtype,k", vg.TIE_CASES, ids=_ids)
def test_fp8_tie_grid(dtype, k):
    """Every e4m3 rounding tie and its neighbours at an exact power-of-two
    scale, on the fast and the generic path, and back into every dtype."""
    from torchstore_amd.ops import gpu, quant

    x = vg.e4m3_tie_grid(dtype, k)
    want = torch.from_numpy(vg.e4m3_rne(x.double().numpy() / 2.0 ** k))
    want = want.view(x.shape)
    xd = x.to(_dev())
    assert xd.data_ptr() % 16 == 0

    before = gpu.quant_launches()
    (public,) = quant.quantize_fp8([xd])
    assert gpu.quant_launches() == before + 1
    torch.cuda.synchronize()
    fast, generic = _quant_into_arenas([xd, _shifted(x)])
    for pair in (public, fast, generic):
        assert torch.equal(pair[0].cpu().view(torch.uint8), want)
        assert (pair[1].cpu().double() == 2.0 ** k).all()
        assert_pair_matches(pair, x)

    pair = (fast[0].cpu(), fast[1].cpu())
    for out_dtype in DTYPES:
        ref = oracle_dequant(*pair, out_dtype)
        es = _es(out_dtype)
        aligned, off = _dequant_into_arenas([pair, pair], out_dtype, [0, es])
        assert off.data_ptr() % 16 != 0
        for out in (aligned, off):
            assert same_bytes(out, ref)
            vg.check_dequant(
                out, vg.dequant_reference_bits(*pair, out_dtype)
            )
        if k == 118 and out_dtype == F16:  # the recipe's IEEE overflow
            assert torch.equal(
                torch.isinf(aligned.cpu()), pair[0].float() != 0
            )


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_fp8_subnormal_and_tiny_blocks(dtype):
    """A block wholly in the subnormal range of its dtype (f16: a real scale
    and many codes, so a flushed subnormal shows; bf16/f32: the floor scale
    and +-0 with every sign kept), an all-zero block and one below the amax
    floor; fast and generic path in one launch."""
    sub = vg.subnormal_block(dtype)
    tiny = vg.zero_and_tiny_blocks(dtype)
    xs = [sub.to(_dev()), tiny.to(_dev()), _shifted(sub), _shifted(tiny)]
    pairs = _quant_into_arenas(xs)
    for pair, x in zip(pairs, [sub, tiny, sub, tiny]):
        assert_pair_matches(pair, x)
    for pair in (pairs[0], pairs[2]):
        check_subnormal_pair(pair, dtype)
    for pair in (pairs[1], pairs[3]):
        check_zero_and_tiny_pair(pair)


@requires_gpu
@pytest.mark.parametrize("out_dtype", DTYPES, ids=_ids)
def test_fp8_dequant_all_codes(out_dtype):
    """All 256 codes times five scales in one launch, into aligned (fast)
    and off-by-one-element (generic) destinations: the narrowing convert in
    the f16 subnormal range, at overflow to inf and at the sign of zero; the
    two NaN codes give NaN."""
    payload = vg.all_codes_payload()
    pairs = [(payload, vg.scales_for(payload, s)) for s in vg.DEQUANT_SCALES]
    es = _es(out_dtype)
    outs = _dequant_into_arenas(
        pairs + pairs, out_dtype, [0] * len(pairs) + [es] * len(pairs)
    )
    assert outs[-1].data_ptr() % 16 != 0
    for (p, s), out in zip(pairs + pairs, outs):
        vg.check_dequant(out, vg.dequant_reference_bits(p, s, out_dtype))
        vg.check_dequant(out, vg.bits_of(oracle_dequant(p, s, out_dtype)))
        assert torch.isnan(out.cpu().view(-1)[[0x7F, 0xFF, 256 + 0x7F]]).all()


WALK_GRID = 64
WALK_INPUTS = [
    ((300, 1024), BF16),  # 38 units, fast
    ((1, 128), F32),      # 1 unit
    ((257, 1000), F16),   # 33 units; cols % 16 != 0: generic
    ((3, 128), BF16),     # 1 unit
    ((0, 8), BF16),       # empty: no descriptor
    ((64, 4112), F32),    # 33 units, short last block
    ((5, 200), F32),      # 1 unit, generic
    ((200, 2048), BF16),  # 50 units
]


def _walk_units():
    """Unit count per descriptor (empty tensors have none), as plan_quant
    counts them."""
    units = []
    for shape, _ in WALK_INPUTS:
        nblocks = shape[0] * -(-shape[1] // 128)
        if nblocks:
            units.append(-(-nblocks // UNIT_BLOCKS))
    return units


def _check_walk_geometry():
    units = _walk_units()
    assert units == [38, 1, 33, 1, 33, 1, 50]
    total = sum(units)
    assert total > 2 * WALK_GRID  # every workgroup takes at least two trips
    owner = [i for i, n in enumerate(units) for _ in range(n)]
    crossing = []
    for b in range(WALK_GRID):
        trips = [owner[u] for u in range(b, total, WALK_GRID)]
        for a, c in zip(trips, trips[1:]):
            if c > a + 1 and any(units[i] == 1 for i in range(a + 1, c)):
                crossing.append(b)
                break
    # the forward seek with unit >= next_prefix, past a one-unit descriptor
    assert crossing, "no workgroup skips a one-unit descriptor between trips"
    assert any(
        len({owner[u] for u in range(b, total, WALK_GRID)}) == 3
        for b in crossing
    )


@requires_gpu
def test_fp8_unit_walk_under_small_grid(monkeypatch):
    """64 workgroups over 157 units of seven descriptors: each workgroup
    takes two or three trips and re-seeks forward across descriptors,
    skipping one-unit ones; quantise, then dequantise into bf16."""
    _check_walk_geometry()
    monkeypatch.setenv("HIPSTORE_QUANT_GRID", str(WALK_GRID))
    xs = [make_input(shape, dtype) if shape[0] else torch.empty(shape, dtype=dtype)
          for shape, dtype in WALK_INPUTS]
    pairs = _quant_into_arenas([x.to(_dev()) for x in xs])
    live = [(pair, x) for pair, x in zip(pairs, xs) if x.numel()]
    assert len(live) == len(xs) - 1
    for pair, x in live:
        assert_pair_matches(pair, x)

    cpu_pairs = [oracle_quant(x) for _, x in live]
    outs = _dequant_into_arenas(cpu_pairs, BF16)
    for (p, s), out in zip(cpu_pairs, outs):
        assert same_bytes(out, oracle_dequant(p, s, BF16))
