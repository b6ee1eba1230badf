"""General slice-copy kernel: wide rows, non-power-of-two packed rows and
the per-wave walk across descriptors, bit-exact against torch's own copy.

As in test_flat_copy.py every destination lies inside one buffer between
4 KiB guard bands pre-filled with a sentinel, and the WHOLE buffer is
compared with an expected image that torch's ``copy_`` filled in, so a byte
written outside a destination (or into the gap between two rows of a strided
one) fails the test as surely as a wrong or missing byte inside.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an AMD GPU"
)

GUARD = 4096
SENTINEL = 0xA5
KNOBS = ("HIPSTORE_FLAT", "HIPSTORE_FLAT_SPAN", "HIPSTORE_GRID",
         "HIPSTORE_NT", "HIPSTORE_FLAT_NTLOAD", "HIPSTORE_TILE")
TILE = 16384        # default tile of a launch below 512 MiB
PACK_SPAN = 65536   # bytes of small rows in one row-packed unit


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


class Arena:
    """Guarded destination buffer + the image torch's own copies produce."""

    def __init__(self, nbytes):
        self.dev = torch.device("cuda", 0)
        self.buf = torch.full((nbytes,), SENTINEL, dtype=torch.uint8,
                              device=self.dev)
        self.exp = self.buf.clone()
        self.off = GUARD
        self.pairs = []
        self.gen = torch.Generator(device="cpu")
        self.gen.manual_seed(4321)

    def region(self, dtype, shape):
        """The same contiguous region of ``buf`` and of ``exp``."""
        n = torch.empty((), dtype=dtype).element_size()
        for s in shape:
            n *= s
        off, self.off = self.off, (self.off + n + GUARD + 15) // 16 * 16
        assert self.off <= self.buf.numel(), "arena too small"
        return tuple(b[off:off + n].view(dtype).view(shape)
                     for b in (self.buf, self.exp))

    def source(self, dtype, shape):
        """Random BYTES seen as ``dtype``: any bit pattern must survive."""
        n = torch.Size(shape).numel() * torch.empty((), dtype=dtype).element_size()
        raw = torch.randint(0, 256, (n,), generator=self.gen, dtype=torch.uint8)
        return raw.view(dtype).view(shape).to(self.dev)

    def add(self, src, dst, exp):
        """Queue src -> dst for the kernel; torch copies it into the image."""
        assert src.shape == dst.shape == exp.shape
        _bytes(exp).copy_(_bytes(src))
        self.pairs.append((src, dst))

    def gather(self, dtype, rows, cols, col0=4):
        """Column slice of a tensor twice as wide -> contiguous rows."""
        src = self.source(dtype, (rows, 2 * cols))[:, col0:col0 + cols]
        dst, exp = self.region(dtype, (rows, cols))
        self.add(src, dst, exp)

    def scatter(self, dtype, rows, cols, col0=4):
        """Contiguous rows -> column slice of a region twice as wide."""
        src = self.source(dtype, (rows, cols))
        dst, exp = self.region(dtype, (rows, 2 * cols))
        self.add(src, dst[:, col0:col0 + cols], exp[:, col0:col0 + cols])

    def run_and_check(self):
        from torchstore_amd.ops import gpu

        e = gpu.ext()
        torch.cuda.synchronize()
        before = e.flat_launches()
        gpu.copy_pairs(self.pairs, self.dev)
        torch.cuda.synchronize()
        assert e.flat_launches() == before, "must take the general kernel"
        wrong = int((self.buf != self.exp).sum())
        assert wrong == 0, f"{wrong} of {self.buf.numel()} bytes differ"


def _bytes(t):
    """Same-shape integer view, so NaN bit patterns copy and compare as data."""
    ints = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
    return t.view(ints[t.element_size()])


def _packed(rows, cols):
    """(rows per unit, units) of a row-packed f32 slice."""
    per_unit = PACK_SPAN // (cols * 4)
    assert per_unit >= 2
    return per_unit, -(-rows // per_unit)


@requires_gpu
@pytest.mark.parametrize("direction", ["gather", "scatter"])
def test_wide_rows(direction):
    """Rows of 32784, 40000 and 65520 bytes — wider than half a pack span,
    so at most one fits a unit and they must keep their tiles — next to a
    32768-byte control that packs two rows per unit."""
    arena = Arena(4 << 20)
    for cols in (8196, 10000, 16380, 8192):
        assert (cols * 4) % 16 == 0 and (2 * cols * 4) % 16 == 0
        getattr(arena, direction)(torch.float32, 5, cols)
    assert _packed(5, 8192) == (2, 3)
    arena.run_and_check()


def _add_odd_packed(arena, direction):
    """Row-packed slices whose rows are 5, 3 and 255 16-byte words (div/mod
    row recovery) and one of 4 words (shift/mask)."""
    move = getattr(arena, direction)
    move(torch.float32, 5, 20)       # 100 words: tail loop only, partial wave
    assert _packed(5, 20) == (819, 1)
    move(torch.float32, 3000, 12)    # unrolled body + tail, short last unit
    assert _packed(3000, 12) == (1365, 3)
    move(torch.float32, 70, 1020)    # 16 rows per unit, short last unit
    assert _packed(70, 1020) == (16, 5)
    move(torch.float32, 64, 16)
    assert _packed(64, 16) == (1024, 1)


@requires_gpu
@pytest.mark.parametrize("direction", ["gather", "scatter"])
def test_non_power_of_two_packed_rows(direction):
    arena = Arena(2 << 20)
    _add_odd_packed(arena, direction)
    arena.run_and_check()


@requires_gpu
def test_wave_walk_crosses_descriptors(monkeypatch):
    """64 blocks = 256 waves over 1013 units of seven descriptors of every
    kind: each wave owns 4 consecutive units, and the order puts the short
    descriptors between the long ones, so chunks start inside one
    descriptor and end in the next (or the one after)."""
    monkeypatch.setenv("HIPSTORE_GRID", "64")
    monkeypatch.setenv("HIPSTORE_FLAT", "0")
    arena = Arena(4 << 20)
    units = []

    arena.gather(torch.float32, 5, 20)
    units.append(1)
    # bf16 3-D view, odd column offset: 66-byte rows on the 2-byte path
    src = arena.source(torch.bfloat16, (30, 20, 40))[:, :, 3:36]
    dst, exp = arena.region(torch.bfloat16, (30, 20, 33))
    assert src.data_ptr() % 4 == 2
    arena.add(src, dst, exp)
    units.append(30 * 20)
    arena.gather(torch.float32, 70, 1020)
    units.append(5)
    # two outer dims: never packed, one unit per 48-byte row
    src = arena.source(torch.float32, (20, 24, 16))[:, 2:22, 4:16]
    dst, exp = arena.region(torch.float32, (20, 20, 12))
    arena.add(src, dst, exp)
    units.append(20 * 20)
    arena.scatter(torch.float32, 3000, 12)
    units.append(3)
    arena.scatter(torch.float32, 64, 16)
    units.append(1)
    # contiguous bytes, odd length and odd source address: byte path, 3 tiles
    n = 2 * TILE + 1001
    src = arena.source(torch.uint8, (n + 1,))[1:]
    dst, exp = arena.region(torch.uint8, (n,))
    assert src.data_ptr() % 2 == 1
    arena.add(src, dst, exp)
    units.append(3)

    total = sum(units)
    assert total == 1013
    chunk = -(-total // 256)
    assert chunk >= 3
    ends, acc = [], 0
    for u in units[:-1]:
        acc += u
        ends.append(acc)
    # every descriptor boundary falls inside a wave's chunk, and one chunk
    # holds two of them
    assert all(e % chunk for e in ends)
    assert len({e // chunk for e in ends}) < len(ends)
    arena.run_and_check()
