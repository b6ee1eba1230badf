"""Flat streaming copy kernel and the descriptor ring, bit-exact.

Every destination lies inside a larger buffer between 4 KiB guard bands
that are pre-filled with a sentinel; the whole buffer is compared with an
expected image, so a byte written outside a destination fails the test as
surely as a wrong byte inside it.
"""

import threading

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


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _ext():
    from torchstore_amd.ops import gpu

    return gpu.ext()


def _edge_sizes():
    s = _ext().FLAT_SPAN_DEFAULT
    return [16, s - 16, s, s + 16, 3 * s + 48, 8192, (1 << 20) + 16]


class Plan:
    """Sources, a guarded destination buffer and its expected image."""

    def __init__(self, sizes, src_shift=None):
        dev = torch.device("cuda", 0)
        self.sizes = list(sizes)
        self.offsets = []
        off = GUARD
        for n in self.sizes:
            self.offsets.append(off)
            off = (off + n + GUARD + 15) // 16 * 16
        self.total = off
        g = torch.Generator(device="cpu")
        g.manual_seed(1234 + len(self.sizes))
        shift = src_shift or {}
        self.srcs = []
        for i, n in enumerate(self.sizes):
            k = shift.get(i, 0)
            raw = torch.randint(
                0, 256, (n + 16,), generator=g, dtype=torch.uint8
            ).to(dev)
            self.srcs.append(raw[k:k + n])
        self.expected = torch.full(
            (self.total,), SENTINEL, dtype=torch.uint8, device=dev
        )
        for o, n, s in zip(self.offsets, self.sizes, self.srcs):
            self.expected[o:o + n] = s
        torch.cuda.synchronize()

    def fresh_dst(self):
        return torch.full_like(self.expected, SENTINEL)

    def batch(self, dst):
        base = dst.data_ptr()
        return [(base + o, 0, s.data_ptr(), 0, n)
                for o, n, s in zip(self.offsets, self.sizes, self.srcs)]

    def slices(self, dst):
        base = dst.data_ptr()
        return [(s.data_ptr(), base + o, n, [], [], [])
                for o, n, s in zip(self.offsets, self.sizes, self.srcs)]

    def run(self, api):
        e = _ext()
        dst = self.fresh_dst()
        torch.cuda.synchronize()
        if api == "copy_batch":
            e.copy_batch(self.batch(dst))
        else:
            e.copy_slices(
                self.slices(dst), 0,
                torch.cuda.current_stream().cuda_stream, True,
            )
        torch.cuda.synchronize()
        return dst


@pytest.fixture(scope="module")
def edge_plan():
    return Plan(_edge_sizes())


@requires_gpu
@pytest.mark.parametrize("api", ["copy_batch", "copy_slices"])
def test_span_edges_in_one_launch(edge_plan, api):
    """Sizes around the unit span: descriptor transitions fall inside and
    between blocks; both entry points build flat descriptors."""
    e = _ext()
    before = e.flat_launches()
    dst = edge_plan.run(api)
    assert e.flat_launches() == before + 1, "launch did not go flat"
    assert torch.equal(dst, edge_plan.expected)


@requires_gpu
def test_grid_stride_small_grid(monkeypatch):
    """64 blocks over 4096 units: every block iterates many times and
    crosses descriptors."""
    monkeypatch.setenv("HIPSTORE_GRID", "64")
    mib = 1 << 20
    sizes = [mib + 16, 7 * mib + 4112, 13 * mib - 48, 19 * mib + 16400]
    sizes.append(64 * mib - sum(sizes))
    assert all(n % 16 == 0 and n > 0 for n in sizes)
    plan = Plan(sizes)
    e = _ext()
    before = e.flat_launches()
    dst = plan.run("copy_batch")
    assert e.flat_launches() == before + 1
    assert torch.equal(dst, plan.expected)


@requires_gpu
@pytest.mark.parametrize("api", ["copy_batch", "copy_slices"])
def test_fallback_on_odd_length(api):
    """One entry of length = 2 (mod 16) keeps the whole launch on the
    general kernel; results stay exact."""
    plan = Plan(_edge_sizes() + [4098])
    e = _ext()
    before = e.flat_launches()
    dst = plan.run(api)
    assert e.flat_launches() == before, "odd launch must not go flat"
    assert torch.equal(dst, plan.expected)


@requires_gpu
@pytest.mark.parametrize("api", ["copy_batch", "copy_slices"])
def test_fallback_on_misaligned_source(api):
    sizes = _edge_sizes() + [8192]
    plan = Plan(sizes, src_shift={len(sizes) - 1: 2})
    assert plan.srcs[-1].data_ptr() % 16 == 2
    e = _ext()
    before = e.flat_launches()
    dst = plan.run(api)
    assert e.flat_launches() == before, "misaligned launch must not go flat"
    assert torch.equal(dst, plan.expected)


@requires_gpu
def test_old_and_new_kernel_agree(edge_plan, monkeypatch):
    e = _ext()
    monkeypatch.setenv("HIPSTORE_FLAT", "0")
    before = e.flat_launches()
    old = edge_plan.run("copy_batch")
    assert e.flat_launches() == before, "HIPSTORE_FLAT=0 must force the old kernel"
    monkeypatch.setenv("HIPSTORE_FLAT", "1")
    new = edge_plan.run("copy_batch")
    assert e.flat_launches() == before + 1
    assert torch.equal(old, new)
    assert torch.equal(new, edge_plan.expected)


def _strided_case(n, rows=64, cols=256, c0=32, c1=160):
    """n strided (src_view, dst_view) pairs + guarded expected image."""
    dev = torch.device("cuda", 0)
    src = torch.randn(n, rows, cols, device=dev)
    dst = torch.full((n, rows, cols), -7.0, device=dev)
    exp = dst.clone()
    exp[:, :, c0:c1] = src[:, :, c0:c1]
    pairs = [(src[i, :, c0:c1], dst[i, :, c0:c1]) for i in range(n)]
    return pairs, dst, exp


@requires_gpu
def test_ring_reuse_across_threads():
    """4 threads x 24 copy_batch calls (3x the ring depth), interleaved
    with non-blocking strided launches on the current stream."""
    from torchstore_amd.ops import gpu

    e = _ext()
    dev = torch.device("cuda", 0)
    n_threads, per_thread, region = 4, 3 * e.DESC_RING_SLOTS, 1 << 20
    assert per_thread == 24
    n = n_threads * per_thread
    g = torch.Generator(device="cpu")
    g.manual_seed(77)
    src = torch.randint(
        0, 256, (n, region), generator=g, dtype=torch.uint8
    ).to(dev)
    row = region + 2 * GUARD
    dst = torch.full((n, row), SENTINEL, dtype=torch.uint8, device=dev)
    exp = dst.clone()
    exp[:, GUARD:GUARD + region] = src
    pairs, sdst, sexp = _strided_case(n)
    torch.cuda.synchronize()
    errors = []

    def worker(t):
        try:
            torch.cuda.set_device(0)
            for k in range(per_thread):
                i = t * per_thread + k
                e.copy_batch([(
                    dst[i].data_ptr() + GUARD, 0,
                    src[i].data_ptr(), 0, region,
                )])
                gpu.copy_pairs([pairs[i]], dev, blocking=False)
        except Exception as exc:  # noqa: BLE001 — reported by the main thread
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(t,))
               for t in range(n_threads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not errors, errors
    assert torch.equal(dst, exp)
    assert torch.equal(sdst, sexp)


@requires_gpu
def test_descriptor_growth_behind_running_launches():
    """A batch with far more entries than any earlier one, issued while
    every ring slot still has a non-blocking launch behind it: the slot
    must be waited on before its buffers are regrown."""
    from torchstore_amd.ops import gpu

    e = _ext()
    dev = torch.device("cuda", 0)
    plan = Plan([4096] * 2000)
    dst = plan.fresh_dst()
    pairs, sdst, sexp = _strided_case(
        e.DESC_RING_SLOTS, rows=4096, cols=1024, c0=0, c1=512
    )
    torch.cuda.synchronize()
    for p in pairs:
        gpu.copy_pairs([p], dev, blocking=False)
    before = e.flat_launches()
    e.copy_batch(plan.batch(dst))
    assert e.flat_launches() == before + 1
    torch.cuda.synchronize()
    assert torch.equal(dst, plan.expected)
    assert torch.equal(sdst, sexp)
