"""The one copy_slices descriptor builder of ops/gpu.py, on CPU tensors
(``data_ptr()`` and strides behave as on a GPU).

Both public paths share it: ``copy_pairs`` (tensor destination) and
``copy_views_to_ptrs`` (contiguous bytes at a raw pointer).  The expected
tuples are spelled out: ``(src_ptr, dst_ptr, row_bytes, outer shape, src
byte strides, dst byte strides)``.
"""

import pytest
import torch

from torchstore_amd.ops import gpu

PTR = 0xD0000000


pair_desc = gpu._slice_desc          # what copy_pairs hands to the kernel


def ptr_desc(src, dst_ptr=PTR):      # what copy_views_to_ptrs hands to it
    return gpu._desc_view_to_ptr(src, dst_ptr)


def test_scalar():
    s, d = torch.zeros((), dtype=torch.float16), torch.zeros((), dtype=torch.float16)
    assert pair_desc(s, d) == (s.data_ptr(), d.data_ptr(), 2, [], [], [])
    assert ptr_desc(s) == (s.data_ptr(), PTR, 2, [], [], [])


def test_empty():
    s = torch.zeros(4, 0)
    assert pair_desc(s, torch.zeros(4, 0)) == ()
    assert ptr_desc(s) == ()
    assert pair_desc(torch.zeros(0), torch.zeros(0)) == ()


def test_contiguous():
    s, d = torch.zeros(8, 6), torch.zeros(8, 6)
    assert pair_desc(s, d) == (s.data_ptr(), d.data_ptr(), 192, [], [], [])
    assert ptr_desc(s) == (s.data_ptr(), PTR, 192, [], [], [])
    # a contiguous source into a strided destination is rows, not flat
    wide = torch.zeros(8, 12)
    dv = wide[:, 3:9]
    assert pair_desc(s, dv) == (s.data_ptr(), dv.data_ptr(), 24, [8], [24], [48])


def test_column_slice_2d():
    big = torch.zeros(8, 12, dtype=torch.bfloat16)
    s = big[2:6, 3:9]
    d = torch.zeros(4, 6, dtype=torch.bfloat16)
    assert s.data_ptr() == big.data_ptr() + (2 * 12 + 3) * 2
    assert pair_desc(s, d) == (s.data_ptr(), d.data_ptr(), 12, [4], [24], [12])
    assert ptr_desc(s) == (s.data_ptr(), PTR, 12, [4], [24], [12])
    # scatter: both sides strided
    big2 = torch.zeros(4, 20, dtype=torch.bfloat16)
    d2 = big2[:, 10:16]
    assert pair_desc(s, d2) == (s.data_ptr(), d2.data_ptr(), 12, [4], [24], [40])


def test_view_3d():
    big = torch.zeros(5, 7, 16)
    s = big[1:4, 2:6, 4:12]  # 3 x 4 x 8
    d = torch.zeros(3, 4, 8)
    want = [3, 4], [7 * 16 * 4, 16 * 4], [4 * 8 * 4, 8 * 4]
    assert pair_desc(s, d) == (s.data_ptr(), d.data_ptr(), 32, *want)
    assert ptr_desc(s) == (s.data_ptr(), PTR, 32, *want)


def test_non_unit_inner_stride_is_rejected():
    a = torch.zeros(8, 6)
    assert pair_desc(a.t(), torch.zeros(6, 8)) is None
    assert pair_desc(torch.zeros(6, 8), a.t()) is None  # destination side
    assert ptr_desc(a.t()) is None
    assert pair_desc(torch.zeros(16)[::2], torch.zeros(8)) is None
    assert ptr_desc(torch.zeros(16)[::2]) is None


def test_shape_or_dtype_mismatch_is_rejected():
    a = torch.zeros(8, 6)
    assert pair_desc(a, torch.zeros(6, 8)) is None
    assert pair_desc(a, torch.zeros(8, 6, dtype=torch.float16)) is None
    assert pair_desc(a, torch.zeros(48)) is None


def test_large_contiguous_source_takes_the_row_form(monkeypatch):
    """Past the flat limit (4 GiB; patched down here) a contiguous source is
    described as rows on BOTH paths instead of one over-long row."""
    assert gpu._FLAT_DESC_MAX_BYTES == 1 << 32
    monkeypatch.setattr(gpu, "_FLAT_DESC_MAX_BYTES", 4096)
    s, d = torch.zeros(3, 20, 32), torch.zeros(3, 20, 32)  # 7680 B
    want = (128, [3, 20], [20 * 128, 128], [20 * 128, 128])
    assert pair_desc(s, d) == (s.data_ptr(), d.data_ptr(), *want)
    assert ptr_desc(s) == (s.data_ptr(), PTR, *want)
    # below the limit both stay flat
    s, d = torch.zeros(1023), torch.zeros(1023)
    assert pair_desc(s, d) == (s.data_ptr(), d.data_ptr(), 4092, [], [], [])
    assert ptr_desc(s) == (s.data_ptr(), PTR, 4092, [], [], [])
    # at the limit: rows
    s = torch.zeros(4, 256)
    assert ptr_desc(s) == (s.data_ptr(), PTR, 1024, [4], [1024], [1024])


def test_rejects_and_fallbacks_without_a_launch(monkeypatch):
    """Pairs the kernel cannot express fall back to ``copy_``; views are
    handed back.  No descriptor is left, so the extension is never asked."""
    monkeypatch.setattr(gpu, "ext", lambda: pytest.fail("no launch expected"))
    dev = torch.device("cpu")
    a = torch.arange(48.0).reshape(8, 6)
    out = torch.zeros(6, 8)
    gpu.copy_pairs([(a.t(), out), (torch.zeros(0), torch.zeros(0))], dev)
    assert torch.equal(out, a.t())
    items = [(a.t(), PTR), (torch.zeros(0), PTR)]
    rejects = gpu.copy_views_to_ptrs(items, dev)
    assert len(rejects) == 1 and rejects[0] is items[0]
