"""pnns_row_mask_kernel and pnns_extract_rows_kernel (pnns_kernels.hip) keep nothing in scratch, spill no register and use no
LDS in any of their forms.  Read from the built object's kernel metadata with the mechanism of tests/test_pnns_scratch.py; no
GPU involved."""
import os

import pytest

import test_kernel_scratch as mechanism
from test_pnns_scratch import _metadata


def test_row_mask_and_extract_kernels_have_no_scratch():
    if not mechanism.library_built():
        pytest.skip("the library's objects are built by __graft_entry__.build()")
    assert os.path.exists(os.path.join(mechanism.BUILD, "pnns_kernels.o"))
    rows = _metadata("pnns_kernels.o")
    masks = [(name, row) for name, row in rows if name.startswith("pnns_row_mask_kernel<")]
    extract = [(name, row) for name, row in rows if name.startswith("pnns_extract_rows_kernel<")]
    assert len(masks) == 2, [name for name, _ in masks]     # 8- and 4-byte words
    assert len(extract) == 4, [name for name, _ in extract]  # x (wave-uniform modulus, per-lane modulus)
    for name, row in masks + extract:
        assert row["scratch"] == 0, (name, row)
        assert row["spills"] == 0, (name, row)
        assert row["lds"] == 0, (name, row)
        assert row["max_flat_workgroup_size"] == 256, (name, row)
