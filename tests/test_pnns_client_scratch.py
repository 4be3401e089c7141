"""The kernels of pnns_client_kernels.hip keep nothing in scratch, spill no register, use no LDS and come in the expected
number of forms.  Read from the built object's kernel metadata with the mechanism of tests/test_pnns_scratch.py; no GPU involved."""
import os

import pytest

import test_kernel_scratch as mechanism
from test_pnns_scratch import _metadata

KERNELS = ["pnns_simd_scatter_kernel", "pnns_simd_gather_kernel", "pnns_dense_row_pack_kernel", "pnns_unpack_kernel",
           "pnns_compose_distances_kernel"]


def test_client_kernels_have_no_scratch():
    if not mechanism.library_built():
        pytest.skip("the library's objects are built by __graft_entry__.build()")
    assert os.path.exists(os.path.join(mechanism.BUILD, "pnns_client_kernels.o"))
    rows = _metadata("pnns_client_kernels.o")
    assert len(rows) == 2 * len(KERNELS), [name for name, _ in rows]  # nothing else lives in the object
    for kernel in KERNELS:
        forms = [(name, row) for name, row in rows if name.startswith(kernel + "<")]
        assert len(forms) == 2, (kernel, [name for name, _ in forms])  # 8- and 4-byte words
        for name, row in forms:
            assert row["scratch"] == 0, (name, row)
            assert row["spills"] == 0, (name, row)
            assert row["lds"] == 0, (name, row)
            assert row["max_flat_workgroup_size"] == 256, (name, row)
