"""The kernels of keyword_pir_client_kernels.hip keep nothing in scratch, spill no register and come in the expected forms; LDS
is used by the staged bucket walk alone, within the budget csrc/keyword_pir_client_plan.hpp states.  Read from the built
object's kernel metadata with the mechanism of tests/test_pir_client_scratch.py; no GPU involved."""
import os

import pytest

import keyword_pir_client_reference as client
import test_kernel_scratch as mechanism
from test_pnns_scratch import _metadata

# kernel: (instantiations, workgroup size of each)
KERNELS = {
    "keyword_client_widen_kernel": [256],
    "keyword_find_staged_kernel": [64, 256],
    "keyword_find_direct_kernel": [256],
    "keyword_find_resolve_kernel": [256],
    "keyword_count_kernel": [64],
}


def test_client_kernels_have_no_scratch_and_only_the_staged_walk_has_lds():
    if not mechanism.library_built():
        pytest.skip("the library's objects are built by __graft_entry__.build()")
    assert os.path.exists(os.path.join(mechanism.BUILD, "keyword_pir_client_kernels.o"))
    rows = _metadata("keyword_pir_client_kernels.o")
    assert len(rows) == sum(len(sizes) for sizes in KERNELS.values()), [name for name, _ in rows]  # nothing else lives there
    for kernel, sizes in KERNELS.items():
        forms = [(name, row) for name, row in rows if name == kernel or name.startswith(kernel + "<") or name.startswith(kernel + "(")]
        assert sorted(row["max_flat_workgroup_size"] for _, row in forms) == sizes, (kernel, forms)
        for name, row in forms:
            assert row["scratch"] == 0, (name, row)
            assert row["spills"] == 0, (name, row)
            if kernel != "keyword_find_staged_kernel":
                assert row["lds"] == 0, (name, row)
    staged = {row["max_flat_workgroup_size"]: row["lds"] for name, row in rows if name.startswith("keyword_find_staged_kernel")}
    # the small instantiation (one wave) and the one of the whole budget: the row limit and the 16 bytes in front of a row
    assert staged == {64: client.STAGED_SMALL_ROW_LIMIT + 16, 256: client.STAGED_ROW_LIMIT + 16}
    assert max(staged.values()) <= client.STAGED_ROW_LIMIT + client.STAGE_PADDING <= 160 * 1024 // 4
