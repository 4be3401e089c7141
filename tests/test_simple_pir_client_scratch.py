"""The kernels of simple_pir_client_kernels.hip keep nothing in scratch, spill no register and come in the expected forms; the
hint product's LDS is what he_simple_pir_client_plan states, and the finishing kernel's is the AES table alone.  Read from the
built object's kernel metadata with the mechanism of tests/test_pnns_scratch.py; no GPU involved."""
import os

import pytest

import simple_pir_client_reference as C
import test_kernel_scratch as mechanism
from test_pnns_scratch import _metadata

# kernel -> forms per slab word
KERNELS = {
    "simple_pir_client_widen_kernel": 1, "simple_pir_client_products_kernel": 1,
    "simple_pir_client_finish_kernel": 2,        # one and two counter blocks per coefficient: stdDev32, stdDev64
    "simple_pir_client_pack_codes_kernel": 1,
    "simple_pir_client_hint_product_kernel": 2,  # 16-byte loads, and single words where N is no multiple of a load
    "simple_pir_client_add_indices_kernel": 1, "simple_pir_client_integrate_kernel": 1, "simple_pir_client_entry_bytes_kernel": 1,
}


def test_client_kernels_have_no_scratch():
    if not mechanism.library_built():
        pytest.skip("the library's objects are built by __graft_entry__.build()")
    assert os.path.exists(os.path.join(mechanism.BUILD, "simple_pir_client_kernels.o"))
    rows = _metadata("simple_pir_client_kernels.o")
    assert len(rows) == 2 * sum(KERNELS.values()), [name for name, _ in rows]  # nothing else lives in the object
    import heamd

    planned = heamd.simple_pir_client_plan(14, 42, 1024, 600, 20)["hint_product_lds_bytes"]
    assert planned == C.SECRET_ROWS_PER_PASS * 256 + C.SECRET_ROWS_PER_PASS * C.HINT_TILE_ROWS * 8  # N = 1024: 256 bytes of codes a row
    for kernel, count in KERNELS.items():
        forms = [(name, row) for name, row in rows if name.startswith(kernel + "<")]
        assert len(forms) == 2 * count, (kernel, [name for name, _ in forms])  # 8- and 4-byte words
        for name, row in forms:
            assert row["scratch"] == 0, (name, row)
            assert row["spills"] == 0, (name, row)
            if kernel == "simple_pir_client_hint_product_kernel":
                assert row["lds"] == planned, (name, row)
            elif kernel == "simple_pir_client_finish_kernel":
                assert row["lds"] == 16 * 256 * 4, (name, row)  # sixteen interleaved copies of the AES T-table
            else:
                assert row["lds"] == 0, (name, row)
            assert row["max_flat_workgroup_size"] == 256, (name, row)
