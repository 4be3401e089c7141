"""The PNNS database kernels (pnns_kernels.hip) keep nothing in scratch and spill no register: the pack kernel's tile lives
in LDS and its loop state in registers for both word sizes.  Read from the built object's kernel metadata with the mechanism
of tests/test_kernel_scratch.py; no GPU involved."""
import os
import subprocess
import sys
import tempfile

import pytest

import test_kernel_scratch as mechanism


def _metadata(obj):
    sys.path.insert(0, os.path.join(mechanism.ROOT, "bench_tools"))
    import kernel_metadata

    with tempfile.TemporaryDirectory() as workdir:
        code = kernel_metadata.code_object(os.path.join(mechanism.BUILD, obj), workdir)
        assert code is not None, obj
        rows = list(kernel_metadata.kernels(code))
        names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True, text=True,
                               check=True).stdout.split("\n")
        return [(kernel_metadata.short_name(name), row) for row, name in zip(rows, names)]


def test_pnns_kernels_keep_nothing_in_scratch_and_spill_nothing():
    if not mechanism.library_built():
        pytest.skip("the library's objects are built by __graft_entry__.build()")
    # where the library is built at all, this object must be there: a renamed or dropped source must not hide the check
    assert os.path.exists(os.path.join(mechanism.BUILD, "pnns_kernels.o"))
    kernels = _metadata("pnns_kernels.o")
    names = [name for name, _ in kernels]
    assert sum(name.startswith("pnns_diagonal_pack_kernel<") for name in names) == 2, names  # 8-byte and 4-byte words
    assert sum(name.startswith("pnns_quantize_rows_kernel") for name in names) == 1, names
    for name, row in kernels:
        assert row["scratch"] == 0, (name, row)
        assert row["spills"] == 0, (name, row)  # vgpr_spill_count of the kernel's metadata note
