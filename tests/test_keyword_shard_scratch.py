"""No kernel of the database partition keeps an array in scratch (as test_keyword_pir_scratch.py holds the keyword kernels to
it): the four elements a lane scans and the rows a gather lane walks stay in registers.  Read from the built object's kernel
metadata (bench_tools/kernel_metadata.py); no GPU involved."""
import glob
import os

import pytest

from test_kernel_scratch import BUILD, _kernels


def test_keyword_shard_kernels_keep_no_array_in_scratch():
    if not glob.glob(os.path.join(BUILD, "keyword_shard_kernels.o")):
        pytest.skip("the library's objects are built by __graft_entry__.build()")
    rows = _kernels("keyword_shard_kernels.o")
    names = {name.split("<")[0] for name, _ in rows}
    assert {"scan_reduce_kernel", "scan_apply_kernel", "shard_digit_count_kernel", "shard_digit_scatter_kernel",
            "identity_order_kernel", "shard_starts_kernel", "row_lengths_kernel", "gather_tile_rows_kernel", "blob_gather_kernel",
            "gather_words_kernel"} <= names, sorted(names)
    assert len(rows) == 12, rows  # both scan kernels at 4 and at 8 bytes
    offenders = [(name, scratch) for name, scratch in rows if scratch > 64]
    assert not offenders, offenders
