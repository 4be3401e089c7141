"""No kernel of the keyword-PIR database build keeps an array in scratch (as test_kernel_scratch.py holds the transforms to it):
the SHA-256 message schedule is a rolling window of 16 words with constant indices, and the candidate indices of
keyword_hash_indices_kernel are a register array under constant indices.  A schedule demoted to scratch would show as hundreds of bytes per lane.
Read from the built object's kernel metadata (bench_tools/kernel_metadata.py); no GPU involved."""
import glob
import os

import pytest

from test_kernel_scratch import BUILD, _kernels


def test_keyword_pir_kernels_keep_no_array_in_scratch():
    if not glob.glob(os.path.join(BUILD, "keyword_pir_kernels.o")):
        pytest.skip("the library's objects are built by __graft_entry__.build()")
    rows = _kernels("keyword_pir_kernels.o")
    names = {name.split("<")[0] for name, _ in rows}
    assert {"keyword_hash_kernel", "keyword_hash_indices_kernel", "keyword_shard_index_kernel",
            "hash_bucket_slot_starts_kernel", "hash_bucket_serialize_kernel"} <= names, sorted(names)
    offenders = [(name, scratch) for name, scratch in rows if scratch > 64]
    assert not offenders, offenders
