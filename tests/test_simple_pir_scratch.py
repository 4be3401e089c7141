"""Every SimplePIR kernel (simple_pir_kernels.hip) keeps nothing in scratch: the reply kernel's per-lane partial sums
(kLaneRows x QT words) and its 16-byte chunks must stay in registers for every element size, word size and request tile.
Read from the built object's kernel metadata with the mechanism of tests/test_kernel_scratch.py; no GPU involved."""
import os

import pytest

import test_kernel_scratch as mechanism


def test_simple_pir_kernels_keep_nothing_in_scratch():
    if not mechanism.library_built():
        pytest.skip("the library's objects are built by __graft_entry__.build()")
    # where the library is built at all, this object must be there: a renamed or dropped source must not hide the check
    assert os.path.exists(os.path.join(mechanism.BUILD, "simple_pir_kernels.o"))
    kernels = mechanism._kernels("simple_pir_kernels.o")
    names = [name for name, _ in kernels]
    # 7 (word, element) pairs x 4 request tiles of the reply kernel, and the process / pack / unpack families
    assert sum(name.startswith("simple_pir_response_kernel<") for name in names) == 28, names
    for family in ("simple_pir_database_kernel<", "simple_pir_widen_kernel<", "simple_pir_hint_mac_kernel",
                   "simple_pir_pack_kernel<", "simple_pir_unpack_kernel<", "simple_pir_replicate_modulus_kernel"):
        assert any(name.startswith(family) for name in names), family
    offenders = [(name, scratch) for name, scratch in kernels if scratch != 0]
    assert not offenders, offenders
