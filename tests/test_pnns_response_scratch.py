"""pnns_bsgs_inner_product_kernel (pnns_kernels.hip) keeps nothing in scratch and spills no register in any of its forms, and
its static LDS is nil: the tile of rotated ciphertext rows is dynamic (baby_step x queries x 2 KiB, at most 128 KiB of a
compute unit's 160).  Read from the built object's kernel metadata with the mechanism of tests/test_pnns_scratch.py; no GPU
involved."""
import os

import pytest

import test_kernel_scratch as mechanism
from test_pnns_scratch import _metadata

TILE_LIMIT = 128 << 10


def test_bsgs_inner_product_kernel_has_no_scratch():
    if not mechanism.library_built():
        pytest.skip("the library's objects are built by __graft_entry__.build()")
    assert os.path.exists(os.path.join(mechanism.BUILD, "pnns_kernels.o"))
    kernels = [(name, row) for name, row in _metadata("pnns_kernels.o") if name.startswith("pnns_bsgs_inner_product_kernel<")]
    # 8-byte words: 1..4 queries x (narrow, wide moduli) and the general form; 4-byte words: 1..4 queries and the general form
    assert sum("<unsigned long," in name for name, _ in kernels) == 9, [name for name, _ in kernels]
    assert sum("<unsigned int," in name for name, _ in kernels) == 5, [name for name, _ in kernels]
    for name, row in kernels:
        assert row["scratch"] == 0, (name, row)
        assert row["spills"] == 0, (name, row)
        assert row["lds"] == 0, (name, row)  # static; the dynamic tile is bounded by the launcher
        assert row["max_flat_workgroup_size"] in (256, 512), (name, row)
        # registers leave room for the workgroup: 512 per lane of a SIMD, waves of the workgroup spread over four SIMDs
        assert row["vgpr"] * (row["max_flat_workgroup_size"] // 256) <= 512, (name, row)
    text = open(os.path.join(mechanism.ROOT, "swift-homomorphic-encryption_amd", "csrc", "kernels.hpp")).read()
    assert "kPnnsBsgsTileLimit = size_t(128) << 10" in text and TILE_LIMIT <= 160 << 10
