"""No kernel of decrypt_kernels.hip keeps an array in scratch (as test_keyword_shard_scratch.py holds the partition kernels to
it): the mixed-radix digits of the norm kernel -- up to 16 of a coefficient, 16 of the running maximum and 16 limbs -- and the
words of a dot-product lane are indexed at compile time and stay in registers.  Read from the built object's kernel metadata
(bench_tools/kernel_metadata.py); no GPU involved."""
import glob
import os

import pytest

from test_kernel_scratch import BUILD, _kernels


def test_decrypt_kernels_keep_no_array_in_scratch():
    if not glob.glob(os.path.join(BUILD, "decrypt_kernels.o")):
        pytest.skip("the library's objects are built by __graft_entry__.build()")
    rows = _kernels("decrypt_kernels.o")
    names = {name.split("<")[0] for name, _ in rows}
    assert {"secret_dot_product_kernel", "add_first_polynomial_kernel", "noise_norm_kernel", "is_transparent_kernel"} <= names, \
        sorted(names)
    # dot product: 1..3 polynomials with c0 and 2..3 without, x (16 bytes per lane, one word per lane) x two words; norm: 1..16
    # moduli x two words; the addition of c0 and transparency: the two access widths x two words each
    assert len(rows) == (3 + 2) * 2 * 2 + 16 * 2 + 2 * 2 + 2 * 2, rows
    offenders = [(name, scratch) for name, scratch in rows if scratch > 64]
    assert not offenders, offenders
