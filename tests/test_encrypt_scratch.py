"""No kernel of encrypt_kernels.hip uses scratch memory (as test_decrypt_scratch.py holds the decryption kernels to it): the 44
round keys of a chunk are wave-uniform and stay in scalar registers, a lane's four draws and the key-switch factors (a
kernel-argument table indexed by the row) stay out of private memory.  Read from the built object's kernel metadata
(bench_tools/kernel_metadata.py); no GPU involved."""
import glob
import os

import pytest

from test_kernel_scratch import BUILD, _kernels


def test_encrypt_kernels_use_no_scratch():
    if not glob.glob(os.path.join(BUILD, "encrypt_kernels.o")):
        pytest.skip("the library's objects are built by __graft_entry__.build()")
    rows = _kernels("encrypt_kernels.o")
    names = {name.split("<")[0] for name, _ in rows}
    assert names == {"sample_ternary_kernel", "sample_binomial_kernel", "encrypt_finish_coeff_kernel", "encrypt_mul_secret_kernel",
                     "encrypt_finish_eval_kernel", "secret_key_square_kernel", "secret_key_galois_kernel"}, sorted(names)
    # seven kernels x two words, the Eval finish with and without the key-switch term
    assert len(rows) == (7 + 1) * 2, rows
    offenders = [(name, scratch) for name, scratch in rows if scratch != 0]
    assert not offenders, offenders


def test_the_uniform_sampler_kept_its_kernels():
    """seeded_kernels.hip shares its AES with the new samplers through a header: its two kernels are still its own."""
    if not glob.glob(os.path.join(BUILD, "seeded_kernels.o")):
        pytest.skip("the library's objects are built by __graft_entry__.build()")
    names = {name.split("<")[0] for name, _ in _kernels("seeded_kernels.o")}
    assert names == {"seeded_chain_kernel", "seeded_stream_kernel"}, sorted(names)
