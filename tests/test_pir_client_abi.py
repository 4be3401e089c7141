"""The MulPIR client entries (he_pir_client_plan, he_pir_evaluation_key_elements, he_pir_generate_query_device,
he_pir_decrypt_response_device and the two workspace sizes) without a device: declared in both headers, exported and mirrored in
Python; every argument error in the documented order -- the word, the context, the shape, null buffers, overlaps -- before the
device is looked at; HE_ERR_DEVICE last on host-only contexts.

HE_ERR_NOT_INVERTIBLE needs a plaintext modulus that shares a factor with 2: of the even numbers only t = 2 makes a context (a
plaintext modulus is a prime), and that one is used."""
import ctypes
import os
import subprocess

import pytest

import heamd
import pir_client_reference as client
from test_pnns_client_abi import HostBfv32, name_of, slab, vp
from test_pnns_response_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["he_pir_client_plan", "he_pir_evaluation_key_elements", "he_pir_generate_query_workspace_bytes",
           "he_pir_generate_query_device", "he_pir_decrypt_response_workspace_bytes", "he_pir_decrypt_response_device"]
N, T17 = 64, 65537
DIMS, COUNT, SIZE = [4, 3], 70, 20  # pack mode with a prefix: six entries per plaintext, twelve plaintexts


@pytest.fixture(scope="module")
def contexts():
    class Contexts:
        one = heamd.BfvContext(N, T17, heamd.generate_primes([40, 40, 41], False, N), host_only=True)
        word32 = HostBfv32(N, T17, heamd.generate_primes([27, 28, 29], False, N))
        two = heamd.BfvContext(N, 2, heamd.generate_primes([40, 40, 41], False, N), host_only=True)

    return Contexts


def dims_of(dimensions):
    return (ctypes.c_uint32 * max(len(dimensions), 1))(*dimensions)


def test_new_entries_are_declared_exported_and_mirrored():
    lib = heamd.load_library()
    declared = declared_functions()
    out = subprocess.run(["nm", "-D", "--defined-only", heamd.binding.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ENTRIES:
        assert name in declared and name in exported and hasattr(lib, name), name
        assert not hasattr(lib, name + "_u32"), name  # the word is an argument
    for name in ("pir_client_plan", "pir_evaluation_key_elements", "pir_generate_query", "pir_decrypt_response",
                 "pir_generate_query_workspace_bytes", "pir_decrypt_response_workspace_bytes"):
        assert callable(getattr(heamd.BfvContext, name))
    with open(os.path.join(ROOT, "include", "he_amd.h")) as ours, \
            open(os.path.join(ROOT, "swift", "Sources", "CHeAmd", "include", "he_amd.h")) as copy:
        assert ours.read() == copy.read()


def test_client_plan(contexts):
    lib = heamd.load_library()
    one = contexts.one

    def plan(ctx=one.h, dimensions=DIMS, count=None, entries=COUNT, size=SIZE, encoding=1, indices=1):
        count = len(dimensions) if count is None else count
        return name_of(lib.he_pir_client_plan(ctx, dims_of(dimensions), count, entries, size, encoding, indices, *[None] * 6))

    assert plan() == "ok"  # every out pointer may be NULL, and no device is needed
    assert plan(ctx=None) == "invalidArgument"
    # he_pir_database_shape's errors
    assert plan(dimensions=[]) == "invalidArgument" and plan(dimensions=[4, 0]) == "invalidArgument"
    assert plan(entries=73) == "invalidArgument"                  # pack mode: 13 plaintexts for 12 slots
    assert plan(size=300, entries=13) == "invalidArgument"        # split mode: 13 entries for 12 rows
    assert plan(size=0, encoding=0) == "invalidArgument"
    assert plan(size=0) == "ok"                                   # (a prefix alone is an entry)
    # the client's own
    assert plan(indices=0) == "invalidArgument"
    assert plan(indices=1 << 20) == "ok" and plan(indices=(1 << 20) + 1) == "invalidArgument"
    assert plan(dimensions=[1] * 16, entries=1) == "ok"
    assert plan(dimensions=[1] * 17, entries=1) == "unsupportedHeOperation"
    assert plan(dimensions=[1] * 17, entries=1, indices=0) == "invalidArgument"  # in argument order behind the shape
    assert plan(dimensions=[1] * 17, entries=7) == "invalidArgument"             # the shape's errors come first
    for dimensions, entries, size, encoding, indices in (([4, 3], 70, 20, True, 1), ([4, 3], 12, 300, True, 3),
                                                         ([40, 30], 7200, 20, True, 2), ([5], 30, 20, False, 60)):
        expected = client.plan(N, T17, dimensions, entries, size, encoding, indices)
        got = one.pir_client_plan(dimensions, entries, size, encoding, indices)
        assert got == {key: expected[key] for key in got}, dimensions
    assert contexts.two.pir_client_plan([4, 3], 12, 20, True)["bytes_per_plaintext"] == 8


def test_evaluation_key_elements_argument_errors():
    lib = heamd.load_library()
    count, out = ctypes.c_size_t(77), (ctypes.c_uint64 * 8)()

    def elements(degree=N, inputs=7, strategy=0, array=out, capacity=8):
        return name_of(lib.he_pir_evaluation_key_elements(degree, inputs, strategy, array, capacity, ctypes.byref(count)))

    assert elements() == "ok" and count.value == 3 and list(out[:3]) == [17, 33, 65]
    assert elements(array=None, capacity=0) == "ok" and count.value == 3  # asking for the count
    assert elements(capacity=2) == "invalidArgument" and count.value == 3
    assert elements(degree=0) == "invalidArgument" and elements(degree=1) == "invalidArgument"
    assert elements(degree=96) == "invalidArgument"
    assert elements(inputs=0) == "invalidArgument"
    assert elements(strategy=-1) == "invalidArgument" and elements(strategy=3) == "invalidArgument"
    assert elements(inputs=1) == "ok" and count.value == 0
    assert name_of(lib.he_pir_evaluation_key_elements(N, 7, 2, out, 8, None)) == "ok"


def test_device_entries_argument_errors(contexts):
    lib = heamd.load_library()
    one = contexts.one

    def query(ctx=one.h, bits=64, dimensions=DIMS, count=None, entries=COUNT, size=SIZE, encoding=1, indices_count=2,
              indices=slab(0), queries=3, key=slab(1), a=slab(2), e=slab(3), out=slab(4), flag=slab(5), workspace=None,
              workspace_bytes=0):
        count = len(dimensions) if count is None else count
        return name_of(lib.he_pir_generate_query_device(ctx, bits, dims_of(dimensions), count, entries, size, encoding,
                                                        indices_count, indices, queries, key, a, e, out, flag, workspace,
                                                        workspace_bytes, None))

    def answer(ctx=one.h, bits=64, dimensions=DIMS, count=None, entries=COUNT, size=SIZE, encoding=1, indices_count=2, moduli=1,
               response=slab(0), indices=slab(6), queries=3, key=slab(1), out=slab(4), sizes=slab(5), workspace=None,
               workspace_bytes=0):
        count = len(dimensions) if count is None else count
        return name_of(lib.he_pir_decrypt_response_device(ctx, bits, dims_of(dimensions), count, entries, size, encoding,
                                                          indices_count, moduli, response, indices, queries, key, out, sizes,
                                                          workspace, workspace_bytes, None))

    for call in (query, answer):
        assert call() == "deviceError"                           # valid: only the device is missing
        assert call(bits=16) == "invalidArgument"
        assert call(bits=16, ctx=None) == "invalidArgument"
        assert call(ctx=None) == "invalidArgument"
        assert call(bits=32) == "invalidArgument"                # a Bfv<UInt64> context
        assert call(ctx=contexts.word32.h) == "deviceError"      # (a Bfv<UInt32> context serves 8-byte slabs too)
        assert call(ctx=contexts.word32.h, bits=32) == "deviceError"
        # the shape, in front of every buffer
        assert call(dimensions=[]) == "invalidArgument" and call(dimensions=[4, 0], out=None) == "invalidArgument"
        assert call(entries=73) == "invalidArgument"
        assert call(indices_count=0) == "invalidArgument"
        assert call(dimensions=[1] * 17, entries=1) == "unsupportedHeOperation"
        assert call(dimensions=[1] * 17, entries=1, key=None) == "unsupportedHeOperation"
        assert call(dimensions=[1] * 16, entries=1) == "deviceError"
        assert call(queries=1 << 40) == "invalidArgument"        # more lanes than one launch holds
        assert call(queries=0) == "ok"                           # an empty batch does nothing
        assert call(queries=0, out=None, key=None) == "ok"
        assert call(queries=0, bits=32) == "invalidArgument"     # ... after the word is checked
        assert call(queries=0, indices_count=0) == "invalidArgument"  # ... and the shape
        # null buffers, then overlaps, then the device
        assert call(key=None) == "invalidArgument"
        assert call(out=None) == "invalidArgument"
        assert call(out=slab(1)) == "invalidArgument"            # the result inside the secret key
        assert b"overlaps" in lib.he_last_error_message()
        assert call(workspace=slab(7), workspace_bytes=1 << 20) == "deviceError"  # (its size is checked with the device's checks)
        assert call(workspace=slab(4), workspace_bytes=64) == "invalidArgument"   # the workspace inside the result
    assert query(indices=None) == "invalidArgument" and query(a=None) == "invalidArgument" and query(e=None) == "invalidArgument"
    assert query(flag=None) == "deviceError"                     # the flag is optional
    assert query(flag=vp(slab(4).value + 8)) == "invalidArgument"  # ... and may not lie in the ciphertexts
    assert query(e=slab(4)) == "invalidArgument"                 # the seeds inside `out`
    assert query(indices=slab(4)) == "invalidArgument"
    # (2^ceilLog2(count))^-1 mod t: t = 2 has none for more than one input, and it is a shape error: in front of the buffers
    assert query(ctx=contexts.two.h, entries=12) == "notInvertible"
    assert query(ctx=contexts.two.h, entries=12, key=None) == "notInvertible"
    assert query(ctx=contexts.two.h, entries=12, indices_count=0) == "invalidArgument"
    assert query(ctx=contexts.two.h, dimensions=[1], entries=1, indices_count=1) == "deviceError"  # one input: 2^0
    assert answer(ctx=contexts.two.h, entries=12) == "deviceError"   # decryption inverts nothing
    assert answer(moduli=0) == "invalidArgument" and answer(moduli=3) == "invalidArgument"
    assert answer(moduli=2) == "deviceError"
    assert answer(response=None) == "invalidArgument"
    assert answer(response=slab(4)) == "invalidArgument"
    assert answer(sizes=None) == "invalidArgument"               # a prefix is decoded: its size has to go somewhere
    assert answer(sizes=None, encoding=0) == "deviceError"
    assert answer(sizes=None, indices=None) == "deviceError"     # decryptFull
    assert answer(sizes=vp(slab(4).value + 8)) == "invalidArgument"
    assert answer(indices=slab(4)) == "invalidArgument"
    assert answer(size=0, out=None) == "deviceError"             # entries of no bytes: sizes alone
    assert lib.he_last_error_message()


def test_workspace_sizes(contexts):
    one = contexts.one
    for dimensions, entries, size, encoding, indices, queries in (([4, 3], 70, 20, True, 1, 1), ([4, 3], 12, 300, True, 3, 2),
                                                                  ([40, 30], 7200, 20, True, 2, 2)):
        p = client.plan(N, T17, dimensions, entries, size, encoding, indices)
        # the plaintexts, then he_bfv_encrypt_device's / he_bfv_decrypt_device's own; every part a multiple of 16 bytes
        count = queries * p["query_ciphertext_count"]
        assert one.pir_generate_query_workspace_bytes(dimensions, entries, size, encoding, indices, queries) == \
            count * N * 8 + one.encrypt_workspace_bytes("encrypt", count)
        replies = queries * indices * p["reply_ciphertext_count"]
        for moduli_count in (1, 2):
            assert one.pir_decrypt_response_workspace_bytes(dimensions, entries, size, encoding, indices, queries, moduli_count) == \
                replies * N * 8 + one.decrypt_workspace_bytes(replies, moduli_count=moduli_count)
    lib = heamd.load_library()
    good = (dims_of(DIMS), 2, COUNT, SIZE, 1, 2)
    assert lib.he_pir_generate_query_workspace_bytes(one.h, 64, *good, 3) > 0
    assert lib.he_pir_decrypt_response_workspace_bytes(one.h, 64, *good, 1, 3) > 0
    # refused arguments
    assert lib.he_pir_generate_query_workspace_bytes(one.h, 32, *good, 3) == 0
    assert lib.he_pir_generate_query_workspace_bytes(None, 64, *good, 3) == 0
    assert lib.he_pir_generate_query_workspace_bytes(one.h, 64, dims_of(DIMS), 2, 73, SIZE, 1, 2, 3) == 0
    assert lib.he_pir_generate_query_workspace_bytes(one.h, 64, dims_of(DIMS), 2, COUNT, SIZE, 1, 0, 3) == 0
    assert lib.he_pir_generate_query_workspace_bytes(contexts.two.h, 64, dims_of(DIMS), 2, 12, SIZE, 1, 2, 3) == 0
    assert lib.he_pir_decrypt_response_workspace_bytes(one.h, 16, *good, 1, 3) == 0
    assert lib.he_pir_decrypt_response_workspace_bytes(one.h, 64, *good, 3, 3) == 0
    assert lib.he_pir_decrypt_response_workspace_bytes(one.h, 64, dims_of([1] * 17), 17, 1, SIZE, 1, 2, 1, 3) == 0
