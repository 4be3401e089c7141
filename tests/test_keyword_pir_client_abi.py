"""The keyword-PIR client entries (he_keyword_client_plan, he_keyword_client_generate_query_device,
he_keyword_client_find_in_buckets_device, he_keyword_client_decrypt_response_device, he_keyword_client_count_entries_device, their
workspace sizes and he_keyword_client_count_bucket_entries_device) without a device: declared in both headers, exported and
mirrored in Python; the plan's values and every error; every argument error of the device entries in the documented order --
the word, the context, the shape, null buffers, overlaps -- before the device is looked at, HE_ERR_DEVICE last on host-only
contexts; workspace sizes zero on refused arguments and monotone in the batch."""
import ctypes
import os
import subprocess

import pytest

import heamd
import keyword_pir_client_reference as client
from test_pnns_client_abi import HostBfv32, name_of, slab, vp
from test_pnns_response_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["he_keyword_client_plan", "he_keyword_client_generate_query_workspace_bytes", "he_keyword_client_generate_query_device",
           "he_keyword_client_find_in_buckets_workspace_bytes", "he_keyword_client_find_in_buckets_device",
           "he_keyword_client_decrypt_response_workspace_bytes", "he_keyword_client_decrypt_response_device",
           "he_keyword_client_count_entries_workspace_bytes", "he_keyword_client_count_entries_device",
           "he_keyword_client_count_bucket_entries_device"]
N, T17 = 64, 65537
DIMS, COUNT, SIZE, H = [4, 3], 70, 20, 2  # pack mode: six buckets per plaintext, twelve plaintexts


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
    for cls in (heamd.BfvContext, heamd.BfvContext32):
        for name in ("keyword_pir_client_plan", "keyword_pir_generate_query", "keyword_pir_find_in_buckets",
                     "keyword_pir_decrypt_response", "keyword_pir_count_entries", "keyword_pir_count_bucket_entries",
                     "keyword_pir_generate_query_workspace_bytes", "keyword_pir_decrypt_response_workspace_bytes",
                     "keyword_pir_count_entries_workspace_bytes"):
            assert callable(getattr(cls, name)), name
    with open(os.path.join(ROOT, "include", "he_amd.h")) as ours, \
            open(os.path.join(ROOT, "swift", "Sources", "CHeAmd", "include", "he_amd.h")) as copy:
        assert ours.read() == copy.read()


def test_client_plan(contexts):
    lib = heamd.load_library()
    one = contexts.one

    def plan(ctx=one.h, dimensions=DIMS, count=None, entries=COUNT, size=SIZE, h=H):
        count = len(dimensions) if count is None else count
        return name_of(lib.he_keyword_client_plan(ctx, dims_of(dimensions), count, entries, size, h, *[None] * 9))

    assert plan() == "ok"  # every out pointer may be NULL, and no device is needed
    assert plan(ctx=None) == "invalidArgument"
    # he_pir_client_plan's errors
    assert plan(dimensions=[]) == "invalidArgument" and plan(dimensions=[4, 0]) == "invalidArgument"
    assert plan(entries=73) == "invalidArgument"                  # pack mode: 13 plaintexts for 12 slots
    assert plan(size=300, entries=13) == "invalidArgument"        # split mode: 13 buckets for 12 rows
    assert plan(dimensions=[1] * 17, entries=1) == "unsupportedHeOperation"
    # the keyword client's own
    assert plan(h=0) == "invalidArgument"
    assert plan(h=8) == "ok" and plan(h=9) == "unsupportedHeOperation"
    assert plan(h=9, entries=73) == "invalidArgument"             # the shape's errors come first
    assert plan(size=0) == "invalidArgument"                      # "Serialized HashBucket shouldn't be empty"
    assert plan(size=0, h=9) in ("invalidArgument", "unsupportedHeOperation")
    assert plan(entries=0) == "invalidArgument"                   # hashIndices takes a bucket count
    assert plan(size=1) == "ok" and plan(size=10) == "ok"
    for dimensions, entries, size, h in (([4, 3], 70, 20, 2), ([4, 3], 12, 332, 2), ([5], 30, 20, 3), ([4, 3], 12, 128, 1),
                                         ([40, 30], 1200, 33000, 8), ([4, 3], 12, 65546, 2), ([4, 3], 12, 65547, 2),
                                         ([4, 3], 120, 11, 1), ([4, 3], 120, 12, 1), ([4, 3], 120, 10, 1), ([4, 3], 1500, 1, 1),
                                         ([4, 3], 12, 32768, 2), ([4, 3], 12, 32769, 2)):
        expected = client.plan(N, T17, dimensions, entries, size, h)
        got = one.keyword_pir_client_plan(dimensions, entries, size, h)
        assert got == {key: expected[key] for key in got}, (dimensions, size)
        assert set(got) >= {"value_capacity", "find_form", "staged_lds_bytes", "reply_bytes", "query_ciphertext_count"}
    # the form threshold and the capacity at the issue's sizes
    capacities = {size: one.keyword_pir_client_plan([4, 3], 12 if size > 128 else 1, size, 1)["value_capacity"]
                  for size in (1, 10, 11, 12, 65546, 65547)}
    assert capacities == {1: 0, 10: 0, 11: 0, 12: 1, 65546: 65535, 65547: 65535}
    assert one.keyword_pir_client_plan([4, 3], 12, 32768, 2)["find_form"] == "staged"
    assert one.keyword_pir_client_plan([4, 3], 12, 32769, 2)["find_form"] == "direct"


def test_device_entries_argument_errors(contexts):
    lib = heamd.load_library()
    one = contexts.one

    def query(ctx=one.h, bits=64, dimensions=DIMS, count=None, entries=COUNT, size=SIZE, h=H, keywords=slab(0), offsets=slab(8),
              queries=3, key=slab(1), a=slab(2), e=slab(3), out=slab(4), hashes=slab(5), workspace=None, workspace_bytes=0):
        count = len(dimensions) if count is None else count
        return name_of(lib.he_keyword_client_generate_query_device(ctx, bits, dims_of(dimensions), count, entries, size, h, keywords,
                                                                offsets, queries, key, a, e, out, hashes, workspace,
                                                                workspace_bytes, None))

    def answer(ctx=one.h, bits=64, dimensions=DIMS, count=None, entries=COUNT, size=SIZE, h=H, moduli=1, response=slab(0),
               keywords=slab(6), offsets=slab(8), hashes=None, queries=3, key=slab(1), out=slab(4), sizes=slab(5),
               status=slab(9), workspace=None, workspace_bytes=0):
        count = len(dimensions) if count is None else count
        return name_of(lib.he_keyword_client_decrypt_response_device(ctx, bits, dims_of(dimensions), count, entries, size, h, moduli,
                                                                  response, keywords, offsets, hashes, queries, key, out, sizes,
                                                                  status, workspace, workspace_bytes, None))

    def tally(ctx=one.h, bits=64, dimensions=DIMS, count=None, entries=COUNT, size=SIZE, h=H, moduli=1, response=slab(0),
              queries=3, key=slab(1), out=slab(4), workspace=None, workspace_bytes=0):
        count = len(dimensions) if count is None else count
        return name_of(lib.he_keyword_client_count_entries_device(ctx, bits, dims_of(dimensions), count, entries, size, h, moduli,
                                                               response, queries, key, out, workspace, workspace_bytes, None))

    for call in (query, answer, tally):
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
        assert call(h=0) == "invalidArgument"
        assert call(h=9) == "unsupportedHeOperation" and call(h=9, key=None) == "unsupportedHeOperation"
        assert call(h=8) == "deviceError"
        assert call(size=0) == "invalidArgument" and call(entries=0) == "invalidArgument"
        assert call(dimensions=[1] * 17, entries=1) == "unsupportedHeOperation"
        assert call(queries=1 << 40) == "invalidArgument"        # more than one call holds
        assert call(queries=0) == "ok"                           # an empty batch does nothing
        assert call(queries=0, out=None, key=None) == "ok"
        assert call(queries=0, bits=32) == "invalidArgument"     # ... after the word is checked
        assert call(queries=0, h=0) == "invalidArgument"         # ... and the shape
        # null buffers, then overlaps, then the device
        assert call(key=None) == "invalidArgument"
        assert call(out=None) == "invalidArgument"
        assert call(out=slab(1)) == "invalidArgument"            # the result inside the secret key
        assert b"overlaps" in lib.he_last_error_message()
        assert call(workspace=slab(7), workspace_bytes=1 << 20) == "deviceError"  # (its size is checked with the device's checks)
        assert call(workspace=slab(4), workspace_bytes=64) == "invalidArgument"   # the workspace inside the result
    assert query(keywords=None) == "invalidArgument" and query(offsets=None) == "invalidArgument"
    assert query(a=None) == "invalidArgument" and query(e=None) == "invalidArgument"
    assert query(hashes=None) == "deviceError"                   # the hashes are optional
    assert query(hashes=vp(slab(4).value + 8)) == "invalidArgument"  # ... and may not lie in the ciphertexts
    assert query(e=slab(4)) == "invalidArgument" and query(offsets=slab(4)) == "invalidArgument"
    assert query(keywords=slab(4)) == "invalidArgument"          # (the first byte of the blob)
    assert query(ctx=contexts.two.h, entries=12) == "notInvertible"      # a shape error of the index-PIR client
    assert query(ctx=contexts.two.h, entries=12, key=None) == "notInvertible"
    assert query(ctx=contexts.two.h, entries=12, h=0) == "invalidArgument"
    for call in (answer, tally):
        assert call(ctx=contexts.two.h, entries=12) == "deviceError"     # decryption inverts nothing
        assert call(moduli=0) == "invalidArgument" and call(moduli=3) == "invalidArgument"
        assert call(moduli=2) == "deviceError"
        assert call(response=None) == "invalidArgument"
        assert call(response=slab(4)) == "invalidArgument"
    assert answer(keywords=None) == "invalidArgument"            # neither keywords nor hashes
    assert answer(keywords=None, hashes=slab(6)) == "deviceError"
    assert answer(keywords=None, offsets=None, hashes=slab(6)) == "deviceError"
    assert answer(offsets=None) == "invalidArgument"
    assert answer(sizes=None) == "invalidArgument" and answer(status=None) == "invalidArgument"
    assert answer(status=vp(slab(4).value + 8)) == "invalidArgument"
    assert answer(sizes=vp(slab(4).value + 8)) == "invalidArgument"
    assert answer(keywords=None, hashes=slab(4)) == "invalidArgument"
    assert answer(size=10, entries=120, out=None) == "deviceError"   # rows that hold no value: status and sizes alone
    assert answer(size=11, entries=120, out=None) == "deviceError"
    assert answer(size=12, entries=120, out=None) == "invalidArgument"
    assert lib.he_last_error_message()


def test_bytes_level_entries_argument_errors():
    lib = heamd.load_library()

    def find(buckets=slab(0), hashes=slab(1), size=64, h=2, queries=3, form=-1, values=slab(2), sizes=slab(3), status=slab(4),
             workspace=slab(5), workspace_bytes=1 << 20):
        return name_of(lib.he_keyword_client_find_in_buckets_device(buckets, hashes, size, h, queries, form, values, sizes, status,
                                                                 workspace, workspace_bytes, None))

    # the shape first
    assert find(h=0) == "invalidArgument" and find(h=0, buckets=None) == "invalidArgument"
    assert find(h=9) == "unsupportedHeOperation" and find(h=9, buckets=None) == "unsupportedHeOperation"
    assert find(size=0) == "invalidArgument"
    assert find(size=(1 << 48) + 1, queries=1) == "invalidArgument"
    assert find(form=-2) == "invalidArgument" and find(form=2) == "invalidArgument"
    assert find(form=0, size=client.STAGED_ROW_LIMIT + 1) == "invalidArgument"   # too long a row for the staged form
    assert find(queries=1 << 40) == "invalidArgument"
    assert find(queries=1 << 31, size=1 << 40) == "invalidArgument"              # the row bytes would wrap
    assert find(queries=0) == "ok" and find(queries=0, buckets=None, status=None) == "ok"
    assert find(queries=0, h=0) == "invalidArgument"
    # null buffers, then overlaps.  (These two entries take no context: a call that passes every check is launched, so none
    # is made here with addresses that are nobody's.)
    for name in ("buckets", "hashes", "values", "sizes", "status"):
        assert find(**{name: None}) == "invalidArgument", name
    assert find(values=vp(slab(0).value + 8)) == "invalidArgument" and b"overlaps" in lib.he_last_error_message()
    assert find(status=slab(1)) == "invalidArgument"
    assert find(workspace=slab(2), workspace_bytes=64) == "invalidArgument"
    assert find(workspace=vp(slab(5).value + 8)) == "invalidArgument"            # not 16-byte aligned
    assert find(workspace_bytes=3 * 2 * 16 - 16) == "invalidArgument"            # 16 bytes short

    def count(data=slab(0), reply_bytes=100, replies=2, queries=3, out=slab(1)):
        return name_of(lib.he_keyword_client_count_bucket_entries_device(data, reply_bytes, replies, queries, out, None))

    assert count(queries=1 << 40) == "invalidArgument" and count(replies=1 << 40) == "invalidArgument"
    assert count(reply_bytes=(1 << 48) + 1) == "invalidArgument"
    assert count(queries=1 << 31, replies=1 << 31, reply_bytes=1 << 20) == "invalidArgument"
    assert count(queries=0) == "ok" and count(queries=0, out=None) == "ok"
    assert count(out=None) == "invalidArgument" and count(data=None) == "invalidArgument"
    assert count(out=vp(slab(0).value + 16)) == "invalidArgument"


def test_workspace_sizes(contexts):
    one, lib = contexts.one, heamd.load_library()
    for dimensions, entries, size, h in (([4, 3], 70, 20, 2), ([4, 3], 12, 332, 3), ([5], 30, 20, 1)):
        p = client.plan(N, T17, dimensions, entries, size, h)
        sizes = []
        for queries in (1, 2, 5):
            r16 = lambda value: (value + 15) // 16 * 16  # noqa: E731
            index = r16(8 * queries) + r16(4 * queries * h) + r16(8 * queries * h)
            got = one.keyword_pir_generate_query_workspace_bytes(dimensions, entries, size, h, queries)
            assert got == index + one.pir_generate_query_workspace_bytes(dimensions, entries, size, False, h, queries)
            for moduli_count in (1, 2):
                nested = one.pir_decrypt_response_workspace_bytes(dimensions, entries, size, False, h, queries, moduli_count)
                assert one.keyword_pir_decrypt_response_workspace_bytes(dimensions, entries, size, h, queries, moduli_count) == \
                    index + r16(queries * h * size) + r16(queries * h * 16) + nested
                assert one.keyword_pir_count_entries_workspace_bytes(dimensions, entries, size, h, queries, moduli_count) == \
                    r16(queries * h * p["reply_bytes"]) + nested
            assert lib.he_keyword_client_find_in_buckets_workspace_bytes(size, h, queries) == r16(queries * h * 16)
            sizes.append((got, one.keyword_pir_decrypt_response_workspace_bytes(dimensions, entries, size, h, queries),
                          one.keyword_pir_count_entries_workspace_bytes(dimensions, entries, size, h, queries)))
        assert sizes == sorted(sizes) and len(set(sizes)) == 3  # monotone in the batch, entry by entry
        assert all(a < b for first, second in zip(sizes, sizes[1:]) for a, b in zip(first, second))
    good = (dims_of(DIMS), 2, COUNT, SIZE, H)
    assert lib.he_keyword_client_generate_query_workspace_bytes(one.h, 64, *good, 3) > 0
    assert lib.he_keyword_client_decrypt_response_workspace_bytes(one.h, 64, *good, 1, 3) > 0
    assert lib.he_keyword_client_count_entries_workspace_bytes(one.h, 64, *good, 1, 3) > 0
    # refused arguments
    assert lib.he_keyword_client_generate_query_workspace_bytes(one.h, 32, *good, 3) == 0
    assert lib.he_keyword_client_generate_query_workspace_bytes(None, 64, *good, 3) == 0
    assert lib.he_keyword_client_generate_query_workspace_bytes(one.h, 64, dims_of(DIMS), 2, 73, SIZE, H, 3) == 0
    assert lib.he_keyword_client_generate_query_workspace_bytes(one.h, 64, dims_of(DIMS), 2, COUNT, SIZE, 0, 3) == 0
    assert lib.he_keyword_client_generate_query_workspace_bytes(one.h, 64, dims_of(DIMS), 2, COUNT, SIZE, 9, 3) == 0
    assert lib.he_keyword_client_generate_query_workspace_bytes(contexts.two.h, 64, dims_of(DIMS), 2, 12, SIZE, H, 3) == 0
    for sized in (lib.he_keyword_client_decrypt_response_workspace_bytes, lib.he_keyword_client_count_entries_workspace_bytes):
        assert sized(one.h, 16, *good, 1, 3) == 0
        assert sized(one.h, 64, *good, 3, 3) == 0
        assert sized(one.h, 64, dims_of(DIMS), 2, COUNT, 0, H, 1, 3) == 0
        assert sized(one.h, 64, dims_of(DIMS), 2, COUNT, SIZE, 9, 1, 3) == 0
    assert lib.he_keyword_client_find_in_buckets_workspace_bytes(0, 2, 3) == 0
    assert lib.he_keyword_client_find_in_buckets_workspace_bytes(64, 0, 3) == 0
    assert lib.he_keyword_client_find_in_buckets_workspace_bytes(64, 9, 3) == 0
