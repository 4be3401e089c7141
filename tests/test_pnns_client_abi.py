"""The PNNS client entries (he_pnns_simd_encode/decode_device, he_pnns_pack_dense_rows_device, he_pnns_unpack_device,
he_pnns_generate_query_device, he_pnns_decrypt_response_device and the two workspace sizes) without a device: declared in both
headers, exported and mirrored in Python; every argument error in the documented order -- the word, the context(s), the shape,
null buffers, overlaps -- before the device is looked at; HE_ERR_DEVICE last on host-only contexts; HE_ERR_UNSUPPORTED for the
packings left out."""
import ctypes
import os
import subprocess

import pytest

import heamd
import pnns_reference as pnns
from test_pnns_response_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["he_pnns_simd_encode_device", "he_pnns_simd_decode_device", "he_pnns_pack_dense_rows_device", "he_pnns_unpack_device",
           "he_pnns_generate_query_workspace_bytes", "he_pnns_generate_query_device", "he_pnns_decrypt_response_workspace_bytes",
           "he_pnns_decrypt_response_device"]
N = 64
T17, T17B = 65537, 114689
vp = ctypes.c_void_p


def slab(k):
    """distinct addresses far apart, 16-byte aligned, never dereferenced"""
    return vp(0x10000000 * (k + 1))


def name_of(status):
    return heamd.binding.STATUS_NAMES[status]


class HostBfv32:
    """a host-only Context<Bfv<UInt32>>: what PnnsContext reads of a BfvContext32 (whose constructor wants a device)"""

    word_bits = 32

    def __init__(self, degree, t, moduli):
        lib = heamd.load_library()
        self.h, self.degree, self.t = vp(), degree, t
        moduli = (ctypes.c_uint64 * len(moduli))(*moduli)
        assert lib.he_bfv_context_create_u32_host_only(degree, t, moduli, len(moduli), ctypes.byref(self.h)) == 0

    def __del__(self):
        heamd.load_library().he_bfv_context_destroy(self.h)


def host_bfv(t=T17, degree=N, bits=(40, 40, 41), word32=False):
    if word32:
        return HostBfv32(degree, t, heamd.generate_primes([27, 28, 29], False, degree))
    return heamd.BfvContext(degree, t, heamd.generate_primes(list(bits), False, degree), host_only=True)


@pytest.fixture(scope="module")
def contexts():
    class Contexts:
        one = heamd.PnnsContext(host_bfv())
        other = heamd.PnnsContext(host_bfv(T17B))
        same_t = heamd.PnnsContext(host_bfv())
        other_degree = heamd.PnnsContext(host_bfv(T17B, degree=1024))
        other_moduli = heamd.PnnsContext(host_bfv(T17B, bits=(40, 41, 41)))
        word32 = heamd.PnnsContext(host_bfv(T17B, word32=True))
        wide = [heamd.PnnsContext(host_bfv(t)) for t in heamd.generate_primes([32, 32, 32], False, N)[:2]]

    return Contexts


def test_new_entries_are_declared_exported_and_mirrored():
    lib = heamd.load_library()
    declared = declared_functions()
    out = subprocess.run(["nm", "-D", "--defined-only", heamd.binding.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ENTRIES:
        assert name in declared and name in exported and hasattr(lib, name), name
    for name in ("simd_encode", "simd_decode", "pack_dense_rows", "unpack"):
        assert callable(getattr(heamd.PnnsContext, name))
    for name in ("pnns_generate_query", "pnns_decrypt_response", "pnns_generate_query_workspace_bytes",
                 "pnns_decrypt_response_workspace_bytes"):
        assert callable(getattr(heamd, name))
    with open(os.path.join(ROOT, "include", "he_amd.h")) as ours, \
            open(os.path.join(ROOT, "swift", "Sources", "CHeAmd", "include", "he_amd.h")) as copy:
        assert ours.read() == copy.read()


def test_simd_encode_and_decode_argument_errors(contexts):
    lib = heamd.load_library()
    h = contexts.one.h

    def encode(ctx=h, bits=64, slots=slab(0), batch=3, out=slab(1), flag=slab(2)):
        return name_of(lib.he_pnns_simd_encode_device(ctx, bits, slots, batch, out, flag, None))

    def decode(ctx=h, bits=64, plaintexts=slab(0), batch=3, out=slab(1)):
        return name_of(lib.he_pnns_simd_decode_device(ctx, bits, plaintexts, batch, out, None))

    for call in (encode, decode):
        assert call() == "deviceError"  # valid: only the device is missing
        assert call(bits=16) == "invalidArgument"
        assert call(bits=16, ctx=None) == "invalidArgument"
        assert call(ctx=None) == "invalidArgument"
        assert call(bits=32) == "invalidArgument"               # a Bfv<UInt64> context
        assert call(ctx=contexts.word32.h) == "invalidArgument"  # a Bfv<UInt32> context
        assert call(ctx=contexts.word32.h, bits=32) == "deviceError"
        assert call(batch=0) == "ok"
        assert call(batch=0, out=None) == "ok"                   # an empty batch does nothing
        assert call(bits=32, batch=0) == "invalidArgument"       # ... after the word is checked
        assert call(batch=1 << 41) == "invalidArgument"
        assert call(out=None) == "invalidArgument"
        assert call(out=slab(0)) == "invalidArgument"            # in place: the gather reads every word of a plaintext
    assert encode(slots=None) == "invalidArgument" and decode(plaintexts=None) == "invalidArgument"
    assert encode(flag=None) == "deviceError"                    # the flag is optional
    assert encode(flag=vp(slab(1).value + 8)) == "invalidArgument"  # ... and may not lie in the plaintexts
    assert b"overlaps" in lib.he_last_error_message()


def test_packings_argument_errors(contexts):
    lib = heamd.load_library()
    h = contexts.one.h

    def pack(ctx=h, bits=64, values=slab(0), rows=5, cols=3, out=slab(1), flag=slab(2)):
        return name_of(lib.he_pnns_pack_dense_rows_device(ctx, bits, values, rows, cols, 0, out, flag, None))

    def unpack(ctx=h, bits=64, packing=0, plaintexts=slab(0), rows=10, cols=3, out=slab(1)):
        return name_of(lib.he_pnns_unpack_device(ctx, bits, packing, plaintexts, rows, cols, out, None))

    for call in (pack, unpack):
        assert call() == "deviceError"
        assert call(bits=0) == "invalidArgument"
        assert call(ctx=None) == "invalidArgument"
        assert call(bits=32) == "invalidArgument"
        assert call(rows=0) == "invalidArgument" and call(cols=0) == "invalidArgument"  # invalidMatrixDimensions
        assert call(rows=0, out=None) == "invalidArgument"
        assert call(rows=1 << 30, cols=1 << 11) == "invalidArgument"                     # too large
        assert call(out=None) == "invalidArgument"
        assert call(out=slab(0)) == "invalidArgument"
    assert pack(cols=33) == "invalidArgument"        # above N / 2
    assert pack(cols=32) == "deviceError"
    assert pack(values=None) == "invalidArgument"
    assert pack(flag=None) == "deviceError"
    assert unpack(packing=1, cols=33) == "invalidArgument"
    assert unpack(packing=0, cols=33) == "deviceError"   # dense columns have no such bound
    assert unpack(packing=1) == "deviceError"
    assert unpack(plaintexts=None) == "invalidArgument"
    # the packings left out
    assert unpack(packing=2) == "unsupportedHeOperation"
    assert unpack(packing=2, plaintexts=None) == "unsupportedHeOperation"
    assert unpack(packing=2, ctx=None) == "invalidArgument"  # ... behind the word and the context
    assert unpack(packing=3) == "invalidArgument"
    assert not hasattr(lib, "he_pnns_pack_dense_columns_device")


def array_of(*pnns_contexts):
    return (vp * max(len(pnns_contexts), 1))(*[None if ctx is None else ctx.h for ctx in pnns_contexts])


def test_client_argument_errors(contexts):
    lib = heamd.load_library()
    one, other = contexts.one, contexts.other

    def query(ctxs=(one, other), count=None, bits=64, vectors=slab(0), rows=5, cols=4, key=slab(1), a=slab(2), e=slab(3),
              out=slab(4), flag=slab(5), workspace=None, workspace_bytes=0):
        handles = None if ctxs is None else array_of(*ctxs)
        count = (0 if ctxs is None else len(ctxs)) if count is None else count
        return name_of(lib.he_pnns_generate_query_device(handles, count, bits, vectors, rows, cols, 180.0, key, a, e, out, flag,
                                                         workspace, workspace_bytes, None))

    def answer(ctxs=(one, other), count=None, bits=64, moduli=1, response=slab(0), key=slab(1), rows=10, query_rows=5,
               out=slab(4), workspace=None, workspace_bytes=0):
        handles = None if ctxs is None else array_of(*ctxs)
        count = (0 if ctxs is None else len(ctxs)) if count is None else count
        return name_of(lib.he_pnns_decrypt_response_device(handles, count, bits, moduli, response, key, rows, query_rows, 180.0,
                                                           out, workspace, workspace_bytes, None))

    for call in (query, answer):
        assert call() == "deviceError"                     # valid: only the device is missing
        assert call(ctxs=(one,)) == "deviceError"
        assert call(bits=8) == "invalidArgument"
        assert call(ctxs=None) == "invalidArgument"
        assert call(count=0) == "invalidArgument"
        assert call(ctxs=(one,) * 9) == "invalidArgument"  # above 8, before the contexts are looked at
        assert call(ctxs=(one, None)) == "invalidArgument"
        assert call(bits=32) == "invalidArgument"
        assert call(ctxs=(one, contexts.word32)) == "invalidArgument"        # word size
        assert call(ctxs=(one, contexts.other_degree)) == "invalidArgument"  # degree
        assert call(ctxs=(one, contexts.other_moduli)) == "invalidArgument"  # coefficient moduli
        assert call(ctxs=(one, contexts.same_t)) == "invalidArgument"        # equal plaintext moduli
        assert call(ctxs=(one, one)) == "invalidArgument"
        assert call(ctxs=tuple(contexts.wide)) == "invalidArgument"          # 2 q above UInt64.max
        assert call(ctxs=(contexts.wide[0],)) == "deviceError"               # ... which one context never is
        assert call(ctxs=(contexts.word32,), bits=32) == "deviceError"
        assert call(rows=0) == "invalidArgument"
        assert call(key=None) == "invalidArgument"
        assert call(out=None) == "invalidArgument"
        assert call(workspace=slab(6), workspace_bytes=1 << 20) == "deviceError"  # (its size is checked with the device's checks)
        assert call(workspace=slab(4), workspace_bytes=64) == "invalidArgument"   # the workspace inside `out`
    assert query(cols=33) == "invalidArgument" and query(cols=0) == "invalidArgument"
    assert query(vectors=None) == "invalidArgument" and query(a=None) == "invalidArgument" and query(e=None) == "invalidArgument"
    assert query(flag=None) == "deviceError"
    assert query(e=slab(4)) == "invalidArgument"  # the seeds inside `out`
    assert answer(query_rows=0) == "invalidArgument"
    assert answer(moduli=0) == "invalidArgument" and answer(moduli=3) == "invalidArgument"
    assert answer(moduli=2) == "deviceError"
    assert answer(response=None) == "invalidArgument"
    assert answer(response=slab(4)) == "invalidArgument"
    assert lib.he_last_error_message()


def test_workspace_sizes(contexts):
    one, other = contexts.one, contexts.other
    bfv = one.bfv
    # quantised int64 + one plaintext staging slab + he_bfv_encrypt_device's own, every part a multiple of 16 bytes
    for rows, cols in ((5, 4), (20, 4), (3, 32)):
        count = pnns.plaintext_count(N, rows, cols, "denseRow")
        expected = -(-rows * cols * 8 // 16) * 16 + count * N * 8 + bfv.encrypt_workspace_bytes("encrypt", count)
        assert heamd.pnns_generate_query_workspace_bytes([one], rows, cols) == expected
        assert heamd.pnns_generate_query_workspace_bytes([one, other], rows, cols) == expected  # one context at a time
    for rows, query_rows in ((10, 5), (70, 3)):
        count = pnns.plaintext_count(N, rows, query_rows, "denseColumn")
        for ctxs in ([one], [one, other]):
            expected = len(ctxs) * count * N * 8 + bfv.decrypt_workspace_bytes(count, moduli_count=1)
            assert heamd.pnns_decrypt_response_workspace_bytes(ctxs, rows, query_rows) == expected
    assert heamd.pnns_generate_query_workspace_bytes([one, one], 5, 4) == 0
    assert heamd.pnns_generate_query_workspace_bytes([one], 5, 33) == 0
    assert heamd.pnns_decrypt_response_workspace_bytes([one], 10, 5, moduli_count=9) == 0
