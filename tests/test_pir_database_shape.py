"""MulPirServer.process's plan (he_pir_database_shape) and its argument checks on host-only contexts, the compute entry
points' answer there (no device: HE_ERR_DEVICE), and the test restatement (pir_database_reference) against the oracle's
CoefficientPacking.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import heamd
import pir_database_reference as refdb

INVALID, DEVICE = 16, 17


@pytest.fixture(scope="module")
def contexts(oracle):
    out = {}
    for degree, t_bits in ((64, 17), (8192, 17), (4096, 20)):
        t = oracle.generate_primes([t_bits], True, degree)[0]
        q = oracle.generate_primes([40, 40, 41], False, degree)
        out[degree, t_bits] = heamd.BfvContext(degree, t, q, host_only=True)
    return out


def _dims(dimensions):
    return (ctypes.c_uint32 * max(len(dimensions), 1))(*dimensions)


def _cases():
    bpp_64 = 64 * 16 // 8  # N = 64, 17-bit t: 128 bytes per plaintext
    cases = []
    for encoding in (False, True):
        width = 1 if encoding else 0
        # pack mode, split mode
        cases += [((64, 17), [4, 3], 20, 7, encoding), ((64, 17), [4, 3], 12, 300, encoding)]
        # E just below, at and above bpp
        for size in (bpp_64 - width - 1, bpp_64 - width, bpp_64 - width + 1):
            cases.append(((64, 17), [5, 1], 5, size, encoding))
    # the width boundaries of the size prefix (split mode with few rows)
    for size in (255, 256, 65535, 65536, 2**32 - 1, 2**32):
        cases.append(((8192, 17), [2, 2], 3, size, True))
        cases.append(((8192, 17), [2, 2], 3, size, False))
    cases += [((4096, 20), [16, 8], 1000, 9, True), ((4096, 20), [2, 2, 2], 8, 20000, False),
              ((8192, 17), [128, 128], 16384 * 13, 1200, True), ((64, 17), [4], 0, 10, True)]
    return cases


@pytest.mark.parametrize("case", _cases())
def test_shape_agrees_with_the_restatement(contexts, case):
    key, dimensions, entry_count, entry_size, encoding = case
    ctx = contexts[key]
    want = refdb.shape(ctx.degree, ctx.t, dimensions, entry_count, entry_size, encoding)
    assert ctx.pir_database_shape(dimensions, entry_count, entry_size, encoding) == want


@pytest.mark.parametrize("size,width", [(1, 1), (255, 1), (256, 2), (65535, 2), (65536, 4), (2**32 - 1, 4), (2**32, 8)])
def test_encoding_width_boundaries(contexts, size, width):
    ctx = contexts[8192, 17]
    assert ctx.pir_database_shape([4], 1, size, True)["entry_size_encoding_width"] == width
    assert ctx.pir_database_shape([4], 1, size, False)["entry_size_encoding_width"] == 0


@pytest.mark.parametrize("dimensions,entry_count,entry_size,encoding,what", [
    ([], 4, 10, False, "empty dimensions"),
    ([4, 0], 4, 10, False, "zero dimension"),
    ([2, 2], 5, 300, False, "split mode"),       # 5 entries, 4 rows
    ([2, 2], 5 * 6 * 4 + 1, 20, True, "pack mode"),  # 6 entries of 21 bytes per 128-byte plaintext
    ([4], 3, 0, False, "zero bytes"),
])
def test_shape_errors(contexts, dimensions, entry_count, entry_size, encoding, what):
    ctx = contexts[64, 17]
    with pytest.raises(heamd.HeError) as err:
        ctx.pir_database_shape(dimensions, entry_count, entry_size, encoding)
    assert err.value.code == INVALID
    assert what in str(err.value)
    with pytest.raises(refdb.ProcessError):
        refdb.shape(ctx.degree, ctx.t, dimensions, entry_count, entry_size, encoding)


def _process(ctx, dimensions, entry_count, entry_size, encoding, sizes=None, word32=False):
    lib = heamd.load_library()
    entries = np.zeros(max(entry_count * entry_size, 1), dtype=np.uint8)
    database = np.zeros(16, dtype=np.uint64)
    present = np.zeros(16, dtype=np.uint8)
    size_array = None if sizes is None else np.ascontiguousarray(sizes, dtype=np.uint64)
    fn = lib.he_pir_process_database_device_u32 if word32 else lib.he_pir_process_database_device
    status = fn(ctx.h, _dims(dimensions), len(dimensions), entries.ctypes.data_as(ctypes.c_void_p),
                None if size_array is None else size_array.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), entry_count,
                entry_size, int(encoding), database.ctypes.data_as(ctypes.c_void_p), present.ctypes.data_as(ctypes.c_void_p),
                None)
    message = lib.he_last_error_message().decode()
    assert not database.any() and not present.any()  # nothing written on any path here
    return status, message


def test_process_errors_in_the_reference_order(contexts):
    """invalidDatabaseEntrySize comes before the shape checks (MulPir.swift:438-444), with the reference's wording."""
    ctx = contexts[64, 17]
    status, message = _process(ctx, [], 3, 10, False, sizes=[10, 11, 2])
    assert status == INVALID
    assert "Database has entry with size 11 plaintexts, expected all entry sizes to be <= 10" in message
    for dimensions, count, size in (([], 3, 10), ([3, 0], 3, 10), ([2, 2], 5, 300), ([1], 7, 20), ([2], 3, 0)):
        status, message = _process(ctx, dimensions, count, size, False, sizes=[0] * count)
        assert status == INVALID and message.startswith("invalid argument"), (dimensions, message)


def test_compute_entry_points_need_a_device(contexts):
    ctx = contexts[64, 17]
    for sizes in (None, [20] * 12):  # enqueue-only and with sizes to upload
        status, message = _process(ctx, [4, 3], 12, 20, True, sizes=sizes)
        assert status == DEVICE and "host-only" in message


def test_four_byte_database_needs_a_uint32_context(contexts):
    status, message = _process(contexts[64, 17], [4, 3], 12, 20, True, word32=True)
    assert status == INVALID and "UInt32" in message


def test_entry_count_is_checked_by_the_binding(contexts):
    ctx = contexts[64, 17]
    with pytest.raises(heamd.HeError) as err:
        ctx.pir_process_database([b"ab", b"c"], [4], 10, entry_count=3)
    assert err.value.code == INVALID
    assert "Database has 2 entries, expected 3" in str(err.value)


@pytest.mark.parametrize("bits", [1, 3, 7, 8, 13, 17, 20, 31, 33, 59, 63])
def test_unpacking_a_slice_equals_unpacking_it_zero_extended(oracle, bits):
    """CoefficientPacking.bytesToCoefficients reads MSB first with a short last buffer left-aligned: the coefficients of a
    slice are those of the slice followed by zero bytes (the restatement pads with zero coefficients)."""
    rng = np.random.default_rng(bits)
    for length in (1, 3, 7, 9, 13, 17, 23, 40):
        data = rng.integers(1, 256, size=length, dtype=np.uint8)
        coefficients = oracle.bytes_to_coefficients(data, bits, False)
        assert len(coefficients) == -(-length * 8 // bits)
        for extra in (1, 5, 8, 11):
            longer = oracle.bytes_to_coefficients(np.concatenate([data, np.zeros(extra, dtype=np.uint8)]), bits, False)
            assert np.array_equal(longer[:len(coefficients)], coefficients), (length, extra)
            assert not longer[len(coefficients):].any()
        degree = 64
        if len(coefficients) <= degree:
            padded = refdb.unpack(oracle, data.tobytes(), bits, degree)
            assert np.array_equal(padded[:len(coefficients)], coefficients) and not padded[len(coefficients):].any()
        # MSB first: the first coefficient is the top `bits` bits of the stream
        stream = int.from_bytes(data.tobytes(), "big") << (len(coefficients) * bits - length * 8)
        assert int(coefficients[0]) == stream >> ((len(coefficients) - 1) * bits)


def test_restatement_places_pack_and_split_plaintexts():
    """Where bytes go in the restatement itself: the reorder and the slices of both modes."""
    degree, t = 64, (1 << 16) + 1  # 128 bytes per plaintext
    entries = [bytes([e + 1]) * 5 for e in range(13)]
    slices = refdb.plaintext_bytes(entries, [4, 3], degree, t, 20, True)  # E = 21, 6 per plaintext, 3 plaintexts
    assert len(slices) == 1
    assert [refdb.slot_of(j, [4, 3]) for j in range(12)] == [0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11]
    first = slices[0][0]
    assert len(first) == 126 and first[:6] == bytes([5, 1, 1, 1, 1, 1]) and first[21] == 5
    assert len(slices[0][refdb.slot_of(2, [4, 3])]) == 21  # the last plaintext holds one entry
    assert slices[0][refdb.slot_of(3, [4, 3])] == b""
    big = [bytes(range(200)), b""]
    split = refdb.plaintext_bytes(big, [2], degree, t, 300, True)  # prefix width 2, E = 302: 3 chunks
    assert len(split) == 3
    assert split[0][0][:2] == (200).to_bytes(2, "little") and split[1][0] == bytes(range(126, 200)) and split[2][0] == b""
    assert split[0][1] == b"\x00\x00" and split[1][1] == b""
