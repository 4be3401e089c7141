"""he_simple_pir_shape (host only, no GPU): SimplePirServerProtocol.computingParams, process's padded column size and
SimplePirContext's modulus equal the restatement on a grid of shapes, the reference's test shapes included; every invalid
argument is HE_ERR_INVALID_ARGUMENT."""
import ctypes
import itertools

import pytest

import heamd
import simple_pir_reference as R

BIT_PAIRS = [(7, 28, 32), (14, 42, 64)]
ENTRY_COUNTS = [1, 2, 3, 7, 10, 20, 64, 100, 600, 1000, 4096, 10**4, 65537, 10**5, 10**6]
ENTRY_SIZES = [1, 2, 3, 5, 7, 8, 13, 20, 32, 50, 62, 100, 255, 256, 600, 1000, 1024, 4099, 10**4]


@pytest.mark.parametrize("pbits,cbits,word_bits", BIT_PAIRS)
def test_shape_equals_the_restatement_on_a_grid(oracle, pbits, cbits, word_bits):
    checked = 0
    for entry_count, entry_size in itertools.product(ENTRY_COUNTS, ENTRY_SIZES):
        try:
            expected = R.shape(oracle, pbits, cbits, 1024, entry_count, entry_size, word_bits)
        except R.ShapeError:
            with pytest.raises(heamd.HeError) as err:
                heamd.simple_pir_shape(pbits, cbits, 1024, entry_count, entry_size, word_bits)
            assert err.value.name == "invalidArgument"
            continue
        assert heamd.simple_pir_shape(pbits, cbits, 1024, entry_count, entry_size, word_bits) == expected, (entry_count, entry_size)
        assert expected["entries_per_column"] == 1 or expected["chunks_per_entry"] == 1
        assert expected["column_size"] * expected["database_columns"] >= entry_count * expected["entry_size_in_scalar"]
        checked += 1
    assert checked > 250


@pytest.mark.parametrize("args,columns,rows,chunks", [
    ((7, 28, 1024, 600, 20, 32), 600, 23, 1),
    ((14, 42, 1024, 600, 20, 64), 600, 12, 1),
    ((7, 28, 1024, 20, 600, 32), 100, 138, 5),
    ((14, 42, 1024, 20, 600, 64), 80, 86, 4),
    ((8, 9, 16, 1, 1, 32), 1, 1, 1),
    ((8, 9, 8, 10, 1, 32), 10, 1, 1),
    ((4, 8, 8, 1, 1, 32), 2, 1, 2),     # round(1 / 2) = 1: halves go away from zero
    ((4, 8, 8, 10, 62, 32), 30, 42, 3),
])
def test_reference_test_shapes(oracle, args, columns, rows, chunks):
    plan = heamd.simple_pir_shape(*args[:5], word_bits=args[5])
    assert plan == R.shape(oracle, *args)
    assert (plan["database_columns"], plan["column_size"], plan["chunks_per_entry"]) == (columns, rows, chunks)
    assert plan["modulus"] == oracle.generate_primes([args[1] + 1], True, args[2])[0]
    assert plan["modulus"].bit_length() == args[1] + 1 and plan["modulus"] % (2 * args[2]) == 1


def test_element_bytes():
    for pbits, cbits, expected in [(1, 20, 1), (8, 20, 1), (9, 20, 2), (16, 40, 2), (17, 40, 4), (32, 50, 4), (33, 50, 8)]:
        assert heamd.simple_pir_shape(pbits, cbits, 64, 10, 10)["element_bytes"] == expected


@pytest.mark.parametrize("args", [
    (7, 7, 1024, 10, 10, 64),     # ciphertext_bits <= plaintext_bits
    (8, 7, 1024, 10, 10, 64),
    (0, 7, 1024, 10, 10, 64),
    (7, 28, 1000, 10, 10, 64),    # not a power of two
    (7, 28, 0, 10, 10, 64),
    (7, 30, 1024, 10, 10, 32),    # p would not be a UInt32 PolyRq modulus
    (7, 61, 1024, 10, 10, 64),
    (7, 28, 1024, 10, 10, 16),    # no such word
    (7, 28, 1024, 0, 10, 64),     # empty
    (7, 28, 1024, 10, 0, 64),
])
def test_invalid_arguments(args):
    with pytest.raises(heamd.HeError) as err:
        heamd.simple_pir_shape(*args[:5], word_bits=args[5])
    assert err.value.name == "invalidArgument"
    handle = ctypes.c_void_p()
    status = heamd.load_library().he_simple_pir_context_create(*args[:3], args[5], args[3], args[4], ctypes.byref(handle))
    assert status == 16 and not handle.value


def test_null_outputs_are_accepted():
    null = [None] * 8
    assert heamd.load_library().he_simple_pir_shape(7, 28, 1024, 32, 600, 20, *null) == 0
