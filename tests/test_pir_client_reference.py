"""tests/pir_client_reference.py held to what it restates, and csrc/pir_client_plan.hpp held to it -- all without a device:

  - the coordinates invert pir_database_reference.slot_of: the selection they make picks the slot the server put the plaintext in;
  - the closed form of a reply's byte string (what the device kernel computes) equals oracle.coefficients_to_bytes, the loop of
    CoefficientPacking.swift:186-205 as written, coefficients at and above 2^bits included;
  - the evaluation-key elements equal values worked by hand from MulPir.swift:86-109;
  - a host program compiled against csrc/pir_client_plan.hpp agrees with the Python plan over a sweep of parameters."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pir_client_reference as client
import pir_database_reference as refdb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "swift-homomorphic-encryption_amd", "csrc")
T17 = 65537


def selected_slot(coordinates, dimensions):
    """The database slot a query with these coordinates reads: the dim-0 selection walks the d0 plaintexts of a column, the
    remaining dimensions pick the column, the first of them slowest (PirUtil.swift:448-485)"""
    column = 0
    for coordinate, size in zip(coordinates[1:], dimensions[1:]):
        column = column * size + coordinate
    return column * dimensions[0] + coordinates[0]


@pytest.mark.parametrize("dimensions", [[4, 3], [5], [2, 2, 2], [5, 1], [3, 4, 2], [40, 30]])
def test_coordinates_invert_slot_of(dimensions):
    total = int(np.prod(dimensions))
    for per, encoding in ((6, True), (1, False)):
        entry_size = 20 if per > 1 else 300
        p = client.plan(64, T17, dimensions, total * per, entry_size, encoding)
        assert p["entries_per_plaintext"] == per
        for entry in range(total * per):
            coordinates = client.coordinates(p, entry)
            assert all(0 <= c < d for c, d in zip(coordinates, dimensions))
            assert selected_slot(coordinates, dimensions) == refdb.slot_of(entry // per, dimensions), (entry, coordinates)


def test_nonzero_positions_and_selection_values():
    p = client.plan(64, T17, [40, 30], 1200 * 6, 20, True, indices_count=2)
    assert (p["expanded_query_count"], p["query_ciphertext_count"]) == (140, 3)
    ones = client.nonzero_positions(p, [0, 7199])
    assert ones == [0, 40, 70 + 39, 70 + 40 + 29]
    plaintexts = client.query_plaintexts(p, T17, [0, 7199])
    first, last = pow(64, -1, T17), pow(16, -1, T17)  # 64 inputs, and the last ciphertext's 12: ceilLog2 = 4
    assert first != last
    expected = np.zeros((3, 64), dtype=np.uint64)
    expected[0, 0], expected[0, 40], expected[1, 109 - 64], expected[2, 139 - 128] = first, first, first, last
    assert np.array_equal(plaintexts, expected)
    # an index outside the database selects nothing and leaves the others alone
    outside = client.query_plaintexts(p, T17, [7200, 7199])
    expected[0, 0] = expected[0, 40] = 0
    assert np.array_equal(outside, expected)


# ---- the byte string ---------------------------------------------------------------------------------------------------------------
def check_bytes(oracle, coefficients, bits):
    expected = bytes(oracle.coefficients_to_bytes(np.ascontiguousarray(coefficients, dtype=np.uint64), bits))
    assert client.reply_bytes_closed_form(coefficients, bits) == expected, (bits, list(coefficients[:8]))
    return expected


@pytest.mark.parametrize("bits", range(1, 21))
def test_closed_form_bytes_equal_the_oracle(oracle, bits):
    rng = np.random.default_rng(bits)
    n = 64
    for _ in range(4):
        check_bytes(oracle, rng.integers(0, 1 << (bits + 1), size=n, dtype=np.uint64), bits)
    check_bytes(oracle, rng.integers(0, 1 << bits, size=n, dtype=np.uint64), bits)
    check_bytes(oracle, np.full(n, (1 << (bits + 1)) - 1, dtype=np.uint64), bits)  # all ones, the excess bit too
    check_bytes(oracle, np.full(n, (1 << bits) - 1, dtype=np.uint64), bits)
    masked = None
    for k in range(n):  # one excess coefficient, at every field: byte-aligned ones and the others
        coefficients = np.zeros(n, dtype=np.uint64)
        coefficients[k] = 1 << bits
        got = check_bytes(oracle, coefficients, bits)
        if k * bits % 8 == 0:
            assert not any(got), (bits, k)  # dropped
        else:
            stream = np.unpackbits(np.frombuffer(got, dtype=np.uint8))
            assert stream.sum() == 1 and stream[k * bits - 1] == 1, (bits, k)  # the last bit of the field before
            masked = k
    assert masked is not None or bits % 8 == 0


def test_excess_bit_at_an_aligned_and_an_unaligned_field(oracle):
    """t = 641 (9 bits at N = 64): coefficient 8 begins byte 9, coefficient 1 begins inside byte 1"""
    coefficients = np.zeros(64, dtype=np.uint64)
    coefficients[8] = 640
    aligned = check_bytes(oracle, coefficients, 9)
    assert aligned[9] == 0b01000000 and aligned[8] == 0 and aligned[10] == 0  # 640 - 512 = 128: bit 7 of the field, nothing else
    coefficients = np.zeros(64, dtype=np.uint64)
    coefficients[1] = 640
    unaligned = check_bytes(oracle, coefficients, 9)
    assert unaligned[1] == 0b10100000 and unaligned[0] == 0  # bit 9 lands on the last bit of coefficient 0's field


# ---- the evaluation key -------------------------------------------------------------------------------------------------------------
POWERS = {level: (1 << level) + 1 for level in range(1, 14)}
BY_HAND = {  # N = 4096: degree.log2 = 12, (12 + 1).dividingCeil(2) = 7
    # one input: depth 0, smallestPower 13 -- above degree.log2, so the uncompressed range is empty
    (1, "none"): [], (1, "hybrid"): [POWERS[13]], (1, "max"): [POWERS[13]],
    # two inputs: depth 1, smallestPower 12 = largestPower under every strategy; hybrid's extra power max(12, 25 / 2) = 12 is there
    (2, "none"): [POWERS[12]], (2, "hybrid"): [POWERS[12]], (2, "max"): [POWERS[12]],
    # 100 inputs: depth 7, smallestPower 6; compressed largestPower max(6, 7) = 7; hybrid's extra power max(7, 20 / 2) = 10
    (100, "none"): [POWERS[k] for k in range(6, 13)], (100, "hybrid"): [POWERS[6], POWERS[7], POWERS[10]],
    (100, "max"): [POWERS[6], POWERS[7]],
    # 5000 inputs: min(5000, N) = N, depth 12, smallestPower 1
    (5000, "none"): [POWERS[k] for k in range(1, 13)], (5000, "hybrid"): [POWERS[k] for k in range(1, 8)] + [POWERS[10]],
    (5000, "max"): [POWERS[k] for k in range(1, 8)],
}


@pytest.mark.parametrize("count,strategy", sorted(BY_HAND))
def test_evaluation_key_elements_worked_by_hand(count, strategy):
    assert client.evaluation_key_elements(count, 4096, strategy) == BY_HAND[(count, strategy)]


def test_library_gives_the_same_elements():
    import heamd

    ctx = heamd.BfvContext(4096, T17, heamd.generate_primes([40, 40, 41], False, 4096), host_only=True)
    for (count, strategy), expected in BY_HAND.items():
        assert ctx.pir_evaluation_key_elements(count, strategy) == expected, (count, strategy)
    small = heamd.BfvContext(64, T17, heamd.generate_primes([40, 40, 41], False, 64), host_only=True)
    for count in (1, 2, 7, 8, 64, 140):
        for strategy in ("none", "hybrid", "max"):
            assert small.pir_evaluation_key_elements(count, strategy) == client.evaluation_key_elements(count, 64, strategy)


# ---- the plan header ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    binary = tmp_path_factory.mktemp("pir_client_plan") / "pir_client_plan_probe"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "c", "pir_client_plan_probe.cpp"), "-o", str(binary)], check=True)

    def ask(degree, t, encoding, entry_size, entry_count, indices_count, dimensions, indices):
        args = [degree, t, int(encoding), entry_size, entry_count, indices_count, len(dimensions), *dimensions, *indices]
        out = subprocess.run([str(binary), *map(str, args)], capture_output=True, text=True, check=True).stdout.splitlines()
        return out[0].split(), [[int(v) for v in line.split()] for line in out[1:]]

    return ask


def test_header_includes_nothing_of_hip():
    for name in ("pir_client_plan.hpp", "host_math.hpp"):
        includes = re.findall(r'#include\s*[<"]([^>"]+)[>"]', open(os.path.join(CSRC, name)).read())
        assert includes and all(i in ("cstddef", "cstdint", "vector", "host_math.hpp") for i in includes), (name, includes)


def test_host_program_agrees_with_the_python_plan(probe):
    cases = 0
    for degree, t in ((64, T17), (64, 641), (4096, T17), (8192, (1 << 20) + 8192 * 2 * 3 + 1)):
        bpp = degree * (t.bit_length() - 1) // 8
        for dimensions in ([4, 3], [5], [2, 2, 2], [40, 30], [3] * 16):
            total = int(np.prod(dimensions, dtype=object))
            for entry_size, encoding in ((20, True), (20, False), (bpp - 1, True), (bpp, False), (bpp, True), (2 * bpp + 100, True),
                                         (300, False)):
                for indices_count in (1, 3, 60):
                    p = client.plan(degree, t, dimensions, 0, entry_size, encoding, indices_count)
                    entry_count = min(total * p["entries_per_plaintext"], 1 << 40)
                    p["entry_count"] = entry_count
                    indices = sorted({0, 1 % entry_count, entry_count // 2, entry_count - 1,
                                      (p["entries_per_plaintext"] + 1) % entry_count})
                    head, rows = probe(degree, t, encoding, entry_size, entry_count, indices_count, dimensions, indices)
                    counts = [min(degree, p["expanded_query_count"] - c * degree) for c in (0, p["query_ciphertext_count"] - 1)]
                    expected = [p["expanded_query_count"], p["query_ciphertext_count"], p["reply_ciphertext_count"],
                                p["entries_per_plaintext"], p["bytes_per_plaintext"], p["entry_size_encoding_width"],
                                *[client.selection_value(count, t) for count in counts]]
                    assert head == [str(v) for v in expected], (degree, t, dimensions, entry_size, encoding, indices_count)
                    for index, row in zip(indices, rows):
                        assert row == client.coordinates(p, index) + [index % p["entries_per_plaintext"]], (dimensions, index)
                    cases += 1
    assert cases == 4 * 5 * 7 * 3
    # an even modulus has no inverse of a power of two (but of 2^0: one input)
    head, _ = probe(64, 1 << 16, 0, 20, 12, 1, [4, 3], [0])
    assert head[-2:] == ["-", "-"]
    head, _ = probe(64, 1 << 16, 0, 20, 1, 1, [1], [0])
    assert head[-2:] == ["1", "1"]
