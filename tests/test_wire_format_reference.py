"""tests/wire_format_reference.py held to the standards' and the reference's own vectors, and the oracle and
csrc/serialize_form.hpp held to it -- all without a device:

  - AES-128 against FIPS-197 Appendix C.1, the CTR_DRBG against the NIST vectors and state trace of the golden file;
  - the oracle's DRBG against the Python one at every counter carry a seeded polynomial can meet in its first chunk (the NIST
    vectors carry nowhere, so nothing else pins the oracle's 128-bit addition), which is what lets the oracle stay the device
    tests' reference in tests/test_gpu_wire_format_edges.py;
  - pack / unpack against the golden CoefficientPacking vectors, and unpack against the oracle's deserialize on bytes no
    serializer wrote (all-0xFF and random: fields at and above the modulus);
  - the kernel form a host program compiled against csrc/serialize_form.hpp answers against form()."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import wire_format_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "swift-homomorphic-encryption_amd", "csrc")

# The smallest coefficient width a PolyContext admits is 1 bit, from the modulus 2 (ceilLog2(2) = 1); the modulus 1 has
# width 0, which CoefficientPacking.validate refuses.  The widest is 62 bits (moduli stay below 2^62).
SMALLEST_WIDTH, LARGEST_WIDTH = 1, 62


# ---- AES and the DRBG ----------------------------------------------------------------------------------------------------------
def test_aes128_fips197_appendix_c1():
    aes = W.Aes128(bytes(range(16)))
    assert aes.encrypt(bytes.fromhex("00112233445566778899aabbccddeeff")).hex() == "69c4e0d86a7b0430d8cdb78070b4c55a"
    assert aes.encrypt(0x00112233445566778899aabbccddeeff).hex() == "69c4e0d86a7b0430d8cdb78070b4c55a"
    assert W.SBOX[0] == 0x63 and W.SBOX[1] == 0x7c and W.SBOX[0x53] == 0xed and sorted(W.SBOX) == list(range(256))


def test_python_drbg_reproduces_the_nist_vectors(kats):
    block = kats["nist_ctr_drbg"]
    trace = block["state_trace"]
    drbg = W.CtrDrbg(bytes.fromhex(trace["entropy"]))
    assert [x.hex() for x in drbg.state()] == trace["after_init"]
    drbg.generate(64)
    assert [x.hex() for x in drbg.state()] == trace["after_first_generate"]
    drbg.generate(64)
    assert [x.hex() for x in drbg.state()] == trace["after_second_generate"]
    assert len(block["vectors"]) >= 10
    for vector in block["vectors"]:
        drbg = W.CtrDrbg(bytes.fromhex(vector["entropy"]))
        expected = bytes.fromhex(vector["returned_bits"])
        drbg.generate(len(expected))
        assert drbg.generate(len(expected)) == expected


def test_nist_vectors_carry_nowhere(kats):
    """why the carry table below is needed: in the golden vectors no counter addition leaves the low 32 bits"""
    for vector in kats["nist_ctr_drbg"]["vectors"]:
        drbg = W.CtrDrbg(bytes.fromhex(vector["entropy"]))
        for _ in range(2):
            blocks = len(vector["returned_bits"]) // 2 // 16
            assert not W.carries(drbg.v, blocks + 2, 32)
            drbg.generate(16 * blocks)


def test_carry_table_is_what_it_claims():
    cases = W.carry_cases()
    assert len(cases) == 4 * len(W.CARRY_OFFSETS) and len({seed for *_, seed in cases}) == len(cases)
    assert set(W.CARRY_OFFSETS) >= {1, 2, 4, 5, 129, 253, 254, 255, 256, 257, 258, 259}
    assert sorted(W.CARRY_UPPER) == [32, 64, 96, 128]
    for bits, k, v0, seed in cases:
        assert len(seed) == 32 and 0 <= v0 < 1 << 128
        assert (v0 + k) % (1 << bits) == 0 and (v0 % (1 << bits)) == (1 << bits) - k
        upper = v0 >> bits
        if bits < 128:
            assert upper != (1 << (128 - bits)) - 1 and upper & 0xffffffff != 0xffffffff  # the carry stops in the next word
        # adding k carries out of exactly the words below the boundary
        assert W.carries(v0, k, bits) and not W.carries(v0, k - 1, bits)
        assert ((v0 + k) & W.MASK128) >> bits == (upper + 1) % (1 << (128 - bits)) if bits < 128 else (v0 + k) & W.MASK128 == 0


@pytest.mark.parametrize("bits", sorted(W.CARRY_UPPER))
def test_oracle_drbg_matches_python_at_every_carry(oracle, bits):
    """V_0 = B - k: chunk 0's stream blocks V + 1 .. V + 256, the counter's move to V + 256 and the re-key's V + 257 and V + 258
    each cross B for some k; the second chunk shows the re-key (its key and counter are the blocks at V + 257, V + 258)."""
    restated = 0
    for level, k, v0, seed in W.carry_cases():
        if level != bits:
            continue
        ours, theirs = W.CtrDrbg(seed), oracle.CtrDrbg(seed)
        assert ours.v == v0
        assert theirs.state() == ours.state() and theirs.state()[1] == v0.to_bytes(16, "big"), (bits, k)
        for chunk in range(2):
            assert theirs.generate(4096) == ours.generate(4096), (bits, k, chunk)
            assert theirs.state() == ours.state(), (bits, k, chunk)
        restated += ours.blocks
    assert 0 < restated <= 15000


def test_seed_for_counter_leaves_the_key_part_free(oracle):
    for key_part in (bytes(16), bytes(range(16)), b"\xff" * 16):
        seed = W.seed_for_counter(W.MASK128, key_part)
        key, counter = oracle.CtrDrbg(seed).state()
        assert counter == b"\xff" * 16
        assert key == bytes(a ^ b for a, b in zip(W.Aes128(bytes(16)).encrypt(1), key_part))


# ---- packing -------------------------------------------------------------------------------------------------------------------
def test_pack_and_unpack_against_the_golden_vectors(kats):
    block = kats["coefficient_packing"]
    assert len(block["coeffs_to_bytes"]) >= 3 and len(block["bytes_to_coeffs"]) >= 3
    for case in block["coeffs_to_bytes"]:
        assert list(W.pack(case["coeffs"], case["bits"] - case["skip"], case["skip"])) == case["expected"], case
    for case in block["bytes_to_coeffs"]:
        width = case["bits"] - case["skip"]
        count = 8 * len(case["bytes"]) // width if case["decode"] else -(-8 * len(case["bytes"]) // width)
        assert W.unpack(bytes(case["bytes"]), count, width, case["skip"]) == case["expected"], case


def test_pack_unpack_roundtrip_and_padding():
    rng = np.random.default_rng(11)
    for width in range(SMALLEST_WIDTH, LARGEST_WIDTH + 1):
        for n in (1, 3, 8, 13):
            values = [int(v) & ((1 << width) - 1) for v in rng.integers(0, 1 << 62, size=n, dtype=np.uint64)]
            row = W.pack(values, width)
            assert len(row) == W.row_byte_count(n, width) and W.unpack(row, n, width) == values
            pad = 8 * len(row) - n * width
            assert 0 <= pad < 8 and row[-1] & ((1 << pad) - 1) == 0
            dirty = row[:-1] + bytes([row[-1] | ((1 << pad) - 1)])
            assert W.unpack(dirty, n, width) == values  # pad bits are not read
            assert W.unpack(row, n, width, 3) == [v << 3 for v in values]
            assert W.pack([v << 3 | 5 for v in values], width, 3) == row


def _context_moduli(oracle, width):
    """one modulus whose ceilLog2 is `width`: 2^width, and for 62 bits (2^62 is no valid modulus) the largest 62-bit prime"""
    return [1 << width] if width < LARGEST_WIDTH else oracle.generate_primes([width], False, 1)


def test_unpack_matches_oracle_deserialize_on_arbitrary_bytes(oracle):
    rng = np.random.default_rng(12)
    cases = 0
    with pytest.raises(oracle.OracleError):
        oracle.PolyContext(8, [1 << LARGEST_WIDTH])
    assert oracle.PolyContext(8, [2]).serialization_byte_count() == 1  # SMALLEST_WIDTH
    assert oracle.PolyContext(8, [1]).serialization_byte_count() == 0
    for degree in (8, 16, 64, 128):
        for bits in range(SMALLEST_WIDTH, LARGEST_WIDTH + 1):
            ctx = oracle.PolyContext(degree, _context_moduli(oracle, bits))
            for skip in sorted({0, 1, bits - 1}):
                if not 0 <= skip < bits:
                    continue  # CoefficientPacking.validate
                width = bits - skip
                count = ctx.serialization_byte_count(skip)
                assert count == W.row_byte_count(degree, width)
                for record in (b"\xff" * count, bytes(rng.integers(0, 256, size=count, dtype=np.uint8))):
                    got = ctx.deserialize(np.frombuffer(record, dtype=np.uint8)[None], skip)
                    assert got.ravel().tolist() == W.unpack(record, degree, width, skip), (degree, bits, skip)
                    cases += 1
    assert cases == 4 * 2 * (1 + 2 + 3 * (LARGEST_WIDTH - 2)) == 1464


def test_product_context_admits_the_same_widths():
    import heamd

    assert heamd.PolyContext(8, [2], host_only=True).serialization_byte_count() == 1  # SMALLEST_WIDTH
    assert heamd.PolyContext(8, [1], host_only=True).serialization_byte_count() == 0
    with pytest.raises(heamd.HeError):
        heamd.PolyContext(8, [1 << LARGEST_WIDTH], host_only=True)
    assert heamd.PolyContext(8, [(1 << 62) - 57], host_only=True).serialization_byte_count() == LARGEST_WIDTH


# ---- the kernel form -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    binary = tmp_path_factory.mktemp("serialize_form") / "serialize_form_probe"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "c", "serialize_form_probe.cpp"), "-o", str(binary)], check=True)

    def ask(queries):
        """queries: (direction, degree, widths, bytes_address, slab_address, bytes_per_poly or None)"""
        args = []
        for direction, degree, widths, bytes_address, slab_address, stride in queries:
            args += [direction, degree.bit_length() - 1, bytes_address, slab_address]
            if direction == "deserialize":
                args.append(stride)
            args += [len(widths), *widths, *W.row_offsets(degree, widths)]
        result = subprocess.run([str(binary), *map(str, args)], capture_output=True, text=True, check=True)
        answers = result.stdout.split()
        assert len(answers) == len(queries)
        return answers

    return ask


def test_header_includes_nothing_of_hip():
    text = open(os.path.join(CSRC, "serialize_form.hpp")).read()
    includes = re.findall(r'#include\s*[<"]([^>"]+)[>"]', text)
    assert includes and all(name in ("cstddef", "cstdint") for name in includes), includes


def test_launchers_choose_through_the_header():
    text = open(os.path.join(CSRC, "galois_kernels.hip")).read()
    assert '#include "serialize_form.hpp"' in text
    assert "serialize_form::for_serialize(" in text and "serialize_form::for_deserialize(" in text
    assert not re.search(r"\bbool\s+(word_aligned|tile_aligned)\b", text)  # no second copy of the predicates
    assert not re.search(r"bytes_per_poly\s*&\s*(7|15)\b", text)


FORM_WIDTHS = ([1], [8], [16], [62], [64], [65], [0, 16], [2, 16], [9, 17, 40, 62], [62, 33, 8], [33, 8], [16, 48],
               list(range(1, 63)))
BASE_ADDRESS = 0x7f12_3456_7000


def test_probe_matches_form(probe):
    queries = []
    for degree in (8, 16, 32, 64, 128, 256, 512, 1024):
        for widths in FORM_WIDTHS:
            record = W.row_offsets(degree, widths)[-1]
            for bytes_residue in (0, 1, 8, 16):
                for slab_residue in (0, 1, 8, 16):
                    addresses = (BASE_ADDRESS + bytes_residue, BASE_ADDRESS + 0x10000 + slab_residue)
                    queries.append(("serialize", degree, widths, *addresses, None))
                    for extra in (0, 1, 8, 16, 24):
                        queries.append(("deserialize", degree, widths, *addresses, record + extra))
    answers = []
    for start in range(0, len(queries), 512):
        answers += probe(queries[start:start + 512])
    expected = [W.form(*query) for query in queries]
    assert answers == expected
    # the grid reaches every form in both directions, and the stride alone moves a call from each form to the next
    for direction in ("serialize", "deserialize"):
        assert {a for q, a in zip(queries, answers) if q[0] == direction} == {"tile", "word", "byte"}
    by_query = dict(zip([(q[0], q[1], tuple(q[2]), q[3], q[4], q[5]) for q in queries], answers))
    record = W.row_offsets(128, [16, 48])[-1]
    at = ("deserialize", 128, (16, 48), BASE_ADDRESS, BASE_ADDRESS + 0x10000)
    assert [by_query[(*at, record + extra)] for extra in (0, 1, 8, 16, 24)] == ["tile", "byte", "word", "tile", "word"]
    # a tile-aligned call is word-aligned: what the launchers rely on when a tile grid does not fit a launch
    for (direction, degree, widths, bytes_address, _, stride), answer in zip(queries, answers):
        if answer == "tile":
            assert bytes_address % 8 == 0 and all(o % 8 == 0 for o in W.row_offsets(degree, widths))
            assert direction == "serialize" or stride % 8 == 0


def test_form_on_the_shapes_the_device_tests_name():
    aligned = (BASE_ADDRESS, BASE_ADDRESS + 0x10000)
    assert W.form("deserialize", 8, [9, 17, 40, 62], *aligned) == "byte"
    assert W.form("deserialize", 64, [9, 17, 40, 62], *aligned) == "word"
    for degree in (128, 512, 1024):
        assert W.form("deserialize", degree, [9, 17, 40, 62], *aligned) == "tile"
        assert W.form("serialize", degree, [9, 17, 40, 62], *aligned) == "tile"
    assert W.form("deserialize", 128, [9], aligned[0] + 8, aligned[1]) == "word"
    assert W.form("deserialize", 128, [9], aligned[0], aligned[1] + 8) == "word"
    assert W.form("deserialize", 128, [9], aligned[0] + 1, aligned[1]) == "byte"
