"""The ciphertext-level wire format without a GPU: Bfv.skipLSBsForDecryption against the reference's 17 known
answers, byte counts, every error code the entries name, the kernel-form choice of csrc/ciphertext_wire_form.hpp and of the
4-byte functions of csrc/serialize_form.hpp against their restatement (tests/ciphertext_wire_reference.py) over the device
tests' whole case table (tests/ciphertext_wire_cases.py), and the ABI."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest

import ciphertext_wire_cases as C
import ciphertext_wire_reference as R
import wire_format_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "swift-homomorphic-encryption_amd", "csrc")
ENTRIES = ("he_bfv_skip_lsbs_for_decryption", "he_ciphertexts_serialization_byte_count", "he_ciphertexts_wire_plan",
           "he_ciphertexts_serialize_device", "he_ciphertexts_serialize_device_u32", "he_ciphertexts_deserialize_device",
           "he_ciphertexts_deserialize_device_u32", "he_ciphertexts_deserialize_seeded_device",
           "he_ciphertexts_deserialize_seeded_device_u32", "he_poly_serialize_device_u32", "he_poly_deserialize_device_u32",
           "he_poly_random_from_seeds_device_u32")
NOMINAL = 0x7f12_3456_7000  # a 256-byte aligned address: the device tests assert that their buffers are aligned so


def _context(degree, bits):
    import heamd

    return heamd.PolyContext(degree, C.moduli_of(bits, heamd.generate_primes), host_only=True)


def _status(name):
    import heamd

    return {v: k for k, v in heamd.binding.STATUS_NAMES.items()}[name]


# ---- Bfv.skipLSBsForDecryption -------------------------------------------------------------------------------------------------
def _kats():
    with open(os.path.join(ROOT, "tests", "golden", "skip_lsbs_kats.json")) as f:
        return json.load(f)["rows"]


def test_skip_lsbs_known_answers():
    import heamd

    rows = _kats()
    assert len(rows) == 17
    for row in rows:
        q0, t = row["coefficient_moduli"][0], row["plaintext_modulus"]
        assert heamd.skip_lsbs_for_decryption(row["degree"], q0, t, 1) == row["skip_lsbs"], row["name"]
        assert R.skip_lsbs_for_decryption(row["degree"], q0, t, 1) == row["skip_lsbs"], row["name"]
        for moduli_count in (2, 3):  # only a ciphertext at its last modulus drops bits
            assert heamd.skip_lsbs_for_decryption(row["degree"], q0, t, moduli_count) == [0, 0]
    assert {tuple(row["skip_lsbs"]) for row in rows} >= {(22, 13), (11, 3), (11, 0)}  # what the device tests and the bench use


def test_skip_lsbs_small_ratios_and_arguments():
    import heamd

    lib = heamd.load_library()
    for degree, q0, t in ((8, 17, 16), (8, 31, 16), (8, 32, 16), (4096, 1 << 20, 3), (16, (1 << 62) - 57, 2), (1, 1000, 3)):
        assert heamd.skip_lsbs_for_decryption(degree, q0, t) == R.skip_lsbs_for_decryption(degree, q0, t), (degree, q0, t)
    out = (ctypes.c_int * 2)()
    assert lib.he_bfv_skip_lsbs_for_decryption(8, 17, 3, 1, None) == _status("invalidArgument")
    for args in ((0, 17, 3, 1), (8, 0, 3, 1), (8, 17, 0, 1), (8, 17, 3, 0)):
        assert lib.he_bfv_skip_lsbs_for_decryption(*args, out) == _status("invalidArgument"), args


# ---- byte counts and error codes -------------------------------------------------------------------------------------------------
def test_byte_counts_over_the_case_table():
    seen = set()
    for case in C.ALL:
        key = (case.degree, case.bits, case.poly_count, case.skip_kind)
        if key in seen:
            continue
        seen.add(key)
        ctx = _context(case.degree, case.bits)
        skips = C.skips_of(case)
        expected = R.record_bytes(case.degree, ctx.moduli, skips or [0] * case.poly_count)
        assert ctx.ciphertexts_serialization_byte_count(case.poly_count, skips) == expected, case
        one = [ctx.serialization_byte_count(s) for s in (skips or [0] * case.poly_count)]
        assert expected == 2 + sum(one)


def test_byte_count_is_zero_on_invalid_arguments():
    import heamd

    ctx = _context(64, (55, 40, 62))
    assert heamd.load_library().he_ciphertexts_serialization_byte_count(None, 2, None) == 0
    for poly_count in (0, 4):
        assert ctx.ciphertexts_serialization_byte_count(poly_count, None) == 0
    assert ctx.ciphertexts_serialization_byte_count(2, [0, 40]) == 0  # the 40-bit row would keep no bit
    assert ctx.ciphertexts_serialization_byte_count(2, [-1, 0]) == 0


def _call_all(ctx, word_bits, poly_count, skips, stride, count=1):
    """the status of serialize, deserialize and the plan (both directions) for one set of arguments: device pointers are
    never touched when the arguments are refused"""
    import heamd

    lib = heamd.load_library()
    suffix = "_u32" if word_bits == 32 else ""
    skip_array = None if skips is None else (ctypes.c_int * len(skips))(*skips)
    fake = ctypes.c_void_p(0x1000)
    return [
        getattr(lib, "he_ciphertexts_serialize_device" + suffix)(ctx.h, fake, count, poly_count, skip_array, fake, stride, None),
        getattr(lib, "he_ciphertexts_deserialize_device" + suffix)(ctx.h, fake, stride, count, poly_count, skip_array, fake, None,
                                                                    None),
        lib.he_ciphertexts_wire_plan(0, word_bits, ctx.h, poly_count, skip_array, stride, 0, 0, None, None, None, None),
        lib.he_ciphertexts_wire_plan(1, word_bits, ctx.h, poly_count, skip_array, stride, 0, 0, None, None, None, None),
    ]


@pytest.mark.parametrize("word_bits", [64, 32])
def test_error_codes(word_bits):
    import heamd

    lib = heamd.load_library()
    bits = C.BITS[word_bits][3]
    ctx = _context(64, bits)
    need = ctx.ciphertexts_serialization_byte_count(2, None)
    # no reference ciphertext has more than three polynomials (poly_count 0 is the plan's polynomial-level query)
    assert _call_all(ctx, word_bits, 4, None, 1 << 20)[:] == [_status("unsupportedHeOperation")] * 4
    assert _call_all(ctx, word_bits, 0, None, 1 << 20)[:2] == [_status("unsupportedHeOperation")] * 2
    # CoefficientPacking.validate per polynomial: the second polynomial's skip leaves its narrowest row nothing
    for skips in ([0, min(bits)], [0, -1], [min(bits) + 3, 0]):
        assert _call_all(ctx, word_bits, 2, skips, 1 << 20) == [_status("invalidCoefficientPacking")] * 4, skips
    assert _call_all(ctx, word_bits, 2, [0, min(bits) - 1], 1 << 20) != [_status("invalidCoefficientPacking")] * 4
    # a stride below the byte count
    assert _call_all(ctx, word_bits, 2, None, need - 1) == [_status("serializedBufferSizeMismatch")] * 4
    # ... and nothing else is wrong with those arguments: no ciphertexts, no work, no device
    assert _call_all(ctx, word_bits, 2, None, need, count=0)[:2] == [0, 0]
    suffix = "_u32" if word_bits == 32 else ""
    seeded = getattr(lib, "he_ciphertexts_deserialize_seeded_device" + suffix)
    fake = ctypes.c_void_p(0x1000)
    assert seeded(ctx.h, fake, ctx.serialization_byte_count(0) - 1, fake, 1, 0, fake, None) == _status("serializedBufferSizeMismatch")
    assert seeded(ctx.h, fake, ctx.serialization_byte_count(0), fake, 0, 0, fake, None) == 0
    assert seeded(None, fake, 1 << 20, fake, 1, 0, fake, None) == _status("invalidArgument")
    assert lib.he_ciphertexts_wire_plan(2, word_bits, ctx.h, 2, None, need, 0, 0, None, None, None, None) == _status("invalidArgument")
    assert lib.he_ciphertexts_wire_plan(0, 16, ctx.h, 2, None, need, 0, 0, None, None, None, None) == _status("invalidArgument")


def test_u32_entries_refuse_moduli_that_do_not_fit():
    import heamd

    lib = heamd.load_library()
    ctx = _context(64, (55,))
    fake = ctypes.c_void_p(0x1000)
    refused = _status("invalidModulus")
    assert _call_all(ctx, 32, 2, None, 1 << 20) == [refused] * 4
    assert lib.he_ciphertexts_deserialize_seeded_device_u32(ctx.h, fake, 1 << 20, fake, 1, 0, fake, None) == refused
    assert lib.he_poly_serialize_device_u32(ctx.h, fake, 1, 0, fake, None) == refused
    assert lib.he_poly_deserialize_device_u32(ctx.h, fake, 1 << 20, 1, 0, fake, None) == refused
    assert lib.he_poly_random_from_seeds_device_u32(ctx.h, fake, 1, fake, None) == refused
    narrow = _context(64, (30, 27, 2))
    assert lib.he_poly_deserialize_device_u32(narrow.h, fake, narrow.serialization_byte_count(0) - 1, 1, 0, fake,
                                              None) == _status("serializedBufferSizeMismatch")
    assert lib.he_poly_serialize_device_u32(narrow.h, fake, 1, 2, fake, None) == _status("invalidCoefficientPacking")


def test_seeded_coeff_refuses_what_has_no_transform_before_any_launch():
    """a Coeff seeded call needs the inverse transform of slot 1: a modulus that is no NTT modulus, and (4-byte words) a degree
    the 4-byte transform does not reach, are refused with a message before anything is enqueued -- host-only contexts, whose
    device is never touched, get these codes and not deviceError"""
    import heamd

    lib = heamd.load_library()
    fake = ctypes.c_void_p(0x1000)
    seeds, cts = ctypes.c_void_p(1 << 28), ctypes.c_void_p(2 << 28)  # a range each: the slabs of a call must not overlap
    plain = _context(64, (30, 27, 2))  # 3 is no NTT modulus for degree 64
    for name in ("he_ciphertexts_deserialize_seeded_device", "he_ciphertexts_deserialize_seeded_device_u32"):
        seeded = getattr(lib, name)
        assert seeded(plain.h, fake, 1 << 20, seeds, 1, 1, cts, None) == _status("invalidNttModulus")
        assert b"not an NTT modulus" in lib.he_last_error_message()
        # Eval takes no transform, and neither does a call that skips the seeds: both get as far as the device
        assert seeded(plain.h, fake, 1 << 20, seeds, 1, 0, cts, None) == _status("deviceError")
        assert seeded(plain.h, fake, 1 << 20, None, 1, 1, cts, None) == _status("deviceError")
    degree = 65536
    wide = heamd.PolyContext(degree, heamd.generate_primes([28], False, degree), host_only=True)
    assert lib.he_ciphertexts_deserialize_seeded_device_u32(wide.h, fake, 1 << 20, seeds, 1, 1, cts,
                                                            None) == _status("unsupportedHeOperation")
    assert b"32768" in lib.he_last_error_message()
    assert lib.he_ciphertexts_deserialize_seeded_device_u32(wide.h, fake, 1 << 20, seeds, 1, 0, cts, None) == _status("deviceError")
    assert lib.he_ciphertexts_deserialize_seeded_device(wide.h, fake, 1 << 20, seeds, 1, 1, cts, None) == _status("deviceError")


# ---- the kernel form -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    binary = tmp_path_factory.mktemp("ciphertext_wire_form") / "ciphertext_wire_form_probe"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "c", "ciphertext_wire_form_probe.cpp"), "-o", str(binary)], check=True)

    def ask(args):
        return subprocess.run([str(binary), *map(str, args)], capture_output=True, text=True, check=True).stdout.splitlines()

    return ask


def test_headers_include_nothing_of_hip():
    for name in ("ciphertext_wire_form.hpp", "serialize_form.hpp"):
        includes = re.findall(r'#include\s*[<"]([^>"]+)[>"]', open(os.path.join(CSRC, name)).read())
        assert includes and all(i in ("cstddef", "cstdint") for i in includes), (name, includes)
    text = open(os.path.join(CSRC, "ciphertext_wire_kernels.hip")).read()
    assert "ciphertext_wire_form::for_serialize(" in text and "ciphertext_wire_form::for_deserialize(" in text


def test_case_table_covers_what_it_claims():
    for word_bits in (64, 32):
        table = C.cases(word_bits)
        assert len(table) == 32 and len({(c.degree, len(c.bits), c.poly_count, c.count) for c in table}) == 32
        for degree in C.DEGREES:
            mine = [c for c in table if c.degree == degree]
            assert {c.skip_kind for c in mine} == set(C.SKIP_KINDS)
            assert {c.stride_kind for c in mine} == set(C.STRIDE_KINDS)
            assert {c.record_offset for c in mine} == set(C.RECORD_OFFSETS) and {c.slab_offset for c in mine} == set(C.SLAB_OFFSETS)
        # the one-bit pair really leaves a 1-bit row, the known-answer pair really is unequal
        for c in table:
            skips = C.skips_of(c)
            if c.skip_kind == "one-bit":
                assert min(c.bits) - skips[1] == 1
            if c.skip_kind == "unequal":
                assert skips[0] != skips[1]
    known = {tuple(r["skip_lsbs"]) for r in _kats()}
    assert {tuple(C.UNEQUAL_SKIPS[key]) for key in ((64, 1), (64, 3), (32, 1))} <= known  # (32, 3): see the table's comment
    # every kind of record deserialize is fed meets every degree on both word sizes
    kinds = {(c.word_bits, c.degree, C.RECORD_KINDS[i % 3]) for i, c in enumerate(C.ALL)}
    assert len(kinds) == 2 * len(C.DEGREES) * len(C.RECORD_KINDS)
    assert {b for c in C.cases(32) for b in c.bits} == {30, 27, 2}


def test_form_over_the_device_tests_case_table(probe):
    """the library's plan, the header compiled on its own and the restatement agree on every case of the device tests, and the
    table reaches every form a launcher can return, in both directions and both word sizes"""
    queries, expected, planned = [], [], []
    for case in C.ALL:
        ctx = _context(case.degree, case.bits)
        skips = C.skips_of(case)
        record = ctx.ciphertexts_serialization_byte_count(case.poly_count, skips)
        stride = C.stride_of(case, record)
        assert stride >= record and (case.stride_kind != "mult16" or stride % 16 == 0)
        address = NOMINAL + case.record_offset
        for direction in ("serialize", "deserialize"):
            expected.append(R.ciphertext_form(direction, case.degree, len(case.bits), case.poly_count, record, stride, address))
            planned.append(ctx.ciphertexts_wire_plan(direction, case.poly_count, skips, stride, address, NOMINAL + 0x10000,
                                                     case.word_bits))
            if direction == "serialize":
                queries += ["ct-serialize", record, stride, address]
            else:
                queries += ["ct-deserialize", case.poly_count, len(case.bits), case.degree.bit_length() - 1, stride, address]
    assert planned == expected
    names = {"0": False, "1": True}
    answers = [(form, int(items), names[edge]) for form, items, edge in (line.split() for line in probe(queries))]
    assert answers == [(e["form"], e["items_per_record"], e["edge_free"]) for e in expected]
    # every form the launchers can return, per direction and word size; and both kinds of record placement
    pairs = [(c.word_bits, d) for c in C.ALL for d in ("serialize", "deserialize")]
    for word_bits in (64, 32):
        assert {e["form"] for (w, d), e in zip(pairs, expected) if w == word_bits and d == "serialize"} == {"chunk"}
        assert {e["form"] for (w, d), e in zip(pairs, expected) if w == word_bits and d == "deserialize"} == {"field"}
        assert {e["edge_free"] for (w, _), e in zip(pairs, expected) if w == word_bits} == {True, False}


def test_narrow_form_over_the_device_tests_case_table(probe):
    queries, expected, planned = [], [], []
    for case in C.NARROW:
        ctx = _context(case.degree, case.bits)
        widths = R.widths(ctx.moduli, case.skip)
        offsets = W.row_offsets(case.degree, widths)
        address = NOMINAL + case.bytes_offset
        stride = offsets[-1] + case.extra
        expected += [R.poly_form(4, "serialize", case.degree, widths, address, NOMINAL + 0x10000),
                     R.poly_form(4, "deserialize", case.degree, widths, address, NOMINAL + 0x10000, stride)]
        assert expected[-2:] == [case.serialize_form, case.deserialize_form], case
        planned += [ctx.ciphertexts_wire_plan("serialize", 0, [case.skip], 0, address, NOMINAL + 0x10000, 32)["form"],
                    ctx.ciphertexts_wire_plan("deserialize", 0, [case.skip], stride, address, NOMINAL + 0x10000, 32)["form"]]
        queries += ["narrow-serialize", address, len(widths), *offsets, "narrow-deserialize", address, stride, len(widths), *offsets]
    assert planned == expected and probe(queries) == expected
    assert set(expected[0::2]) == {"byte", "word"} and set(expected[1::2]) == {"byte", "word"}  # 4-byte slabs never take tiles
    # on 8-byte words the plan's polynomial-level answer is serialize_form.hpp's, the tile form included
    ctx = _context(128, (55, 40, 62))
    record = ctx.serialization_byte_count(0)
    for residue, want in ((0, "tile"), (8, "word"), (1, "byte")):
        assert ctx.ciphertexts_wire_plan("serialize", 0, [0], 0, NOMINAL + residue, NOMINAL + 0x10000, 64)["form"] == want
        assert ctx.ciphertexts_wire_plan("deserialize", 0, [0], record, NOMINAL + residue, NOMINAL + 0x10000, 64)["form"] == want


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound():
    import heamd

    lib = heamd.load_library()
    bound = {name for name, _, _ in heamd.binding.SIGNATURES}
    header = open(os.path.join(ROOT, "include", "he_amd.h")).read()
    assert header == open(os.path.join(ROOT, "swift", "Sources", "CHeAmd", "include", "he_amd.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in bound and re.search(r"\b%s\(" % name, header), name
