"""Processed-database files without a GPU: the restatement of ProcessedDatabase.serialize() /
init(from:context:) round trips; he_pir_database_file_scan, _byte_count and _header against it over the device tests' whole
case table on host-only contexts; every error the entries name, with its status and string; and the ABI."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import pir_database_file_cases as C
import pir_database_file_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("he_pir_database_file_scan", "he_pir_database_file_byte_count", "he_pir_database_file_header",
           "he_pir_database_load_device", "he_pir_database_load_device_u32", "he_pir_database_save_device",
           "he_pir_database_save_device_u32")


@functools.lru_cache(maxsize=None)
def _context(params):
    """a host-only context of the parameter set (8-byte constants: the file does not depend on the word size)"""
    import heamd

    t, q = C.moduli_of(params, heamd.generate_primes)
    return heamd.BfvContext(params.degree, t, q, host_only=True)


def _moduli(ctx):
    return ctx.coefficient_moduli[:ctx.L]


def _plaintexts(case, moduli, random_fields=False):
    """reduced random rows under the case's mask (random_fields: any value of the field's width, also >= q)"""
    rng = np.random.default_rng(C.seed_of(case))
    out = []
    for here in C.mask_of(case):
        if not here:
            out.append(None)
            continue
        tops = [1 << w for w in R.widths(moduli)] if random_fields else moduli
        out.append([[int(v) for v in rng.integers(0, top, size=case.params.degree, dtype=np.uint64)] for top in tops])
    return out


def _status(name):
    import heamd

    return {v: k for k, v in heamd.binding.STATUS_NAMES.items()}[name]


def _scan(ctx, data, capacity=None, mask=True):
    """the raw entry -> (status, count, present count, consumed, mask bytes)"""
    import heamd

    lib = heamd.load_library()
    image = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(bytes(data).ljust(1, b"\0"))
    capacity = len(data) if capacity is None else capacity
    present = (ctypes.c_uint8 * max(capacity, 1))(*([0xEE] * max(capacity, 1)))
    outs = [ctypes.c_size_t(12345) for _ in range(3)]
    status = lib.he_pir_database_file_scan(ctx.h, image, len(data), present if mask else None, capacity,
                                           *[ctypes.byref(o) for o in outs])
    return status, outs[0].value, outs[1].value, outs[2].value, bytes(present)[:capacity]


# ---- the restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.ALL, ids=C.case_id)
def test_restatement_round_trip(case):
    moduli = _moduli(_context(case.params))
    for random_fields in (False, True):
        plaintexts = _plaintexts(case, moduli, random_fields)
        data = R.serialize(plaintexts, moduli)
        payload = R.payload_bytes(case.params.degree, moduli)
        present = [p is not None for p in plaintexts]
        assert len(data) == R.byte_count(present, payload) == 5 + case.count + payload * sum(present)
        assert data[0] == 1 and int.from_bytes(data[1:5], "little") == case.count
        for index, here in enumerate(present):
            assert data[5 + R.tag_offset(present, index, payload)] == (1 if here else 0)
        assert R.scan(data, payload) == ([int(p) for p in present], len(data))
        assert R.deserialize(data, case.params.degree, moduli) == plaintexts
        assert R.deserialize_body(data[5:], C.mask_of(case), case.params.degree, moduli) == plaintexts


def test_case_table_covers_what_it_claims():
    assert {c.params.degree for c in C.ALL} == {8, 64, 256}
    assert {C.rows_of(p) for p in C.PARAMS} == {1, 2, 3}
    assert {p.word_bits for p in C.PARAMS} == {64, 32}
    assert any(max(p.q_bits[:C.rows_of(p)]) > 56 for p in C.PARAMS if p.word_bits == 64)
    assert all(max(p.q_bits) <= 30 for p in C.PARAMS if p.word_bits == 32)
    for params in C.PARAMS:
        mine = [c for c in C.ALL if c.params == params]
        assert {c.pattern for c in mine} == set(C.PATTERNS) and {c.count for c in mine} >= {0, 1}
    assert {c.count for c in C.ALL} == {0, 1, *C.COUNTS}
    for case in C.ALL:
        mask = C.mask_of(case)
        assert len(mask) == case.count
        if case.pattern == "edges-nil":
            assert mask[0] == 0 and mask[-1] == 0
        if case.pattern == "run-one-nil":
            assert int((mask == 0).sum()) == 1
        if case.pattern == "random" and case.count > 4:
            assert 0 < int((mask != 0).sum()) < case.count and int(mask.max()) > 1


# ---- the host entries against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.ALL, ids=C.case_id)
def test_scan_byte_count_and_header_over_the_case_table(case):
    import heamd

    ctx = _context(case.params)
    moduli = _moduli(ctx)
    payload = R.payload_bytes(case.params.degree, moduli)
    assert ctx.database_file_payload_bytes() == payload
    plaintexts = _plaintexts(case, moduli)
    data = R.serialize(plaintexts, moduli)
    want_present, want_consumed = R.scan(data, payload)
    status, count, present_count, consumed, mask = _scan(ctx, data)
    assert (status, count, present_count, consumed) == (0, case.count, sum(want_present), want_consumed)
    assert list(mask[:count]) == want_present and set(mask[count:]) <= {0xEE}
    assert _scan(ctx, data, mask=False)[:4] == (0, case.count, sum(want_present), want_consumed)  # the mask is optional
    assert _scan(ctx, data, capacity=case.count)[0] == 0
    scanned = ctx.scan_database_file(data)
    assert scanned["count"] == case.count and list(scanned["present"]) == want_present
    assert scanned["present_count"] == sum(want_present) and scanned["bytes_consumed"] == len(data)
    # the size formula takes any byte != 0 as present
    assert ctx.database_file_byte_count(C.mask_of(case)) == len(data) == R.byte_count(want_present, payload)
    header = (ctypes.c_uint8 * 5)()
    assert heamd.load_library().he_pir_database_file_header(case.count, header) == 0
    assert bytes(header) == data[:5] == R.header(case.count)


def test_header_and_byte_count_arguments():
    import heamd

    lib = heamd.load_library()
    ctx = _context(C.PARAMS[0])
    header = (ctypes.c_uint8 * 5)()
    assert lib.he_pir_database_file_header(0xffffffff, header) == 0 and bytes(header) == b"\x01\xff\xff\xff\xff"
    assert lib.he_pir_database_file_header(1 << 32, header) == _status("invalidArgument")
    assert lib.he_pir_database_file_header(3, None) == _status("invalidArgument")
    out = ctypes.c_size_t(77)
    assert lib.he_pir_database_file_byte_count(ctx.h, None, 0, ctypes.byref(out)) == 0 and out.value == 5
    assert lib.he_pir_database_file_byte_count(ctx.h, None, 2, ctypes.byref(out)) == _status("invalidArgument")
    assert lib.he_pir_database_file_byte_count(None, None, 0, ctypes.byref(out)) == _status("invalidArgument")
    mask = (ctypes.c_uint8 * 3)(1, 0, 9)
    assert lib.he_pir_database_file_byte_count(ctx.h, mask, 3, None) == _status("invalidArgument")
    assert lib.he_pir_database_file_byte_count(ctx.h, mask, 3, ctypes.byref(out)) == 0
    assert out.value == 5 + 3 + 2 * ctx.database_file_payload_bytes()


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def _small_file():
    case = C.Case(C.PARAMS[0], "edges-nil", 5)  # nil, three present plaintexts of 80 bytes, nil: 250 bytes
    ctx = _context(case.params)
    return ctx, R.serialize(_plaintexts(case, _moduli(ctx)), _moduli(ctx)), R.payload_bytes(8, _moduli(ctx))


def test_new_statuses_have_their_strings():
    import heamd

    lib = heamd.load_library()
    assert _status("invalidDatabaseSerializationVersion") == 23 and _status("invalidDatabaseSerializationPlaintextTag") == 24
    assert lib.he_status_string(23) == b"invalidDatabaseSerializationVersion"
    assert lib.he_status_string(24) == b"invalidDatabaseSerializationPlaintextTag"
    header = open(os.path.join(ROOT, "include", "he_amd.h")).read()
    assert re.search(r"HE_ERR_INVALID_DATABASE_SERIALIZATION_VERSION = 23\b", header)
    assert re.search(r"HE_ERR_INVALID_DATABASE_SERIALIZATION_PLAINTEXT_TAG = 24\b", header)


def test_wrong_version_and_wrong_tag():
    import heamd

    lib = heamd.load_library()
    ctx, data, payload = _small_file()
    for version in (0, 2, 255):
        bad = bytes([version]) + data[1:]
        assert _scan(ctx, bad)[0] == _status("invalidDatabaseSerializationVersion")
        assert f"version number {version}, expected 1".encode() in lib.he_last_error_message()
        with pytest.raises(R.InvalidVersion):
            R.scan(bad, payload)
        assert _scan(ctx, bad[:1])[0] == _status("invalidDatabaseSerializationVersion")  # read before the count, as the reference
        with pytest.raises(heamd.HeError) as err:
            ctx.scan_database_file(bad)
        assert err.value.code == 23 and err.value.name == "invalidDatabaseSerializationVersion"
    present, _ = R.scan(data, payload)
    for index in range(len(present)):
        for tag in (2, 0x80, 0xff):
            at = 5 + R.tag_offset(present, index, payload)
            bad = data[:at] + bytes([tag]) + data[at + 1:]
            status, count, _, _, mask = _scan(ctx, bad)
            assert status == _status("invalidDatabaseSerializationPlaintextTag") and count == 12345  # outs on success only
            assert f"plaintext tag: {tag}".encode() in lib.he_last_error_message()
            assert list(mask[:index]) == present[:index]
            with pytest.raises(R.InvalidTag):
                R.scan(bad, payload)


def test_every_cut_of_a_small_file_is_refused():
    import heamd

    ctx, data, payload = _small_file()
    assert len(data) == 5 + 5 + 3 * payload
    for cut in range(len(data)):
        status, count, _, _, _ = _scan(ctx, data[:cut])
        assert status == _status("invalidArgument") and count == 12345, cut
        with pytest.raises(R.Truncated):
            R.scan(data[:cut], payload)
    assert _scan(ctx, data)[0] == 0
    # a file whose last plaintext is nil ends with that tag: one byte less is refused, the whole file is not
    status = _scan(ctx, data[:-1])[0]
    assert status == _status("invalidArgument") and b"before its tag" in heamd.load_library().he_last_error_message()
    assert _scan(ctx, data[:-2])[0] == _status("invalidArgument")
    assert b"payload of plaintext 3" in heamd.load_library().he_last_error_message()
    assert _scan(ctx, data[:3])[0] == _status("invalidArgument")
    assert b"header" in heamd.load_library().he_last_error_message()


def test_trailing_bytes_are_accepted_and_reported():
    ctx, data, payload = _small_file()
    for extra in (b"\x07", b"\x01" * 300, bytes(range(256))):
        status, count, present_count, consumed, mask = _scan(ctx, data + extra)
        assert (status, count, present_count, consumed) == (0, 5, 3, len(data))
        assert list(mask[:5]) == [0, 1, 1, 1, 0]
        assert R.scan(data + extra, payload) == ([0, 1, 1, 1, 0], len(data))
        assert ctx.scan_database_file(data + extra)["bytes_consumed"] == len(data)


def test_a_mask_too_small_is_refused_and_untouched():
    import heamd

    lib = heamd.load_library()
    ctx, data, _ = _small_file()
    for capacity in (0, 4):
        status, count, _, _, mask = _scan(ctx, data, capacity=capacity)
        assert status == _status("invalidArgument") and count == 12345 and set(mask) <= {0xEE}
    assert _scan(ctx, data, capacity=0, mask=False)[0] == 0  # no mask: the capacity does not matter
    out = ctypes.c_size_t()
    assert lib.he_pir_database_file_scan(None, data, len(data), None, 0, ctypes.byref(out), None, None) == _status("invalidArgument")
    assert lib.he_pir_database_file_scan(ctx.h, None, len(data), None, 0, ctypes.byref(out), None, None) == _status("invalidArgument")
    assert lib.he_pir_database_file_scan(ctx.h, data, len(data), None, 0, None, None, None) == 0  # every out is optional


@pytest.mark.parametrize("word_bits", [64, 32])
def test_device_entries_check_their_arguments_before_any_device_work(word_bits):
    """on a host-only context: null pointers and overlapping buffers are invalidArgument, everything else gets as far as the
    device check (deviceError); the _u32 forms want a Bfv<UInt32> context; an empty range is no work"""
    import heamd

    lib = heamd.load_library()
    ctx = _context(C.PARAMS[5])  # moduli that fit UInt32, 8-byte constants
    suffix = "_u32" if word_bits == 32 else ""
    load, save = getattr(lib, "he_pir_database_load_device" + suffix), getattr(lib, "he_pir_database_save_device" + suffix)
    vp = ctypes.c_void_p
    records, present, database = vp(0x10000), vp(0x20000), vp(0x30000)
    invalid, device = _status("invalidArgument"), _status("deviceError")
    if word_bits == 32:
        assert load(ctx.h, records, 100, present, 4, database, None, None) == invalid
        assert b"Bfv<UInt32>" in lib.he_last_error_message()
        assert save(ctx.h, database, present, 4, records, 100, None, None) == invalid
        return
    assert load(None, records, 100, present, 4, database, None, None) == invalid
    assert save(None, database, present, 4, records, 100, None, None) == invalid
    for args in ((None, 100, present, 4, database), (records, 100, None, 4, database), (records, 100, present, 4, None)):
        assert load(ctx.h, *args, None, None) == invalid, args
    for args in ((None, present, 4, records, 100), (database, None, 4, records, 100), (database, present, 4, None, 100)):
        assert save(ctx.h, *args, None, None) == invalid, args
    words = 4 * ctx.L * ctx.degree * 8
    for records_at in (0x30000, 0x30000 + words - 1, 0x30000 - 99):  # inside, at the last byte, reaching the first byte
        assert load(ctx.h, vp(records_at), 100, present, 4, database, None, None) == invalid
        assert b"overlaps" in lib.he_last_error_message()
        assert save(ctx.h, database, present, 4, vp(records_at), 100, None, None) == invalid
    for records_at in (0x30000 + words, 0x30000 - 100):  # abutting on either side is no overlap
        assert load(ctx.h, vp(records_at), 100, present, 4, database, None, None) == device
        assert save(ctx.h, database, present, 4, vp(records_at), 100, None, None) == device
    assert load(ctx.h, records, 100, present, 1 << 32, database, None, None) == invalid
    assert load(ctx.h, None, 0, None, 0, None, None, None) == 0 and save(ctx.h, None, None, 0, None, 0, None, None) == 0


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_bound(monkeypatch):
    import heamd
    import torch
    from binding_recorder import Stream, recording

    lib = heamd.load_library()
    bound = {name for name, _, _ in heamd.binding.SIGNATURES}
    header = open(os.path.join(ROOT, "include", "he_amd.h")).read()
    assert header == open(os.path.join(ROOT, "swift", "Sources", "CHeAmd", "include", "he_amd.h")).read()
    exports = open(os.path.join(ROOT, "swift-homomorphic-encryption_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*he_\*;", exports)  # the map exports the he_ prefix
    for name in ENTRIES:
        assert name.startswith("he_") and hasattr(lib, name) and name in bound and re.search(r"\b%s\(" % name, header), name
    for method in ("scan_database_file", "load_database_file", "save_database_file", "load_database_segment",
                   "save_database_segment", "database_file_byte_count"):
        assert hasattr(heamd.BfvContext, method) and hasattr(heamd.BfvContext32, method), method
    for cls, suffix, word in ((heamd.BfvContext, "", torch.int64), (heamd.BfvContext32, "_u32", torch.int32)):
        with recording(monkeypatch) as rec:  # the entries the class resolves, without a device
            ctx = cls(8, 17, [97, 193, 257])
            present = rec.tensor("present", (3,), torch.uint8)
            ctx.load_database_segment(rec.tensor("records", (30,), torch.uint8), present, stream=Stream())
            ctx.save_database_segment(rec.tensor("database", (3, 2, 8), word), present, stream=Stream())
            reached = [name for name, _ in rec.calls if name.startswith("he_pir_database_")]
        assert reached == ["he_pir_database_load_device" + suffix, "he_pir_database_save_device" + suffix]
