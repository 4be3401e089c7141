"""tests/keyword_pir_client_reference.py held to what it restates, and csrc/keyword_pir_client_plan.hpp held to it -- all without
a device:

  - the per-query outcome over the hand-built table of tests/keyword_pir_client_cases.py equals what the table states and, where
    every bucket deserializes, what keyword_pir_reference.deserialize_bucket / find give; on buckets serialize_bucket wrote the
    walk finds the slots that were written;
  - the hash and the indices equal the reference's known answers (tests/golden/keyword_pir_kats.json), and the keywords the query
    test relies on do collide;
  - the count scan equals the table's counts;
  - a host program compiled against csrc/keyword_pir_client_plan.hpp agrees with the Python plan."""
import json
import os
import re
import shutil
import subprocess

import pytest

import keyword_pir_client_cases as cases
import keyword_pir_client_reference as client
import keyword_pir_reference as kw
import pir_client_reference as index_client

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "swift-homomorphic-encryption_amd", "csrc")
T17 = 65537


@pytest.mark.parametrize("case", cases.CASES, ids=lambda case: case.name)
def test_case_table_against_the_restatement_and_the_bucket_reference(case):
    assert client.find_in_buckets(case.rows, case.target) == (case.status, case.size, case.value)
    assert len(client.padded_value(case.status, case.value, case.entry_size)) == client.value_capacity(case.entry_size)
    # keyword_pir_reference, bucket by bucket as decrypt(response:at:using:) goes through them
    expected = (client.NIL, None)
    for raw in case.rows:
        try:
            value = kw.find(raw, hash_=case.target)
        except kw.PirError as error:
            assert error.name == "corruptedData"
            expected = (client.CORRUPT, None)
            break
        if value is not None:
            expected = (client.FOUND, value)
            break
    assert expected == (case.status, case.value if case.status == client.FOUND else None)


def test_the_table_holds_what_it_has_to():
    by = {case.name: case for case in cases.CASES}
    assert {case.h for case in cases.CASES} >= {1, 2, 3, 8}
    assert {case.status for case in cases.CASES} == {client.NIL, client.FOUND, client.CORRUPT}
    assert by["empty value found"].status == client.FOUND and by["empty value found"].size == 0
    assert by["empty value, other hash"].status == client.NIL
    assert by["255 slots, the last"].entry_size == 2551 and by["255 slots, the last"].rows[0][0] == 255
    assert by["a value of 65535 bytes"].entry_size == 65546 and by["a value of 65535 bytes"].size == 65535
    sizes = {case.entry_size for case in cases.CASES}
    assert {1, 11, client.STAGED_ROW_LIMIT, client.STAGED_ROW_LIMIT + 1, client.STAGED_SMALL_ROW_LIMIT,
            client.STAGED_SMALL_ROW_LIMIT + 1} <= sizes
    assert any(size % 2 == 1 for size in sizes)
    for entry_size, form in cases.FORMS.items():
        assert client.find_form(entry_size) == form and entry_size in sizes
    # the slots of the near-miss case lie at odd offsets
    walked = client.walk(by["byte 0 and byte 7 differ"].rows[0])
    assert [offset - 10 for _, offset, _ in walked[0]] == [1, 13, 25]
    # the batch has three outcomes
    assert {status for _, _, status, _ in cases.BATCH} == {client.NIL, client.FOUND, client.CORRUPT}
    for rows, target, status, value in cases.BATCH:
        assert client.find_in_buckets(rows, target) == (status, len(value), value)
        assert all(len(raw) == cases.BATCH_E for raw in rows) and len(rows) == cases.BATCH_H


def test_walk_finds_the_slots_serialize_bucket_wrote():
    slots = [(cases.T, b""), (cases.A, b"abc"), (cases.B, cases.pattern(300, 1)), (0, b"\x00")]
    raw = kw.serialize_bucket(slots)
    for padding in (0, 1, 9, 10, 11):
        walked, end = client.walk(raw + bytes(padding))
        assert end == len(raw) and [(h, (raw + bytes(padding))[o:o + s]) for h, o, s in walked] == slots
        assert kw.deserialize_bucket(raw + bytes(padding)) == slots
    for cut in range(1, len(raw)):
        assert client.walk(raw[:cut]) is None
        with pytest.raises(kw.PirError):
            kw.deserialize_bucket(raw[:cut])
    assert client.walk(b"") is None


@pytest.mark.parametrize("name,data,expected", cases.COUNT_CASES, ids=[name for name, _, _ in cases.COUNT_CASES])
def test_count_cases(name, data, expected):
    assert client.count_reply_entries(data) == expected
    # the reference's loop, on keyword_pir_reference: `while let bucket = try? HashBucket(deserialize: bytes[offset...])`
    offset, found = 0, 0
    while True:
        try:
            slots = kw.deserialize_bucket(data[offset:])
        except kw.PirError:
            break
        found += len(slots)
        offset += kw.serialized_size([len(value) for _, value in slots])
    assert found == expected


def test_count_batch():
    for replies, expected in zip(cases.COUNT_BATCH, cases.COUNT_BATCH_EXPECTED):
        assert all(len(data) <= cases.COUNT_BATCH_LENGTH for data in replies)
        assert client.count_entries(replies) == expected
        assert client.count_entries([data + bytes(cases.COUNT_BATCH_LENGTH - len(data)) for data in replies]) == expected


def test_hash_and_indices_against_the_known_answers():
    with open(os.path.join(ROOT, "tests", "golden", "keyword_pir_kats.json")) as f:
        kats = json.load(f)
    for kat in kats["hash_indices"]:
        hash_, indices = client.hash_and_indices(bytes(kat["keyword"]), kat["bucket_count"], kat["hash_function_count"])
        assert indices == kat["expected"] and hash_ == kw.keyword_hash(bytes(kat["keyword"]))
    raw = bytes(kats["raw_bucket"]["bytes"])
    for found in kats["raw_bucket"]["finds"]:
        keyword, value = bytes(found["keyword"]), bytes(found["value"])
        assert client.find_in_buckets([bytes(50), raw], kw.keyword_hash(keyword)) == (client.FOUND, len(value), value)
    assert client.find_in_buckets([raw], kw.keyword_hash(b"not there")) == (client.NIL, 0, b"")


def test_colliding_keywords_collide():
    for bucket_count, (keyword, indices) in cases.COLLIDING.items():
        hash_ = kw.keyword_hash(keyword)
        assert kw.index_from_hash(hash_, bucket_count, 0) == kw.index_from_hash(hash_, bucket_count, 1)  # the second candidate
        assert client.hash_and_indices(keyword, bucket_count, 3)[1] == indices and len(set(indices)) == 3
        assert keyword in cases.KEYWORDS


# ---- the plan --------------------------------------------------------------------------------------------------------------------
def test_plan_is_the_index_plan_without_a_prefix():
    for degree, t, dimensions, entries, entry_size, h in ((64, T17, [4, 3], 70, 20, 2), (64, T17, [5], 5, 332, 3),
                                                          (8192, T17, [40, 30], 1200, 16384, 2)):
        p = client.plan(degree, t, dimensions, entries, entry_size, h)
        index = index_client.plan(degree, t, dimensions, entries, entry_size, False, h)
        assert all(p[key] == value for key, value in index.items())
        assert p["entry_size_encoding_width"] == 0 and p["indices_count"] == h
        assert p["reply_bytes"] == index["reply_ciphertext_count"] * index["bytes_per_plaintext"] >= entry_size


def test_value_capacity_and_form_by_hand():
    assert [client.value_capacity(e) for e in (0, 1, 10, 11, 12, 65546, 65547, 1 << 20)] == [0, 0, 0, 0, 1, 65535, 65535, 65535]
    assert [client.find_form(e) for e in (1, 32768, 32769, 65546)] == ["staged", "staged", "direct", "direct"]
    assert [client.staged_lds_bytes(e) for e in (1, 4096, 4097, 32768, 32769)] == [4112, 4112, 32784, 32784, 0]


def test_header_includes_nothing_of_hip():
    includes = re.findall(r'#include\s*[<"]([^>"]+)[>"]', open(os.path.join(CSRC, "keyword_pir_client_plan.hpp")).read())
    assert includes and all(i in ("cstddef", "cstdint") for i in includes), includes


def test_host_program_agrees_with_the_python_plan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    binary = tmp_path / "keyword_pir_client_plan_probe"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "c", "keyword_pir_client_plan_probe.cpp"), "-o", str(binary)], check=True)
    sizes = [1, 10, 11, 12, 13, 76, 1024, 4095, 4096, 4097, 32767, 32768, 32769, 65545, 65546, 65547, 1 << 20]
    for replies, bpp in ((1, 128), (3, 128), (2, 16384)):
        out = subprocess.run([str(binary), str(replies), str(bpp), *map(str, sizes)], capture_output=True, text=True,
                             check=True).stdout.splitlines()
        assert out[0].split() == [str(v) for v in (client.STAGED_ROW_LIMIT, client.STAGED_SMALL_ROW_LIMIT, client.STAGE_PADDING, 16,
                                                   8)]
        assert len(out) == 1 + len(sizes)
        for entry_size, line in zip(sizes, out[1:]):
            expected = [client.value_capacity(entry_size), 0 if client.find_form(entry_size) == "staged" else 1,
                        client.staged_lds_bytes(entry_size), replies * bpp]
            assert [int(v) for v in line.split()] == expected, entry_size
