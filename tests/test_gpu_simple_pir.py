"""SimplePirServer on the device (he_simple_pir_*), word for word against tests/simple_pir_reference.py -- the numpy
restatement with a materialised A that tests/test_simple_pir_reference.py holds to the reference's own acceptance tests.

Shapes: the reference's four (SimplePirTests.swift:23-46); database_columns below, at and above N (a_poly_count 3, not a
multiple of N); chunks_per_entry > 1 with zero padding; one entry; a plaintext_bits in every element_bytes class the word
allows.  The bench-size test checks every word of the reply for four stacked requests and 64 rows of the hint (the first and
last 16, and the 16 either side of the device's first row-block boundary at row 4096); the host's materialised-A product for
those 64 rows takes well under a minute, so the bound the issue names is not lowered."""
import zlib

import numpy as np
import pytest

import simple_pir_reference as R

pytestmark = pytest.mark.gpu

# (entry_count, entry_size_in_bytes, plaintext_bits, ciphertext_bits, lattice_dimension, word_bits)
SHAPES = {
    "ref-small-u32": (600, 20, 7, 28, 1024, 32),
    "ref-small-u64": (600, 20, 14, 42, 1024, 64),
    "ref-large-u32": (20, 600, 7, 28, 1024, 32),   # chunks_per_entry 5, 686 scalars padded to 690
    "ref-large-u64": (20, 600, 14, 42, 1024, 64),  # chunks_per_entry 4, 343 scalars padded to 344
    "columns-equal-n-u32": (1024, 2, 7, 28, 1024, 32),
    "columns-equal-n-u64": (256, 3, 14, 42, 256, 64),
    "three-polys-u32": (700, 3, 7, 28, 256, 32),
    "three-polys-u64": (700, 3, 14, 42, 256, 64),
    "one-entry-u32": (1, 50, 7, 28, 64, 32),
    "one-entry-u64": (1, 50, 14, 42, 64, 64),
    "bytes2-u32": (90, 9, 14, 28, 64, 32),
    "bytes4-u32": (90, 9, 20, 29, 64, 32),
    "bytes1-u64": (90, 9, 7, 42, 64, 64),
    "bytes4-u64": (90, 9, 20, 42, 64, 64),
    "bytes8-u64": (90, 9, 40, 55, 64, 64),
}


def _server_class(word_bits):
    import heamd

    return heamd.SimplePirServer if word_bits == 64 else heamd.SimplePirServer32


def _words_to_device(values, word_bits):
    import heamd

    return heamd.to_device(values) if word_bits == 64 else heamd.to_device32(values)


def _words_to_host(tensor, word_bits):
    import heamd

    return heamd.to_host(tensor) if word_bits == 64 else heamd.to_host32(tensor)


class Case:
    def __init__(self, name):
        import torch

        import oracle

        entry_count, entry_size, pbits, cbits, n, word_bits = SHAPES[name]
        self.word_bits = word_bits
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        self.rng = rng
        self.entries = rng.integers(0, 256, size=(entry_count, entry_size), dtype=np.uint8)
        self.seed = bytes(rng.integers(0, 256, size=32, dtype=np.uint8))
        self.params = R.shape(oracle, pbits, cbits, n, entry_count, entry_size, word_bits)
        self.database = R.process_database(oracle, self.entries, self.params)
        self.a_matrix = R.materialize_a(self.params, R.a_polynomials(oracle, self.params, self.seed))
        self.hint = R.hint(self.params, self.database, self.a_matrix)
        self.server = _server_class(word_bits).process(torch.from_numpy(self.entries).cuda(), pbits, cbits, n, self.seed)
        torch.cuda.synchronize()

    def respond(self, requests):
        return _words_to_host(self.server.compute_response(_words_to_device(requests, self.word_bits)), self.word_bits)


_cases = {}


@pytest.fixture(params=sorted(SHAPES))
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(request.param)
    return _cases[request.param]


def test_shapes_cover_what_they_claim():
    import oracle

    plan = {name: R.shape(oracle, *s[2:5], s[0], s[1], s[5]) for name, s in SHAPES.items()}
    assert plan["ref-small-u32"]["database_columns"] < 1024
    assert plan["columns-equal-n-u32"]["database_columns"] == 1024 and plan["columns-equal-n-u64"]["database_columns"] == 256
    for name in ("three-polys-u32", "three-polys-u64"):
        assert plan[name]["a_poly_count"] >= 3 and plan[name]["database_columns"] % 256 != 0
    for name in ("ref-large-u32", "ref-large-u64"):
        assert plan[name]["chunks_per_entry"] > 1 and plan[name]["entry_size_in_scalar"] % plan[name]["chunks_per_entry"] != 0
    assert {plan[n]["element_bytes"] for n in plan if n.endswith("u32")} == {1, 2, 4}
    assert {plan[n]["element_bytes"] for n in plan if n.endswith("u64")} == {1, 2, 4, 8}


def test_database_and_hint(case):
    assert case.server.params == case.params
    assert case.server.database.element_size() == case.params["element_bytes"]
    assert np.array_equal(_words_to_host(case.server.wide_database(), case.word_bits), case.database)
    assert np.array_equal(_words_to_host(case.server.hint, case.word_bits), case.hint)


def test_hint_in_row_blocks(case, monkeypatch):
    """Many row blocks give the words of one."""
    import torch

    monkeypatch.setenv("HEAMD_SIMPLE_PIR_ROW_BLOCK", "5")
    p = case.params
    again = _server_class(case.word_bits).process(torch.from_numpy(case.entries).cuda(), p["plaintext_bits"],
                                                  p["ciphertext_bits"], p["lattice_dimension"], case.seed)
    assert np.array_equal(_words_to_host(again.hint, case.word_bits), case.hint)


def test_pack_unpack(case):
    import torch

    wide = case.server.wide_database()
    packed = type(case.server).from_wide(wide, case.server.hint, case.params)
    assert torch.equal(packed.database, case.server.database)
    # pack masks (documented in the header): bits at and above plaintext_bits are dropped
    if case.params["plaintext_bits"] < case.word_bits - 1:
        dirty = _words_to_device(case.database | np.uint64(1 << case.params["plaintext_bits"]), case.word_bits)
        assert torch.equal(type(case.server).from_wide(dirty, case.server.hint, case.params).database, case.server.database)


@pytest.mark.parametrize("query_count", [1, 2, 3, 5, 8, 17])
def test_replies(case, query_count):
    p = case.params
    top = 1 << p["ciphertext_bits"]
    uniform = case.rng.integers(0, top, size=(query_count, p["database_columns"]), dtype=np.uint64)
    ones = np.full((query_count, p["database_columns"]), top - 1, dtype=np.uint64)
    for requests in (uniform, ones):
        expected = R.compute_response(p, case.database, requests, case.word_bits).astype(np.uint64)
        assert np.array_equal(case.respond(requests), expected)


def test_delta_request_returns_the_entries(case):
    """Independent of the restatement's server: Delta in one column returns Delta x that column, whose elements pack back to
    the raw bytes of the entries stored there."""
    import oracle

    p = case.params
    shift = p["ciphertext_bits"] - p["plaintext_bits"]
    size = R.chunk_size(p)
    for entry in sorted({0, p["entry_count"] - 1, p["entry_count"] // 2}):
        coefficients = []
        for q in range(p["chunks_per_entry"]):
            sub = q + entry * p["chunks_per_entry"]
            requests = np.zeros((1, p["database_columns"]), dtype=np.uint64)
            requests[0, sub // p["entries_per_column"]] = 1 << shift
            reply = case.respond(requests)[0]
            assert not np.any(reply & np.uint64((1 << shift) - 1))
            start = (sub % p["entries_per_column"]) * size
            coefficients.extend(int(v) >> shift for v in reply[start:start + size])
        data = oracle.coefficients_to_bytes(coefficients, p["plaintext_bits"])
        assert bytes(data[:p["entry_size_in_bytes"]]) == case.entries[entry].tobytes()


# The reference's two parameter pairs (SimplePirTests.swift:23-46), the only ones it decrypts with: the reply's noise is about
# 2^plaintext_bits x 3.24 x sqrt(database_columns), which Delta / 2 = 2^(ciphertext_bits - plaintext_bits - 1) must exceed;
# the element-size cases (20 / 42 bits: noise near 2^25 against 2^21) are toy widths that no client could decrypt.
END_TO_END = sorted(name for name, s in SHAPES.items() if s[2:4] in ((7, 28), (14, 42)))


@pytest.mark.parametrize("name", END_TO_END)
def test_end_to_end(name):
    """The restated client against the device-built database and hint."""
    import oracle

    if name not in _cases:
        _cases[name] = Case(name)
    case = _cases[name]
    p = case.params
    device_hint = _words_to_host(case.server.hint, case.word_bits)
    client = R.Client(oracle, p, device_hint, case.a_matrix, case.rng)
    for index in sorted({0, p["entry_count"] - 1, int(case.rng.integers(0, p["entry_count"]))}):
        responses = case.respond(client.query(index))
        assert client.decrypt(responses, index) == case.entries[index].tobytes()


def test_stream_ordered(case):
    """Two calls on two streams with an event between them give the words of the serial order.  The server keeps its context,
    so process returns with its work in flight: stream `first` is kept busy for a while ahead of it, the outputs start as
    zeros, and the event is still pending when the reply is enqueued on `second` -- a reply that did not wait for the event, or
    a kernel of either call launched on another stream, would read zeros."""
    import torch

    p = case.params
    requests = case.rng.integers(0, 1 << p["ciphertext_bits"], size=(3, p["database_columns"]), dtype=np.uint64)
    expected = R.compute_response(p, case.database, requests, case.word_bits).astype(np.uint64)
    assert expected.any()
    device_entries = torch.from_numpy(case.entries).cuda()
    device_requests = _words_to_device(requests, case.word_bits)
    seed = torch.from_numpy(np.frombuffer(case.seed, dtype=np.uint8).copy()).cuda()
    other_seed = torch.zeros(32, dtype=torch.uint8, device="cuda")
    server = _server_class(case.word_bits).process(device_entries, p["plaintext_bits"], p["ciphertext_bits"],
                                                   p["lattice_dimension"], other_seed)
    database, hint = torch.zeros_like(server.database), torch.zeros_like(server.hint)
    load = torch.randn(8192, 8192, device="cuda")
    load @ load  # library start-up outside the ordered part
    torch.cuda.synchronize()
    first, second = torch.cuda.Stream(), torch.cuda.Stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(first):
        for _ in range(20):
            load @ load
    server.reprocess(device_entries, seed, stream=first, out=(database, hint))
    done.record(first)
    pending = not done.query()
    second.wait_event(done)
    responses = server.compute_response(device_requests, stream=second)
    second.synchronize()
    assert pending, "process did not return before its stream had drained: not enqueue-only"
    assert np.array_equal(_words_to_host(responses, case.word_bits), expected)
    assert np.array_equal(_words_to_host(server.hint, case.word_bits), case.hint)
    assert np.array_equal(_words_to_host(server.wide_database(), case.word_bits), case.database)


@pytest.mark.parametrize("pbits,cbits,word_bits", [(7, 28, 32), (14, 42, 64)])
def test_bench_size(pbits, cbits, word_bits):
    """About 2^30 elements: 32768 entries of 32768 scalars each, a square database of 32768 columns (32 seeded polynomials)."""
    import torch

    import oracle

    n, count = 1024, 32768
    entry_size = 32768 * pbits // 8
    p = R.shape(oracle, pbits, cbits, n, count, entry_size, word_bits)
    assert p["column_size"] == 32768 and p["database_columns"] == 32768 and p["a_poly_count"] == 32
    rng = np.random.default_rng(pbits)
    entries = rng.integers(0, 256, size=(count, entry_size), dtype=np.uint8)
    seed = bytes(rng.integers(0, 256, size=32, dtype=np.uint8))
    server = _server_class(word_bits).process(torch.from_numpy(entries).cuda(), pbits, cbits, n, seed)
    requests = rng.integers(0, 1 << cbits, size=(4, p["database_columns"]), dtype=np.uint64)
    responses = _words_to_host(server.compute_response(_words_to_device(requests, word_bits)), word_bits)
    # the restated database, kept in the narrow type on the host too (2^30 uint64 would be 8 GiB)
    narrow = np.uint8 if pbits <= 8 else np.uint16
    flat = np.zeros((p["database_columns"], p["column_size"]), dtype=narrow)
    for e in range(count):
        flat[e] = oracle.bytes_to_coefficients(entries[e], pbits, False)
    database = np.ascontiguousarray(flat.T)
    del flat
    assert np.array_equal(server.database.cpu().numpy().view(narrow), database)
    for first in range(0, p["column_size"], 2048):  # every word of the reply
        block = database[first:first + 2048].astype(np.uint64)
        expected = R.compute_response(p, block, requests, word_bits).astype(np.uint64)
        assert np.array_equal(responses[:, first:first + 2048], expected), first
    rows = list(range(16)) + list(range(4096 - 16, 4096 + 16)) + list(range(p["column_size"] - 16, p["column_size"]))
    a_matrix = R.materialize_a(p, R.a_polynomials(oracle, p, seed))
    expected_hint = R.hint(p, database[rows].astype(np.uint64), a_matrix)
    device_hint = _words_to_host(server.hint[torch.tensor(rows, device="cuda")], word_bits)
    assert np.array_equal(device_hint, expected_hint)
