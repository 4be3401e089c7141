"""SimplePirServer.compute_response_batch (he_simple_pir_compute_response_batch_device: the int8 matrix kernel of
csrc/simple_pir_matrix_kernels.hip) word for word against tests/simple_pir_reference.py::compute_response, which is numpy
and wraps in the word.  Every case asserts through the plan which path it takes.  Databases are built directly as narrow
arrays and uploaded, so a case is milliseconds of GPU time.

Shapes sit on the kernel's edges: its 16-row and 16-request MFMA tiles, the workgroup's 128 rows, the 64-column K step, the
column tile staged in LDS (256 / 128 / 64 columns by word and limbs), requests_per_pass (32 or 16), rows that are no multiple
of 16 bytes and a database pointer that is only element-aligned (the element-wise loads)."""
import zlib

import numpy as np
import pytest

import simple_pir_batch_plan as P
import simple_pir_reference as R

pytestmark = pytest.mark.gpu

NARROW = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def _element_bytes(pbits):
    return 1 if pbits <= 8 else 2 if pbits <= 16 else 4 if pbits <= 32 else 8


def _server(pbits, cbits, word_bits, database, offset=0):
    """A server over `database` (numpy, [rows][columns] in the narrow type); offset > 0 puts its first element that many
    elements past an allocation's start, so that the pointer is only element-aligned."""
    import torch

    import heamd

    rows, columns = database.shape
    narrow = NARROW[_element_bytes(pbits)]
    flat = np.zeros(offset + rows * columns, dtype=narrow)
    flat[offset:] = database.astype(narrow).reshape(-1)
    signed = {np.uint8: np.uint8, np.uint16: np.int16, np.uint32: np.int32, np.uint64: np.int64}[narrow]
    tensor = torch.from_numpy(flat.view(signed)).cuda()[offset:].view(rows, columns)
    assert tensor.data_ptr() % 16 == (offset * flat.itemsize) % 16
    params = dict(plaintext_bits=pbits, ciphertext_bits=cbits, column_size=rows, database_columns=columns,
                  element_bytes=flat.itemsize)
    cls = heamd.SimplePirServer if word_bits == 64 else heamd.SimplePirServer32
    return cls(tensor, None, params)


def _to_device(requests, word_bits):
    import heamd

    return heamd.to_device(requests) if word_bits == 64 else heamd.to_device32(requests)


def _to_host(tensor, word_bits):
    import heamd

    return heamd.to_host(tensor) if word_bits == 64 else heamd.to_host32(tensor)


def _check(pbits, cbits, word_bits, database, requests, matrix_path=1, offset=0):
    """The batch entry's words for `requests` (uint64 values, reduced to the word on upload) equal the reference's."""
    import heamd

    plan = heamd.simple_pir_batch_plan(pbits, cbits, database.shape[1], len(requests), word_bits)
    assert plan == P.plan(pbits, cbits, word_bits) and plan["matrix_path"] == matrix_path, plan
    server = _server(pbits, cbits, word_bits, database, offset)
    words = requests & np.uint64(2**word_bits - 1)
    got = _to_host(server.compute_response_batch(_to_device(words, word_bits)), word_bits)
    expected = R.compute_response(server.params, database, words, word_bits).astype(np.uint64)
    assert got.shape == expected.shape == (len(requests), database.shape[0])
    assert np.array_equal(got, expected), np.argwhere(got != expected)[:8]
    return server, words, got


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _random_case(pbits, cbits, word_bits, rows, columns, queries, offset=0, matrix_path=1):
    rng = _rng(pbits, cbits, word_bits, rows, columns, queries, offset)
    database = rng.integers(0, 1 << pbits, size=(rows, columns), dtype=np.uint64)
    requests = rng.integers(0, 2**word_bits - 1, size=(queries, columns), dtype=np.uint64, endpoint=True)
    return _check(pbits, cbits, word_bits, database, requests, matrix_path, offset)


# (plaintext_bits, ciphertext_bits, word_bits, rows, columns, query_count, element offset of the database pointer)
# (7, 28, 32): one limb, column tile 256, 32 requests per pass; (14, 42, 64): two limbs, column tile 64, 32 per pass;
# (5, 32, 32) and (14, 60, 64): 16 per pass; (14, 28, 32): two limbs at column tile 128; (7, 42, 64): one limb at tile 128
TILE_EDGES = [
    (7, 28, 32, 1, 1, 1, 0), (7, 28, 32, 15, 63, 15, 0), (7, 28, 32, 16, 64, 16, 0), (7, 28, 32, 17, 65, 17, 0),
    (7, 28, 32, 127, 255, 31, 0), (7, 28, 32, 128, 256, 32, 0), (7, 28, 32, 129, 257, 33, 0), (7, 28, 32, 17, 690, 1, 0),
    (7, 28, 32, 1, 256, 33, 0), (7, 28, 32, 129, 1, 16, 0), (7, 28, 32, 16, 690, 32, 0), (7, 28, 32, 15, 512, 17, 0),
    (7, 28, 32, 17, 64, 15, 1), (7, 28, 32, 128, 257, 17, 1), (7, 28, 32, 300, 272, 65, 0),
    (14, 42, 64, 1, 1, 1, 0), (14, 42, 64, 15, 63, 15, 0), (14, 42, 64, 16, 64, 16, 0), (14, 42, 64, 17, 65, 17, 0),
    (14, 42, 64, 127, 127, 31, 0), (14, 42, 64, 128, 128, 32, 0), (14, 42, 64, 129, 129, 33, 0), (14, 42, 64, 17, 690, 16, 0),
    (14, 42, 64, 16, 64, 17, 1), (14, 42, 64, 129, 690, 33, 1), (14, 42, 64, 260, 200, 1, 0),
    (5, 32, 32, 17, 255, 15, 0), (5, 32, 32, 128, 256, 16, 0), (5, 32, 32, 129, 257, 17, 0), (5, 32, 32, 16, 65, 33, 1),
    (14, 60, 64, 15, 63, 15, 0), (14, 60, 64, 128, 64, 16, 0), (14, 60, 64, 129, 65, 17, 0), (14, 60, 64, 17, 690, 33, 1),
    (14, 28, 32, 17, 127, 31, 0), (14, 28, 32, 128, 128, 32, 0), (14, 28, 32, 129, 129, 33, 0), (14, 28, 32, 16, 690, 17, 1),
    (7, 42, 64, 127, 127, 32, 0), (7, 42, 64, 128, 128, 31, 0), (7, 42, 64, 129, 129, 33, 0), (7, 42, 64, 16, 690, 17, 1),
    (7, 64, 64, 17, 65, 17, 0),
]


def test_tile_edge_list_covers_what_it_claims():
    import heamd

    for word_bits, pairs in ((32, [(7, 28), (5, 32), (14, 28)]), (64, [(14, 42), (14, 60), (7, 42)])):
        for pbits, cbits in pairs:
            mine = [c for c in TILE_EDGES if c[:3] == (pbits, cbits, word_bits)]
            per_pass = heamd.simple_pir_batch_plan(pbits, cbits, 1, 1, word_bits)["requests_per_pass"]
            tile = P.tile_columns(word_bits, P.database_limbs(pbits))
            assert {per_pass - 1, per_pass, per_pass + 1} <= {c[5] for c in mine}, (pbits, cbits)
            assert {tile - 1, tile, tile + 1} <= {c[4] for c in mine}, (pbits, cbits)
            assert {P.BLOCK_ROWS, P.BLOCK_ROWS + 1} <= {c[3] for c in mine}, (pbits, cbits)
            assert any(c[6] for c in mine)
    for pbits, cbits, word_bits in ((7, 28, 32), (14, 42, 64)):
        mine = [c for c in TILE_EDGES if c[:3] == (pbits, cbits, word_bits)]
        assert {1, 15, 16, 17, 127, 128, 129} <= {c[3] for c in mine}
        assert {1, 63, 64, 65, 690} <= {c[4] for c in mine}
        assert {1, 15, 16, 17, 31, 32, 33} <= {c[5] for c in mine}
    assert 690 * 2 % 16 != 0  # unaligned rows at 2 bytes


@pytest.mark.parametrize("pbits,cbits,word_bits,rows,columns,queries,offset", TILE_EDGES)
def test_tile_edges(pbits, cbits, word_bits, rows, columns, queries, offset):
    _random_case(pbits, cbits, word_bits, rows, columns, queries, offset)


WIDTHS = [(7, 28, 32), (7, 29, 32), (5, 32, 32), (14, 28, 32), (9, 32, 32),
          (7, 42, 64), (14, 42, 64), (14, 60, 64), (7, 64, 64), (14, 64, 64), (9, 57, 64)]


@pytest.mark.parametrize("pbits,cbits,word_bits", WIDTHS)
def test_widths(pbits, cbits, word_bits):
    """Uniform requests over the whole word, all-ones words and 2^cb - 1, over more than one pass and more than one tile."""
    import heamd

    rows, columns = 37, 200
    queries = heamd.simple_pir_batch_plan(pbits, cbits, columns, 1, word_bits)["requests_per_pass"] + 3
    rng = _rng("widths", pbits, cbits, word_bits)
    database = rng.integers(0, 1 << pbits, size=(rows, columns), dtype=np.uint64)
    database[0, :] = (1 << pbits) - 1
    uniform = rng.integers(0, 2**word_bits - 1, size=(queries, columns), dtype=np.uint64, endpoint=True)
    for requests in (uniform, np.full_like(uniform, 2**word_bits - 1), np.full_like(uniform, 2**cbits - 1)):
        _check(pbits, cbits, word_bits, database, requests)


@pytest.mark.parametrize("pbits,cbits,word_bits", [(8, 28, 32), (16, 42, 64), (20, 42, 64), (40, 55, 64)])
def test_fallback(pbits, cbits, word_bits):
    """Off the matrix path the plan says 0 and the words are those of the existing entry."""
    server, words, got = _random_case(pbits, cbits, word_bits, 70, 130, 19, matrix_path=0)
    existing = _to_host(server.compute_response(_to_device(words, word_bits)), word_bits)
    assert np.array_equal(got, existing)


@pytest.mark.parametrize("pbits,cbits,word_bits", [(7, 28, 32), (14, 28, 32), (7, 42, 64), (14, 42, 64), (14, 64, 64)])
def test_orientation_and_recombination(pbits, cbits, word_bits):
    """Asymmetric data: a transposed write, a swapped limb order or a wrong request-to-lane assignment fails one of these."""
    rows, columns, queries = 40, 100, 20
    r0, c0 = 21, 70
    top = (1 << pbits) - 1
    # a single non-zero element against requests that differ in every (q, c): response[q][r0] = element * requests[q][c0]
    database = np.zeros((rows, columns), dtype=np.uint64)
    database[r0, c0] = top - 2
    q_index, c_index = np.meshgrid(np.arange(queries, dtype=np.uint64), np.arange(columns, dtype=np.uint64), indexing="ij")
    requests = ((q_index * np.uint64(columns) + c_index + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)) & np.uint64(2**word_bits - 1)
    assert len(np.unique(requests)) == requests.size
    _, words, got = _check(pbits, cbits, word_bits, database, requests)
    mask = (1 << cbits) - 1
    assert [int(v) for v in got[:, r0]] == [(top - 2) * int(w) & mask for w in words[:, c0]]
    assert not got[:, np.arange(rows) != r0].any()
    # a delta request in one column (another column per request) against a database whose elements differ
    r_index, c_index = np.meshgrid(np.arange(rows, dtype=np.uint64), np.arange(columns, dtype=np.uint64), indexing="ij")
    database = r_index * np.uint64(columns) + c_index + np.uint64(1)
    if pbits >= 12:
        assert database.max() <= top and len(np.unique(database)) == database.size
    else:
        database = (r_index * np.uint64(31) + c_index * np.uint64(7) + np.uint64(1)) % np.uint64(top + 1)
    requests = np.zeros((queries, columns), dtype=np.uint64)
    delta = 1 << (cbits - pbits)
    picked = [(3 + 5 * q) % columns for q in range(queries)]
    requests[np.arange(queries), picked] = delta
    _, _, got = _check(pbits, cbits, word_bits, database, requests)
    assert np.array_equal(got, (database[:, picked].T * np.uint64(delta)) & np.uint64(mask))


def _worst_case(pbits, cbits, word_bits, rows, columns, queries):
    """Elements all 2^p - 1 against all-ones words: every limb product is the largest there is.  The words also have a closed
    form, -(columns (2^p - 1)) mod 2^word under the mask."""
    database = np.full((rows, columns), (1 << pbits) - 1, dtype=np.uint64)
    requests = np.full((queries, columns), 2**word_bits - 1, dtype=np.uint64)
    _, _, got = _check(pbits, cbits, word_bits, database, requests)
    closed = (-(columns * ((1 << pbits) - 1))) % 2**word_bits & ((1 << cbits) - 1)
    assert np.all(got == np.uint64(closed)), (int(got[0, 0]), closed)


@pytest.mark.parametrize("pbits,cbits,word_bits", [(7, 28, 32), (14, 28, 32), (7, 42, 64), (14, 42, 64)])
def test_fold_at_a_forced_cadence(monkeypatch, pbits, cbits, word_bits):
    import heamd

    monkeypatch.setenv("HEAMD_SIMPLE_PIR_FOLD_COLUMNS", "128")
    assert heamd.simple_pir_batch_plan(pbits, cbits, 300, 3, word_bits)["fold_columns"] == 128
    for columns in (127, 128, 129, 256, 300):
        _worst_case(pbits, cbits, word_bits, 19, columns, 3)
    _random_case(pbits, cbits, word_bits, 19, 300, 3)


@pytest.mark.parametrize("pbits,cbits,word_bits", [(7, 28, 32), (14, 42, 64)])
def test_fold_at_the_natural_cadence(monkeypatch, pbits, cbits, word_bits):
    import heamd

    monkeypatch.delenv("HEAMD_SIMPLE_PIR_FOLD_COLUMNS", raising=False)
    fold = heamd.simple_pir_batch_plan(pbits, cbits, 1, 1, word_bits)["fold_columns"]
    assert fold == P.natural_fold_columns(P.database_limbs(pbits))
    for columns in (fold, fold + 1, 2 * fold + 64):
        _worst_case(pbits, cbits, word_bits, 16, columns, 2)


@pytest.mark.parametrize("name", ["ref-small-u32", "ref-small-u64"])
def test_against_the_existing_entry(name):
    """A database built through process: compute_response_batch equals compute_response word for word."""
    import torch

    import test_gpu_simple_pir as G

    if name not in G._cases:
        G._cases[name] = G.Case(name)
    case = G._cases[name]
    p = case.params
    assert case.server.batch_plan(17)["matrix_path"] == 1
    requests = _rng(name).integers(0, 1 << p["ciphertext_bits"], size=(17, p["database_columns"]), dtype=np.uint64)
    device_requests = _to_device(requests, case.word_bits)
    batch = case.server.compute_response_batch(device_requests)
    assert torch.equal(batch, case.server.compute_response(device_requests))
    expected = R.compute_response(p, case.database, requests, case.word_bits).astype(np.uint64)
    assert np.array_equal(_to_host(batch, case.word_bits), expected)


def test_stream_ordered():
    """The reply enqueued on a second stream behind an event gives the words of the serial order: the database is written on
    stream `first` behind work that keeps it busy, and the event is still pending when the reply is enqueued on `second` --
    a reply that did not wait for the event, or a kernel launched on another stream, would read the zeros it started from."""
    import torch

    pbits, cbits, word_bits, rows, columns, queries = 7, 28, 32, 200, 600, 35
    rng = _rng("stream")
    database = rng.integers(0, 1 << pbits, size=(rows, columns), dtype=np.uint64)
    requests = rng.integers(0, 1 << cbits, size=(queries, columns), dtype=np.uint64)
    real = _server(pbits, cbits, word_bits, database)
    server = _server(pbits, cbits, word_bits, np.zeros_like(database))
    expected = R.compute_response(server.params, database, requests, word_bits).astype(np.uint64)
    assert expected.any()
    device_requests = _to_device(requests, word_bits)
    load = torch.randn(8192, 8192, device="cuda")
    load @ load  # library start-up outside the ordered part
    torch.cuda.synchronize()
    first, second = torch.cuda.Stream(), torch.cuda.Stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(first):
        for _ in range(20):
            load @ load
        server.database.copy_(real.database, non_blocking=True)
    done.record(first)
    pending = not done.query()
    second.wait_event(done)
    responses = server.compute_response_batch(device_requests, stream=second)
    second.synchronize()
    assert pending, "the database's stream had drained before the reply was enqueued: nothing was ordered"
    assert np.array_equal(_to_host(responses, word_bits), expected)
