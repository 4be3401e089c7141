"""he_pir_database_load_device(_u32) / he_pir_database_save_device(_u32): the body of a processed-database
file into the device database and back, bit for bit against the restatement (tests/pir_database_file_reference.py) over the
case table of tests/pir_database_file_cases.py -- at every address residue, with guards around every buffer -- against one
he_poly_deserialize_device per present plaintext, on segments, on buffers that are too short, and end to end: a database built
by he_pir_process_database_device is saved, loaded and answers a query with the same words."""
import functools

import numpy as np
import pytest

import heamd
import pir_database_file_cases as C
import pir_database_file_reference as R
import pir_database_reference as refdb

pytestmark = pytest.mark.gpu

GUARD_BYTES = 64   # poisoned bytes on either side of a records buffer
GUARD_WORDS = 24   # poisoned words on either side of a database slab
POISON_BYTE = 0xA5
POISON_WORD = 0x5A5A5A5A  # fits both word sizes (as a slab value it is above every 30-bit field)


@functools.lru_cache(maxsize=None)
def _context(params):
    t, q = C.moduli_of(params, heamd.generate_primes)
    return heamd.BfvContext32(params.degree, t, q) if params.word_bits == 32 else heamd.BfvContext(params.degree, t, q)


def _moduli(ctx):
    return ctx.coefficient_moduli[:ctx.L]


@functools.lru_cache(maxsize=None)
def _reference(case):
    """computed once per case and shared, never modified: (reduced plaintexts, their body, a body of random payload bytes,
    the plaintexts those bytes deserialize to)"""
    ctx = _context(case.params)
    moduli, degree = _moduli(ctx), case.params.degree
    rng = np.random.default_rng(C.seed_of(case))
    mask = C.mask_of(case)
    plaintexts = [None if not here else [[int(v) for v in rng.integers(0, q, size=degree, dtype=np.uint64)] for q in moduli]
                  for here in mask]
    body = R.serialize_body(plaintexts, moduli)
    payload = R.payload_bytes(degree, moduli)
    noise = bytearray()
    for here in mask:  # arbitrary payload bytes: fields at or above the modulus included (N >= 8: a row has no pad bit)
        noise += bytes([1]) + rng.integers(0, 256, size=payload, dtype=np.uint8).tobytes() if here else bytes([0])
    noise = bytes(noise)
    return plaintexts, body, noise, R.deserialize_body(noise, mask, degree, moduli)


def _words(plaintexts, ctx):
    """the database of these plaintexts as a flat uint64 array"""
    return np.array(R.slab(plaintexts, ctx.L, ctx.degree), dtype=np.uint64).reshape(-1)


def _byte_buffer(content, residue, capacity=None):
    """a poisoned device buffer with `content` (capacity bytes of room, the rest poison) at an address of this residue mod 8
    -> (whole buffer, the view that starts at the content)"""
    import torch

    capacity = len(content) if capacity is None else capacity
    whole = torch.full((GUARD_BYTES + 8 + capacity + GUARD_BYTES,), POISON_BYTE, dtype=torch.uint8, device="cuda")
    start = GUARD_BYTES + (residue - (whole.data_ptr() + GUARD_BYTES)) % 8
    assert (whole.data_ptr() + start) % 8 == residue
    if len(content):
        whole[start:start + len(content)] = torch.from_numpy(np.frombuffer(content, dtype=np.uint8).copy()).cuda()
    return whole, whole[start:start + capacity], start


def _slab(ctx, words, values=None):
    """a poisoned slab of `words` words between poisoned guards -> (whole, the view); values: what the view holds"""
    import torch

    dtype = torch.int32 if ctx.word_bits == 32 else torch.int64
    whole = torch.full((GUARD_WORDS + words + GUARD_WORDS,), POISON_WORD, dtype=dtype, device="cuda")
    view = whole[GUARD_WORDS:GUARD_WORDS + words]
    if values is not None and words:
        view.copy_((heamd.to_device32 if ctx.word_bits == 32 else heamd.to_device)(values))
    return whole, view


def _host(ctx, tensor):
    return (heamd.to_host32 if ctx.word_bits == 32 else heamd.to_host)(tensor)


def _mask_tensor(mask):
    import torch

    return torch.from_numpy(np.ascontiguousarray(mask)).cuda()


def _flag():
    import torch

    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _load_and_check(ctx, body, mask, want_words, residue, records_bytes=None, want_flag=0):
    whole_bytes, records, _ = _byte_buffer(body, residue)
    before = whole_bytes.clone()
    whole, view = _slab(ctx, len(want_words))
    flag = _flag()
    ctx.load_database_segment(records, _mask_tensor(mask), records_bytes=records_bytes, out=view, mismatch=flag)
    got = _host(ctx, whole)
    assert np.array_equal(got[GUARD_WORDS:GUARD_WORDS + len(want_words)], want_words), residue
    assert (got[:GUARD_WORDS] == POISON_WORD).all() and (got[GUARD_WORDS + len(want_words):] == POISON_WORD).all()
    assert int(flag.item()) == want_flag
    assert bool((whole_bytes == before).all())  # a load writes nothing into the records


# ---- load ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.ALL, ids=C.case_id)
def test_load_matches_the_restatement_at_every_residue(case):
    """reduced plaintexts and payloads of arbitrary bytes; nil plaintexts become zeros over a poisoned slab; the guard words
    around the slab stay"""
    ctx = _context(case.params)
    plaintexts, body, noise, noise_plaintexts = _reference(case)
    mask = C.mask_of(case)
    assert R.deserialize_body(body, mask, ctx.degree, _moduli(ctx)) == plaintexts
    for residue in range(8):
        _load_and_check(ctx, body, mask, _words(plaintexts, ctx), residue)
        _load_and_check(ctx, noise, mask, _words(noise_plaintexts, ctx), residue)


@pytest.mark.parametrize("case", [c for c in C.ALL if c.count >= 5], ids=C.case_id)
def test_load_equals_one_polynomial_call_per_present_plaintext(case):
    """the composition the entry replaces: he_poly_deserialize_device(_u32) of each present payload, arbitrary bytes included"""
    import torch

    ctx = _context(case.params)
    _, _, noise, _ = _reference(case)
    mask = C.mask_of(case)
    poly = ctx.ciphertext_context()
    payload = ctx.database_file_payload_bytes()
    whole = torch.from_numpy(np.frombuffer(noise, dtype=np.uint8).copy()).cuda()
    got = ctx.load_database_segment(whole, _mask_tensor(mask))
    for index, here in enumerate(mask):
        if not here:
            assert not bool(got[index].any()), index
            continue
        at = R.tag_offset(list(mask), index, payload) + 1
        record = whole[at:at + payload].clone().reshape(1, payload)
        one = poly.deserialize_u32(record) if case.params.word_bits == 32 else poly.deserialize(record)
        assert bool((got[index] == one[0]).all()), index


@pytest.mark.parametrize("case", [c for c in C.ALL if c.count >= 5], ids=C.case_id)
def test_load_and_save_of_segments(case):
    """every split of the range into two segments at a plaintext boundary: the second starts mid-file (first > 0), at the
    byte the size formula gives, and its buffer starts at that tag"""
    ctx = _context(case.params)
    plaintexts, body, _, _ = _reference(case)
    mask = C.mask_of(case)
    payload = ctx.database_file_payload_bytes()
    per = ctx.L * ctx.degree
    words = _words(plaintexts, ctx)
    for first in sorted({1, case.count // 2, case.count - 1}):
        cut = R.tag_offset(list(mask), first, payload)
        assert cut == ctx.database_file_byte_count(mask[:first]) - 5
        for piece, piece_mask, piece_words in ((body[:cut], mask[:first], words[:first * per]),
                                               (body[cut:], mask[first:], words[first * per:])):
            residue = (first + len(piece)) % 8
            _load_and_check(ctx, piece, piece_mask, piece_words, residue)
            _save_and_check(ctx, piece_words, piece_mask, piece, residue)


# ---- save ------------------------------------------------------------------------------------------------------------------------
def _save_and_check(ctx, words, mask, want_body, residue, records_bytes=None, want_flag=0, poison_nil=True):
    import torch

    values = words.copy()
    if poison_nil:  # the slab of a nil plaintext is ignored: it need not be zero
        per = ctx.L * ctx.degree
        for index, here in enumerate(mask):
            if not here:
                values[index * per:(index + 1) * per] = POISON_WORD - index
    _, view = _slab(ctx, len(words), values)
    capacity = len(want_body) if records_bytes is None else max(records_bytes, len(want_body))
    whole, records, start = _byte_buffer(b"", residue, capacity=capacity)
    flag = _flag()
    ctx.save_database_segment(view, _mask_tensor(mask), records_bytes=records_bytes, out=records, mismatch=flag)
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    written = len(want_body) if records_bytes is None else min(records_bytes, len(want_body))
    assert got[start:start + written].tobytes() == want_body[:written], residue
    assert (got[:start] == POISON_BYTE).all() and (got[start + written:] == POISON_BYTE).all(), residue
    assert int(flag.item()) == want_flag


@pytest.mark.parametrize("case", C.ALL, ids=C.case_id)
def test_save_matches_the_restatement_at_every_residue(case):
    """exactly the range's bytes are written: the 64 poisoned bytes on either side stay, and so does the slack up to the next
    aligned chunk; the poisoned slabs of nil plaintexts do not leak"""
    ctx = _context(case.params)
    plaintexts, body, _, _ = _reference(case)
    mask = C.mask_of(case)
    assert len(body) == ctx.database_file_byte_count(mask) - 5
    for residue in range(8):
        _save_and_check(ctx, _words(plaintexts, ctx), mask, body, residue)


@pytest.mark.parametrize("params", [C.PARAMS[0], C.PARAMS[5]], ids=lambda p: p.name)
@pytest.mark.parametrize("pattern", ["random", "run-one-nil"])
def test_masks_longer_than_one_trip_of_the_rank_kernel(params, pattern):
    """the prefix count walks the mask 1024 bytes a trip and carries the count from trip to trip: 2500 plaintexts are two whole
    trips and a ragged third, and the nil of "run-one-nil" lies in the second"""
    case = C.Case(params, pattern, 2500)
    ctx = _context(params)
    plaintexts, body, _, _ = _reference(case)
    mask = C.mask_of(case)
    assert 1024 < int((mask[:2048] != 0).sum()) and (pattern != "run-one-nil" or 1024 <= int(np.flatnonzero(mask == 0)[0]) < 2048)
    words = _words(plaintexts, ctx)
    _load_and_check(ctx, body, mask, words, 1)
    _save_and_check(ctx, words, mask, body, 6)


# ---- buffers that are too short ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in C.ALL if c.count == 13 or (c.count == 1 and c.pattern == "all")], ids=C.case_id)
def test_short_buffers_set_the_flag_and_bound_every_access(case):
    """records_bytes below count + S popcount: load reads what lies past it as zero (the bytes there are poison: a read would
    show) and sets bit 0; save writes nothing at or past it and sets bit 0.  A tag that contradicts the mask sets bit 1."""
    ctx = _context(case.params)
    plaintexts, body, _, _ = _reference(case)
    mask = C.mask_of(case)
    moduli = _moduli(ctx)
    words = _words(plaintexts, ctx)
    payload = ctx.database_file_payload_bytes()
    for short in sorted({1, 3, 8, payload, payload + 1} & set(range(1, len(body) + 1))):
        cut = len(body) - short
        residue = short % 8
        want = _words(R.deserialize_body(body[:cut], mask, ctx.degree, moduli), ctx)
        _load_and_check(ctx, body, mask, want, residue, records_bytes=cut, want_flag=1)
        _save_and_check(ctx, words, mask, body, residue, records_bytes=cut, want_flag=1)
    if len(body):
        _load_and_check(ctx, body, mask, words, 3, records_bytes=len(body), want_flag=0)
        flipped = bytearray(body)
        at = R.tag_offset(list(mask), case.count - 1, payload)
        flipped[at] ^= 1  # the payload bytes are where the mask says, so the words are the mask's
        last_nil = _words(R.deserialize_body(bytes(flipped), mask, ctx.degree, moduli), ctx)
        _load_and_check(ctx, bytes(flipped), mask, last_nil, 5, want_flag=2)


# ---- whole files, end to end -------------------------------------------------------------------------------------------------------
def _uniform(rng, shape_prefix, moduli, degree):
    rows = [rng.integers(0, q, size=tuple(shape_prefix) + (degree,), dtype=np.uint64) for q in moduli]
    return np.ascontiguousarray(np.stack(rows, axis=len(shape_prefix)))


@pytest.mark.parametrize("word32", [False, True], ids=["u64", "u32"])
def test_processed_database_round_trips_through_its_file(oracle, word32):
    """he_pir_process_database_device(_u32) -> save_database_file is the restatement's file of pir_database_reference's
    plaintexts; load_database_file of it gives back the identical slab and mask (trailing bytes ignored); and
    he_pir_compute_response_device(_u32) answers from the loaded database with the words it gives from the built one"""
    import torch

    if word32:  # test_database_on_a_uint32_parameter_set's set and shape: pack mode, one chunk
        degree, t = 4096, (1 << 16) + 1
        q = [(1 << 27) - 40959, (1 << 28) - 65535, (1 << 28) - 73727]
        ours, ref = heamd.BfvContext32(degree, t, q), oracle.BfvContext(degree, t, q, word_bits=32)
        dims, entry_size, count = [4, 3], 500, 100
    else:  # test_device_database_answers_queries' split shape: three chunks, rows 10 and 11 nil
        degree = 256
        t = oracle.generate_primes([17], True, degree)[0]
        q = oracle.generate_primes([40, 40, 40, 41], False, degree)
        ours, ref = heamd.BfvContext(degree, t, q), oracle.BfvContext(degree, t, q)
        dims, entry_size, count = [4, 3], 1100, 10
    rng = np.random.default_rng(411 + word32)
    entries = [rng.integers(0, 256, size=int(s), dtype=np.uint8).tobytes() for s in rng.integers(1, entry_size + 1, size=count)]
    entries[3] = bytes(len(entries[3]))
    want_db, want_present = refdb.process(oracle, ref, entries, dims, entry_size, True)
    database, present = ours.pir_process_database(entries, dims, entry_size, True)
    chunks = want_db.shape[0]
    moduli = [int(v) for v in q[:ours.L]]
    flat = want_db.reshape(-1, ours.L, degree)
    plaintexts = [flat[i].tolist() if here else None for i, here in enumerate(want_present.reshape(-1))]
    assert any(p is None for p in plaintexts) and any(p is not None for p in plaintexts)
    want_file = R.serialize(plaintexts, moduli)

    got_file = ours.save_database_file(database, present)
    assert got_file == want_file
    assert ours.scan_database_file(got_file)["present"].tolist() == want_present.reshape(-1).tolist()

    loaded, loaded_present = ours.load_database_file(want_file + b"\x02trailing")
    assert bool((loaded.reshape(-1) == database.reshape(-1)).all())
    assert bool((loaded_present.reshape(-1) == present.reshape(-1)).all())

    to_device = heamd.to_device32 if word32 else heamd.to_device
    dim0 = to_device(_uniform(rng, (dims[0], 2), moduli, degree))
    rest = to_device(_uniform(rng, (dims[1], 2), moduli, degree))
    key = to_device(_uniform(rng, (ours.L, 2), q, degree))
    built = ours.pir_compute_response(dims, dim0, rest, database, chunks, present_device=present, relinearization_key=key)
    answered = ours.pir_compute_response(dims, dim0, rest, loaded.reshape(database.shape), chunks,
                                         present_device=loaded_present.reshape(present.shape), relinearization_key=key)
    torch.cuda.synchronize()
    assert bool((built == answered).all()) and bool(built.any())


def test_empty_database_file():
    ctx = _context(C.PARAMS[0])
    import torch

    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    assert ctx.save_database_file(torch.empty(0, dtype=torch.int64, device="cuda"), empty) == R.header(0)
    database, present = ctx.load_database_file(R.header(0))
    assert database.numel() == 0 and present.numel() == 0
