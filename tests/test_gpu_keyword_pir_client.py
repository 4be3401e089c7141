"""The keyword-PIR client on the device against tests/keyword_pir_client_reference.py: byte for byte on values,
word for word on query ciphertexts -- no comparison here has a tolerance.

  bucket search  he_keyword_client_find_in_buckets_device over the hand-built table of tests/keyword_pir_client_cases.py, in both
                 forms, with the buckets pointer at 0, 1, 3 and 15 bytes inside a 16-byte line; the batch of distinct rows
  count          he_keyword_client_count_bucket_entries_device over the count cases and one batched call
  query words    he_keyword_client_generate_query_device against he_pir_generate_query_device on the Python hash_indices and against
                 the Python-integer client on the same seeds, on both slab words
  end to end     table -> process_database -> evaluation keys -> generate_query from keywords -> compute_response_to_query with
                 one database per sub-table -> decrypt_response and count_entries, nothing on the host in between
  footprint      the composite entries on tests/footprint.py arenas under both poisons, with and without a caller's workspace

Shapes are the smallest at which each branch exists."""
import collections
import ctypes

import numpy as np
import pytest

import heamd
import keyword_pir_client_cases as cases
import keyword_pir_client_reference as client
import keyword_pir_reference as kw
import pir_client_reference as index_client
import pir_database_reference as refdb
from test_gpu_pir_client import T17, as_bytes, check_footprint, device_indices, ring_for, seeds

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
FORMS = ("staged", "direct")


def at_offset(data, offset):
    """a uint8 device tensor holding `data` whose first byte lies `offset` bytes inside a 16-byte line"""
    import torch

    backing = torch.empty(len(data) + 32, dtype=torch.uint8, device="cuda")
    skew = (offset - backing.data_ptr()) % 16
    view = backing[skew: skew + len(data)]
    if len(data):
        view.copy_(torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()))
    assert len(data) == 0 or view.data_ptr() % 16 == offset
    return view


def device_blob(items):
    import torch

    blob, offsets = heamd.binding._blob(items)
    blob = np.concatenate([blob, np.zeros(1, dtype=np.uint8)])  # (an empty blob still has an address)
    return torch.from_numpy(blob).cuda(), torch.from_numpy(offsets.view(np.int64)).cuda()


def device_hashes(hashes):
    return device_indices(hashes)


# ---- the bucket search over the case table --------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("offset", cases.OFFSETS)
def test_find_in_buckets_over_the_case_table(form, offset):
    import torch

    for case in cases.CASES:
        if form == "staged" and case.entry_size > client.STAGED_ROW_LIMIT:
            continue
        capacity = client.value_capacity(case.entry_size)
        buckets = at_offset(b"".join(case.rows), offset).view(1, case.h, case.entry_size)
        keep = buckets.clone()
        # the values too start anywhere: at the complement of the buckets' offset
        values = at_offset(b"\xa5" * capacity, (16 - offset) % 16)
        got, sizes, status = heamd.BfvContext.keyword_pir_find_in_buckets(buckets, device_hashes([case.target]), form=form,
                                                                          out_values=values)
        assert int(status[0]) == case.status, (case.name, form, offset)
        assert int(sizes[0]) == case.size, (case.name, form, offset)
        assert bytes(got.cpu().numpy()) == client.padded_value(case.status, case.value, case.entry_size), (case.name, form, offset)
        assert torch.equal(buckets, keep)


def test_the_plan_names_the_form_on_each_side_of_the_budget():
    """None takes the plan's form: the outcome is that of the explicit form, and the staged form refuses a row beyond its budget"""
    by_size = {case.entry_size: case for case in cases.CASES}
    for entry_size, form in cases.FORMS.items():
        case = by_size[entry_size]
        assert client.find_form(entry_size) == form
        buckets = at_offset(b"".join(case.rows), 5).view(1, case.h, entry_size)
        got, sizes, status = heamd.BfvContext.keyword_pir_find_in_buckets(buckets, device_hashes([case.target]))
        assert (int(status[0]), int(sizes[0])) == (case.status, case.size)
        assert bytes(got.cpu().numpy()) == client.padded_value(case.status, case.value, entry_size)
        if form == "direct":
            with pytest.raises(heamd.HeError) as err:
                heamd.BfvContext.keyword_pir_find_in_buckets(buckets, device_hashes([case.target]), form="staged")
            assert err.value.name == "invalidArgument"


@pytest.mark.parametrize("form", FORMS)
def test_find_in_a_batch_of_distinct_rows(form):
    """several queries over h = 2, every (query, bucket) row different: a transposed index fails; then no query at all"""
    import torch

    data = b"".join(raw for rows, _, _, _ in cases.BATCH for raw in rows)
    buckets = at_offset(data, 3).view(len(cases.BATCH), cases.BATCH_H, cases.BATCH_E)
    hashes = device_hashes([target for _, target, _, _ in cases.BATCH])
    workspace = torch.full((len(cases.BATCH) * cases.BATCH_H * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    for ws in (None, workspace):
        got, sizes, status = heamd.BfvContext.keyword_pir_find_in_buckets(buckets, hashes, form=form, workspace=ws)
        assert status.tolist() == [s for _, _, s, _ in cases.BATCH]
        assert sizes.tolist() == [len(value) for _, _, _, value in cases.BATCH]
        for q, (_, _, s, value) in enumerate(cases.BATCH):
            assert bytes(got[q].cpu().numpy()) == client.padded_value(s, value, cases.BATCH_E), q
    assert int(workspace.count_nonzero()) == 0  # the records are zeroized
    none = heamd.BfvContext.keyword_pir_find_in_buckets(buckets[:0], hashes[:0], form=form)
    assert tuple(none[0].shape) == (0, client.value_capacity(cases.BATCH_E)) and none[2].numel() == 0


# ---- the count scan ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", (0, 5))
def test_count_bucket_entries(offset):
    for name, data, expected in cases.COUNT_CASES:
        replies = at_offset(data, offset).view(1, 1, len(data))
        assert heamd.BfvContext.keyword_pir_count_bucket_entries(replies).tolist() == [expected], name
    length = cases.COUNT_BATCH_LENGTH
    padded = b"".join(data + bytes(length - len(data)) for replies in cases.COUNT_BATCH for data in replies)
    replies = at_offset(padded, offset).view(len(cases.COUNT_BATCH), len(cases.COUNT_BATCH[0]), length)
    assert heamd.BfvContext.keyword_pir_count_bucket_entries(replies).tolist() == cases.COUNT_BATCH_EXPECTED
    assert heamd.BfvContext.keyword_pir_count_bucket_entries(replies[:0]).numel() == 0
    # more replies a query than a wave has lanes: 70 copies of the first query's replies
    many = at_offset(padded[:3 * length] * 70, offset).view(1, 210, length)
    assert heamd.BfvContext.keyword_pir_count_bucket_entries(many).tolist() == [70 * cases.COUNT_BATCH_EXPECTED[0]]


# ---- query words -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("word32", [False, True])
@pytest.mark.parametrize("dims,h", [([4, 3], 1), ([4, 3], 2), ([4, 3], 3), ([5], 1), ([5], 2), ([5], 3)])
def test_query_words_equal_the_index_client_on_the_python_indices(oracle, dims, h, word32):
    """N = 64, t = 65537, E = 20: six buckets per plaintext; bucket counts 70 and 28, where KEYWORDS holds a keyword whose first
    two candidates collide"""
    import torch

    ring = ring_for(oracle, 64, T17, word32)
    entry_count = int(np.prod(dims)) * 6 - 2
    assert entry_count in cases.COLLIDING
    p = client.plan(64, T17, dims, entry_count, 20, h)
    C, queries = p["query_ciphertext_count"], len(cases.KEYWORDS)
    keywords, offsets = device_blob(cases.KEYWORDS)
    rng = np.random.default_rng(sum(dims) + h)
    a_seeds, error_seeds = seeds(rng, queries, C), seeds(rng, queries, C)
    out, hashes = ring.ours.keyword_pir_generate_query(keywords, offsets, dims, entry_count, 20, h, ring.key, a_seeds, error_seeds)
    expected = [client.hash_and_indices(keyword, entry_count, h) for keyword in cases.KEYWORDS]
    assert [int(v) & kw.MASK64 for v in hashes.tolist()] == [hash_ for hash_, _ in expected]
    indices = [row for _, row in expected]
    assert tuple(out.shape) == (queries, C, 2, ring.L, 64)
    # he_pir_generate_query_device on the reference's indices and the same seeds
    direct, flag = ring.ours.pir_generate_query(device_indices(indices), dims, entry_count, 20, False, ring.key, a_seeds, error_seeds)
    assert torch.equal(out, direct) and int(flag.item()) == 0
    # the Python-integer client
    a_host, e_host = a_seeds.cpu().numpy(), error_seeds.cpu().numpy()
    words = np.stack([index_client.generate_query(ring.poly_ctx(ring.L), T17, p, indices[q], ring.s_eval,
                                                  [bytes(s) for s in a_host[q]], [bytes(s) for s in e_host[q]], ring.stream)
                      for q in range(queries)])
    assert np.array_equal(ring.to_host(out), words), (dims, h, word32)
    # an empty batch
    none = ring.ours.keyword_pir_generate_query(keywords, offsets[:1], dims, entry_count, 20, h, ring.key, a_seeds[:0],
                                                error_seeds[:0])
    assert tuple(none[0].shape) == (0, C, 2, ring.L, 64)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pack", "split"])
@pytest.mark.parametrize("degree", [64, 256])  # the rings of test_gpu_pir_client.py's end-to-end test
def test_keywords_to_values_on_the_device(oracle, degree, mode):
    import torch

    t = oracle.generate_primes([17], True, degree)[0]
    ours = heamd.BfvContext(degree, t, oracle.generate_primes([40, 40, 40, 41], False, degree))
    L, bpp, dims, h = ours.L, degree * 16 // 8, [4, 3], 2
    rng = np.random.default_rng(degree + (mode == "split"))
    if mode == "pack":
        entry_size, per_table, longest = 40, 30, 12  # several buckets per plaintext
    else:
        entry_size, per_table, longest = 2 * bpp + 76, 11, bpp  # three reply ciphertexts
    stored = [b"keyword %d" % k for k in range(14)] + [b"", b"empty value"]
    values = [bytes(rng.integers(0, 256, int(rng.integers(1, longest + 1)), dtype=np.uint8)) for _ in stored]
    values[-1] = b""  # a stored empty value
    config = heamd.CuckooTableConfig(h, 100, entry_size, bucket_count=h * per_table)
    table = heamd.KeywordPirTable(config, stored, values, seed=degree)
    assert (table.table_count, table.buckets_per_table, table.entry_count) == (h, per_table, len(stored))
    database, present = table.process_database(ours, dims, entry_size)
    plan = ours.keyword_pir_client_plan(dims, per_table, entry_size, h)
    chunks = plan["reply_ciphertext_count"]
    assert chunks == database.shape[1] == (1 if mode == "pack" else 3)
    assert (plan["entries_per_plaintext"] > 1) == (mode == "pack")
    key = ours.generate_secret_key(seeds(rng, 1))[0].contiguous()
    elements = ours.pir_evaluation_key_elements(plan["expanded_query_count"], "none")
    galois = ours.generate_galois_keys(key, elements, seeds(rng, len(elements), L), seeds(rng, len(elements), L))
    relin = ours.generate_relinearization_key(key, seeds(rng, L), seeds(rng, L))
    asked = stored + [b"absent", b"keyword 14", b"Keyword 0"]
    keywords, offsets = device_blob(asked)
    C, queries = plan["query_ciphertext_count"], len(asked)
    query, hashes = ours.keyword_pir_generate_query(keywords, offsets, dims, per_table, entry_size, h, key, seeds(rng, queries, C),
                                                    seeds(rng, queries, C))
    response = torch.stack([ours.pir_compute_response_to_query(dims, query[q], h, {e: galois[k] for k, e in enumerate(elements)},
                                                               relin, [database[i] for i in range(h)], chunks,
                                                               present_devices=[present[i] for i in range(h)])
                            for q in range(queries)]).contiguous()
    got, sizes, status = ours.keyword_pir_decrypt_response(response, dims, per_table, entry_size, key, keywords=keywords,
                                                           keyword_offsets=offsets)
    again = ours.keyword_pir_decrypt_response(response, dims, per_table, entry_size, key, hashes=hashes)
    counts = ours.keyword_pir_count_entries(response, dims, per_table, entry_size, key)
    full, _ = ours.pir_decrypt_response(response, None, dims, per_table, entry_size, False, key)
    # everything above stayed on the device; from here on the host looks at the results
    for first, second in zip((got, sizes, status), again):
        assert torch.equal(first, second)
    capacity = client.value_capacity(entry_size)
    assert tuple(got.shape) == (queries, capacity)
    for q, keyword in enumerate(asked):
        if keyword in stored:
            value = values[stored.index(keyword)]
            assert (int(status[q]), int(sizes[q])) == (client.FOUND, len(value)), keyword
            assert bytes(got[q].cpu().numpy()) == value + bytes(capacity - len(value)), keyword
        else:
            assert (int(status[q]), int(sizes[q])) == (client.NIL, 0), keyword
            assert not got[q].any()
    assert int(sizes[stored.index(b"empty value")]) == 0 and int(status[stored.index(b"empty value")]) == client.FOUND
    full_host = full.cpu().numpy()
    assert full_host.shape == (queries, h, plan["reply_bytes"])
    expected = [client.count_entries([bytes(full_host[q, i]) for i in range(h)]) for q in range(queries)]
    assert counts.tolist() == expected and max(expected) >= 1


# ---- footprint -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("word32", [False, True])
def test_generate_query_footprint(oracle, word32):
    ring = ring_for(oracle, 64, T17, word32)
    lib, bits, word_bytes = heamd.load_library(), 32 if word32 else 64, 4 if word32 else 8
    dims, entries, h = (ctypes.c_uint32 * 2)(4, 3), 70, 3
    asked = cases.KEYWORDS[:4]
    queries = len(asked)
    p = client.plan(64, T17, [4, 3], entries, 20, h)
    C = p["query_ciphertext_count"]
    rng = np.random.default_rng(21)
    keywords, offsets = device_blob(asked)
    inputs = collections.OrderedDict([("keywords", as_bytes(keywords)), ("keyword_offsets", as_bytes(offsets)),
                                      ("secret_key", as_bytes(ring.key)), ("a_seeds", as_bytes(seeds(rng, queries, C))),
                                      ("error_seeds", as_bytes(seeds(rng, queries, C)))])
    parameter = (dims, 2, entries, 20, h)
    needed = int(lib.he_keyword_client_generate_query_workspace_bytes(ring.ours.h, bits, *parameter, queries))

    def invoke(at, nbytes):
        return lib.he_keyword_client_generate_query_device(ring.ours.h, bits, *parameter, vp(at["keywords"]), vp(at["keyword_offsets"]),
                                                        queries, vp(at["secret_key"]), vp(at["a_seeds"]), vp(at["error_seeds"]),
                                                        vp(at["out"]), vp(at["out_hashes"]), vp(at["workspace"]), nbytes, None)

    got = check_footprint("he_keyword_client_generate_query_device u%d" % bits, inputs,
                          {"out": queries * C * 2 * ring.L * 64 * word_bytes, "out_hashes": queries * 8}, {}, needed, invoke)
    expected = [client.hash_and_indices(keyword, entries, h) for keyword in asked]
    assert list(got["out_hashes"].view(np.uint64)) == [hash_ for hash_, _ in expected]
    a_host = inputs["a_seeds"].cpu().numpy().reshape(queries, C, 32)
    e_host = inputs["error_seeds"].cpu().numpy().reshape(queries, C, 32)
    words = np.stack([index_client.generate_query(ring.poly_ctx(ring.L), T17, p, expected[q][1], ring.s_eval,
                                                  [bytes(s) for s in a_host[q]], [bytes(s) for s in e_host[q]], ring.stream)
                      for q in range(queries)])
    assert np.array_equal(got["out"].view(np.uint32 if word32 else np.uint64).astype(np.uint64), words.reshape(-1))


def replies_holding(oracle, rng, p, rows, indices):
    """[h][R][N] coefficients of a query's replies: random byte strings but for bucket row i at the position of indices[i]"""
    bpp, R, size = p["bytes_per_plaintext"], p["reply_ciphertext_count"], p["entry_size"]
    out = []
    for raw, index in zip(rows, indices):
        data = bytearray(rng.integers(0, 256, R * bpp, dtype=np.uint8).tobytes())
        start = (index % p["entries_per_plaintext"]) * size
        data[start:start + size] = raw
        out.append(np.stack([refdb.unpack(oracle, bytes(data[k * bpp:(k + 1) * bpp]), p["bits"], p["degree"]) for k in range(R)]))
    return np.stack(out)


@pytest.mark.parametrize("word32", [False, True])
@pytest.mark.parametrize("mode", ["pack", "split"])
def test_decrypt_response_and_count_entries_footprint(oracle, mode, word32):
    """replies made by encrypting chosen bucket rows at one modulus: a found value, a nil and a corrupt bucket"""
    ring = ring_for(oracle, 64, T17, word32)
    lib, bits = heamd.load_library(), 32 if word32 else 64
    h, entry_size = 2, 40 if mode == "pack" else 300
    entries = 12 * (128 // entry_size if mode == "pack" else 1) - 1
    p = client.plan(64, T17, [4, 3], entries, entry_size, h)
    R = p["reply_ciphertext_count"]
    assert (p["entries_per_plaintext"], R) == ((3, 1) if mode == "pack" else (1, 3))
    asked = [b"found", b"", b"corrupt"]
    queries = len(asked)
    derived = [client.hash_and_indices(keyword, entries, h) for keyword in asked]
    size = 17 if mode == "pack" else 270
    rows = [[cases.row([(cases.A, b"x")], entry_size), cases.row([(cases.B, b"y"), (derived[0][0], cases.pattern(size, 2))], entry_size)],
            [cases.row([(cases.A, b"z")], entry_size), bytes(entry_size)],
            [cases.row([(cases.C, b"")], entry_size), bytes([255]) + bytes(entry_size - 1)]]  # 255 slots need 2551 bytes
    rng = np.random.default_rng(len(mode) + word32)
    plaintexts = np.stack([replies_holding(oracle, rng, p, rows[q], derived[q][1]) for q in range(queries)])
    count = queries * h * R
    cts = ring.ours.encrypt(ring.to_device(plaintexts.reshape(-1, 64)), ring.key, seeds(rng, count), seeds(rng, count), moduli_count=1)
    keywords, offsets = device_blob(asked)
    inputs = collections.OrderedDict([("response", as_bytes(cts)), ("keywords", as_bytes(keywords)),
                                      ("keyword_offsets", as_bytes(offsets)), ("secret_key", as_bytes(ring.key[:1]))])
    parameter = ((ctypes.c_uint32 * 2)(4, 3), 2, entries, entry_size, h)
    needed = int(lib.he_keyword_client_decrypt_response_workspace_bytes(ring.ours.h, bits, *parameter, 1, queries))

    def invoke(at, nbytes):
        return lib.he_keyword_client_decrypt_response_device(ring.ours.h, bits, *parameter, 1, vp(at["response"]), vp(at["keywords"]),
                                                          vp(at["keyword_offsets"]), None, queries, vp(at["secret_key"]),
                                                          vp(at["out_values"]), vp(at["out_sizes"]), vp(at["out_status"]),
                                                          vp(at["workspace"]), nbytes, None)

    capacity = p["value_capacity"]
    got = check_footprint("he_keyword_client_decrypt_response_device u%d %s" % (bits, mode), inputs,
                          {"out_values": queries * capacity, "out_sizes": queries * 8, "out_status": queries * 4}, {}, needed, invoke)
    expected = [client.find_in_buckets(rows[q], derived[q][0]) for q in range(queries)]
    assert [status for status, _, _ in expected] == [client.FOUND, client.NIL, client.CORRUPT]
    assert list(got["out_status"].view(np.uint32)) == [status for status, _, _ in expected]
    assert list(got["out_sizes"].view(np.uint64)) == [size_ for _, size_, _ in expected]
    assert bytes(got["out_values"]) == b"".join(client.padded_value(status, value, entry_size) for status, _, value in expected)

    needed = int(lib.he_keyword_client_count_entries_workspace_bytes(ring.ours.h, bits, *parameter, 1, queries))
    del inputs["keywords"], inputs["keyword_offsets"]

    def invoke_count(at, nbytes):
        return lib.he_keyword_client_count_entries_device(ring.ours.h, bits, *parameter, 1, vp(at["response"]), queries,
                                                       vp(at["secret_key"]), vp(at["out_counts"]), vp(at["workspace"]), nbytes, None)

    got = check_footprint("he_keyword_client_count_entries_device u%d %s" % (bits, mode), inputs, {"out_counts": queries * 8}, {},
                          needed, invoke_count)
    full = [[index_client.reply_bytes(oracle, plaintexts[q, i], p["bits"]) for i in range(h)] for q in range(queries)]
    assert list(got["out_counts"].view(np.uint64)) == [client.count_entries(replies) for replies in full]
