"""The PNNS client on the device against tests/pnns_client_reference.py and the restatements under it: word
for word, and bit for bit on the floats -- no comparison here has a tolerance.

  layer 1  simd_encode / simd_decode against the numpy SimdEncoder over the oracle's transform
  layer 2  pack_dense_rows against denseRowPlaintexts restated line by line, unpack against unpackDenseRow / unpackDenseColumn
  layer 3  generate_query against quantise -> restated packing -> he_bfv_encrypt_device on the same seeds and against the
           Python-integer client; decrypt_response against he_bfv_decrypt_device -> restated unpack / compose / scale and
           against the Python-integer client; composed values at the centring thresholds; float database and float queries
           through process_database, generate_query, device-made Galois keys, compute_response_matrix and decrypt_response
           against the restated fixedPointCosineSimilarity

Shapes are the smallest at which each branch exists; the comment next to a shape names the branch."""

import numpy as np
import pytest

import encrypt_reference
import heamd
import pnns_client_reference as client
import pnns_matrix_reference as pm
import pnns_reference as pnns
from test_gpu_pnns import Setup
from test_gpu_pnns_matrix import element_of_for
from test_gpu_pnns_response import get_setup, to_device, uniform_words
from test_pnns_client_reference import T17, T17B

pytestmark = pytest.mark.gpu

# (N, L, rows, cols) for pack_dense_rows; rows per plaintext is N / nextPowerOfTwo(cols)
DENSE_ROW = [
    (64, 3, 1, 4),      # one row: 4 values repeated over every slot
    (64, 3, 3, 4),      # one plaintext, 12 values padded to 16 and repeated four times
    (64, 3, 5, 3),      # column padding: 20 values padded to 32, the second SIMD row repeats the first
    (64, 3, 20, 4),     # two plaintexts; the last holds 16 values: part of one SIMD row, repeated
    (64, 3, 27, 4),     # the last holds 44 values: a full SIMD row and 12 of the second, padded to 16 and repeated there
    (64, 3, 3, 32),     # P = N / 2: a row is a SIMD row; the last plaintext holds one and repeats it
    (64, 3, 16, 4),     # the last plaintext exactly full: nothing repeats
    (1024, 3, 5, 16),   # the tiled transform
    (4096, 4, 3, 16),   # L = 4
]
# (N, rows, cols) for the dense-column unpack: cols is the query's row count
DENSE_COLUMN = [
    (64, 10, 3),    # one plaintext, one SIMD row
    (64, 10, 5),    # both SIMD rows, padding behind three columns
    (64, 10, 7),    # two plaintexts, a ragged last one
    (64, 32, 3),    # one column per SIMD row
    (64, 70, 3),    # a column spans two plaintexts
    (1024, 100, 5),
]

_setups = {}


def setup_for(oracle, degree, word32=False, t=None):
    """the shared setups of the PNNS files, or one of its own for another plaintext modulus over the same coefficient moduli"""
    if t is None:
        return get_setup(oracle, degree, word32=word32)
    key = (degree, word32, t)
    if key not in _setups:
        _setups[key] = Setup(oracle, degree, word32, t=t)
    return _setups[key]


def pair_of_contexts(oracle, degree):
    """two contexts that differ in the plaintext modulus alone, about 17 bits each: q > 2^26, Float(signed) rounds"""
    return [setup_for(oracle, degree, t=T17), setup_for(oracle, degree, t=T17B)]


def torch_words(s, array):
    return to_device(s, np.ascontiguousarray(array, dtype=np.uint64))


def device_seeds(rng, *shape):
    import torch

    return torch.from_numpy(rng.integers(0, 256, size=shape + (32,), dtype=np.uint8)).cuda()


def secret_key_of(s, rng):
    return s.bfv.generate_secret_key(device_seeds(rng, 1))[0].contiguous()


def bits(floats):
    return np.ascontiguousarray(floats, dtype=np.float32).view(np.uint32)


# ---- layer 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree,word32", [(64, False), (64, True), (1024, False), (1024, True), (4096, False)])
def test_simd_encode_and_decode(oracle, degree, word32):
    import torch

    s = setup_for(oracle, degree, word32)
    rng = np.random.default_rng(degree + word32)
    slots = rng.integers(0, s.t, size=(3, degree), dtype=np.uint64)
    slots[0, :4] = [s.t - 1, 0, 1, s.t - 1]
    slots[1] = s.t - 1
    slots[2, degree // 2:] = 0  # fewer than N values: the caller pads with zeros
    device_slots = torch_words(s, slots)
    plaintexts, flag = s.pnns.simd_encode(device_slots)
    expected = s.encoder.encode(slots)
    assert np.array_equal(s.to_host(plaintexts), expected) and expected.any()
    assert int(flag.item()) == 0
    assert np.array_equal(s.to_host(device_slots), slots)
    keep = plaintexts.clone()
    assert np.array_equal(s.to_host(s.pnns.simd_decode(plaintexts)), slots)
    assert torch.equal(plaintexts, keep)  # the input is never written
    coefficients = rng.integers(0, s.t, size=(2, degree), dtype=np.uint64)
    assert np.array_equal(s.to_host(s.pnns.simd_decode(torch_words(s, coefficients))), s.encoder.decode(coefficients))
    slots[1, degree - 1] = s.t  # not below t: validDataForEncoding
    assert int(s.pnns.simd_encode(torch_words(s, slots))[1].item()) == 1
    assert tuple(s.pnns.simd_encode(torch_words(s, slots[:0]))[0].shape) == (0, degree)


# ---- layer 2 -------------------------------------------------------------------------------------------------------------------
def check_dense_rows(s, rows, cols, seed):
    import torch

    t, n = s.t, s.degree
    rng = np.random.default_rng(seed)
    least, most = -(t >> 1), (t - 1) >> 1
    count = pnns.plaintext_count(n, rows, cols, "denseRow")
    values = rng.integers(least, most + 1, size=(rows, cols), dtype=np.int64)
    values.reshape(-1)[:2] = [least, most][:values.size]
    values[-1, -1] = least if values.size > 2 else values[-1, -1]
    for reduce in (False, True):
        if reduce:  # magnitudes above t and near +-2^62, the multiples of t
            values = rng.integers(-(1 << 62), 1 << 62, size=(rows, cols), dtype=np.int64)
            edge = [(1 << 62) - 1, -(1 << 62), t, -t, t + 1, -t - 1][:values.size]
            values.reshape(-1)[:len(edge)] = edge
        residues, outside = client.signed_to_residues(values, t, reduce)
        assert not outside
        expected = s.encoder.encode(pm.dense_row_slots(residues, rows, cols, n))
        plaintexts, flag = s.pnns.pack_dense_rows(torch.from_numpy(values).cuda(), reduce=reduce)
        label = (n, s.word32, rows, cols, reduce)
        assert tuple(plaintexts.shape) == (count, n), label
        assert np.array_equal(s.to_host(plaintexts), expected) and expected.any(), label
        assert int(flag.item()) == 0, label
        unpacked = s.pnns.unpack(plaintexts, rows, cols, "denseRow")
        assert np.array_equal(heamd.to_host(unpacked), residues), label
        assert np.array_equal(client.unpack_dense_row(s.encoder.decode(expected), rows, cols, n), residues), label
    # one outside either end of the centred range sets the flag (reduce off), and only there
    for bad in (least - 1, most + 1):
        values = np.zeros((rows, cols), dtype=np.int64)
        values[-1, -1] = bad
        assert int(s.pnns.pack_dense_rows(torch.from_numpy(values).cuda())[1].item()) == 1, bad
        assert int(s.pnns.pack_dense_rows(torch.from_numpy(values).cuda(), reduce=True)[1].item()) == 0, bad


@pytest.mark.parametrize("degree,L,rows,cols", DENSE_ROW)
def test_pack_dense_rows(oracle, degree, L, rows, cols):
    s = setup_for(oracle, degree)
    assert s.ref.L == L
    check_dense_rows(s, rows, cols, 1000 * degree + 10 * rows + cols)


@pytest.mark.parametrize("degree,L,rows,cols", [row for row in DENSE_ROW if row[0] in (64, 1024)])
def test_pack_dense_rows_u32(oracle, degree, L, rows, cols):
    check_dense_rows(setup_for(oracle, degree, word32=True), rows, cols, 32 * degree + 10 * rows + cols)


@pytest.mark.parametrize("degree,rows,cols", DENSE_COLUMN)
@pytest.mark.parametrize("word32", [False, True])
def test_unpack_dense_columns(oracle, degree, rows, cols, word32):
    import torch

    s = setup_for(oracle, degree, word32)
    count = pnns.plaintext_count(degree, rows, cols, "denseColumn")
    rng = np.random.default_rng(degree + rows + cols)
    slots = rng.integers(0, s.t, size=(count, degree), dtype=np.uint64)
    slots[0, 0], slots[-1, -1] = s.t - 1, s.t - 1
    plaintexts = torch_words(s, s.encoder.encode(slots))
    keep = plaintexts.clone()
    got = heamd.to_host(s.pnns.unpack(plaintexts, rows, cols, "denseColumn"))
    assert got.shape == (rows, cols)
    assert np.array_equal(got, client.unpack_dense_column(slots, rows, cols, degree))
    assert np.array_equal(got, pm.unpack_dense_column(slots, rows, cols, degree))
    assert torch.equal(plaintexts, keep)
    with pytest.raises(heamd.HeError) as err:
        s.pnns.unpack(plaintexts, rows, cols, "diagonal")
    assert err.value.name == "unsupportedHeOperation"


# ---- layer 3: composition thresholds ---------------------------------------------------------------------------------------------
def dense_column_slots(values, degree):
    """the slots unpackDenseColumn reads values [rows][cols] from, everything else zero: [M][N]"""
    rows, cols = values.shape
    count = pnns.plaintext_count(degree, rows, cols, "denseColumn")
    where = client.unpack_dense_column(np.arange(count * degree, dtype=np.uint64).reshape(count, degree), rows, cols, degree)
    slots = np.zeros(count * degree, dtype=np.uint64)
    slots[where.astype(np.int64)] = values
    return slots.reshape(count, degree)


def encrypted_response(setups, composed, key, rng, moduli_count=1):
    """composed [rows][query_rows] values mod q -> [contexts][M][2][moduli_count][N]: residues packed by columns on the host,
    encoded by simd_encode, encrypted by he_bfv_encrypt_device"""
    import torch

    out = []
    for s in setups:
        residues = np.vectorize(lambda v, t=s.t: int(v) % t, otypes=[np.uint64])(composed)
        plaintexts, flag = s.pnns.simd_encode(torch_words(s, dense_column_slots(residues, s.degree)))
        assert int(flag.item()) == 0
        count = plaintexts.shape[0]
        out.append(s.bfv.encrypt(plaintexts, key, device_seeds(rng, count), device_seeds(rng, count), moduli_count=moduli_count))
    return torch.stack(out).contiguous()


@pytest.mark.parametrize("rows,query_rows", [(10, 5), (70, 3)])
def test_composed_values_at_the_centring_thresholds(oracle, rows, query_rows):
    setups = pair_of_contexts(oracle, 64)
    moduli = [s.t for s in setups]
    q = moduli[0] * moduli[1]
    assert q > 1 << 26
    rng = np.random.default_rng(rows)
    composed = np.array([int(v) for v in rng.integers(0, q, size=rows * query_rows, dtype=np.uint64)], dtype=object)
    special = [0, 1, (q - 1) >> 1, ((q - 1) >> 1) + 1, q - 1, (1 << 24) + 1, (1 << 25) + 2, q - (1 << 24) - 3]
    composed[:len(special)] = special
    composed[-len(special):] = special[::-1]  # in the last column (and the last plaintext) too
    composed = composed.reshape(rows, query_rows)
    key = secret_key_of(setups[0], rng)
    response = encrypted_response(setups, composed, key, rng)
    contexts = [s.pnns for s in setups]
    for scaling_factor in (1, 180):
        got = heamd.pnns_decrypt_response(contexts, response, key, rows, query_rows, scaling_factor).cpu().numpy()
        expected = np.zeros((rows, query_rows), dtype=np.float32)
        for index in np.ndindex(rows, query_rows):
            expected[index] = client.scale_distance(client.remainder_to_centered(int(composed[index]), q), scaling_factor)
        assert np.array_equal(bits(got), bits(expected)), scaling_factor
        if scaling_factor == 1:
            flat = got.reshape(-1)
            assert flat[0] == 0 and flat[1] == 1 and flat[2] == np.float32((q - 1) >> 1)
            assert flat[3] == -np.float32((q - 1) >> 1) and flat[4] == -1  # ((q - 1) >> 1) + 1 - q = -((q - 1) >> 1)
    # one context: no composition, the centring is that of t
    one = heamd.pnns_decrypt_response(contexts[:1], response[:1], key, rows, query_rows, 3).cpu().numpy()
    t = moduli[0]
    expected = np.vectorize(lambda v: client.scale_distance(client.remainder_to_centered(int(v) % t, t), 3),
                            otypes=[np.float32])(composed)
    assert np.array_equal(bits(one), bits(expected))


# ---- layer 3: composition equality -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree,contexts,query_rows,cols,word32", [(64, 1, 5, 4, False), (64, 2, 5, 4, False), (64, 2, 20, 3, False),
                                                                     (64, 1, 5, 4, True), (1024, 2, 5, 16, False)])
def test_generate_query_is_quantise_pack_encrypt(oracle, degree, contexts, query_rows, cols, word32):
    import torch

    if word32:
        setups = [setup_for(oracle, degree, word32=True)]
    else:
        setups = pair_of_contexts(oracle, degree)[:contexts]
    rng = np.random.default_rng(degree + query_rows + contexts)
    vectors = rng.standard_normal((query_rows, cols)).astype(np.float32)
    scaling_factor = client.max_scaling_factor(cols, [s.t for s in setups])
    count = pnns.plaintext_count(degree, query_rows, cols, "denseRow")
    key = secret_key_of(setups[0], rng)
    a_seeds, error_seeds = device_seeds(rng, contexts, count), device_seeds(rng, contexts, count)
    device_vectors = torch.from_numpy(vectors).cuda()
    queries, flag = heamd.pnns_generate_query([s.pnns for s in setups], device_vectors, scaling_factor, key, a_seeds, error_seeds)
    assert tuple(queries.shape) == (contexts, count, 2, setups[0].bfv.L, degree) and int(flag.item()) == 0
    rounded = setups[0].pnns.quantize_rows(device_vectors, scaling_factor)
    assert np.array_equal(rounded.cpu().numpy(), pnns.normalized_scaled_and_rounded(vectors, scaling_factor))
    for c, s in enumerate(setups):
        plaintexts, outside = client.query_plaintexts(s.encoder, vectors, scaling_factor, reduce=contexts > 1)
        assert not outside
        composed = s.bfv.encrypt(torch_words(s, plaintexts), key, a_seeds[c], error_seeds[c])
        assert torch.equal(queries[c], composed), c
        # the device's own layer 2 in between gives the same words
        packed, _ = s.pnns.pack_dense_rows(rounded, reduce=contexts > 1)
        assert np.array_equal(s.to_host(packed), plaintexts), c


def test_generate_query_and_decrypt_response_equal_the_python_integer_client(oracle):
    """N = 64, two contexts, 5 x 4 query, 10-row database: every word and every float from tests/pnns_client_reference.py, whose
    encryption and decryption are Python integers over the oracle's transforms"""
    import torch

    setups = pair_of_contexts(oracle, 64)
    rng = np.random.default_rng(5)
    query_rows, cols, rows = 5, 4, 10
    vectors = rng.standard_normal((query_rows, cols)).astype(np.float32)
    scaling_factor = client.max_scaling_factor(cols, [s.t for s in setups])
    count = pnns.plaintext_count(64, query_rows, cols, "denseRow")
    stream = encrypt_reference.oracle_stream(oracle)
    key_seed = rng.integers(0, 256, size=(1, 32), dtype=np.uint8)
    key = setups[0].bfv.generate_secret_key(torch.from_numpy(key_seed).cuda())[0].contiguous()
    secret_ctx = oracle.PolyContext(64, setups[0].q)
    s_eval = encrypt_reference.generate_secret_key(secret_ctx, bytes(key_seed[0]), stream)
    assert np.array_equal(heamd.to_host(key), s_eval)
    a_seeds = rng.integers(0, 256, size=(2, count, 32), dtype=np.uint8)
    error_seeds = rng.integers(0, 256, size=(2, count, 32), dtype=np.uint8)
    queries, _ = heamd.pnns_generate_query([s.pnns for s in setups], torch.from_numpy(vectors).cuda(), scaling_factor, key,
                                           torch.from_numpy(a_seeds).cuda(), torch.from_numpy(error_seeds).cuda())
    expected = client.generate_query([s.ref for s in setups], [s.encoder for s in setups], vectors, scaling_factor, s_eval,
                                     [[bytes(seed) for seed in row] for row in a_seeds],
                                     [[bytes(seed) for seed in row] for row in error_seeds], stream)
    assert np.array_equal(heamd.to_host(queries), expected)
    # a response with known distances, decrypted by both
    q = setups[0].t * setups[1].t
    composed = np.array([int(v) for v in rng.integers(0, q, size=rows * query_rows, dtype=np.uint64)], dtype=object)
    response = encrypted_response(setups, composed.reshape(rows, query_rows), key, rng)
    got = heamd.pnns_decrypt_response([s.pnns for s in setups], response, key, rows, query_rows, scaling_factor).cpu().numpy()
    reference = client.decrypt_response([s.ref for s in setups], [s.encoder for s in setups], heamd.to_host(response), s_eval, rows,
                                        query_rows, scaling_factor)
    assert np.array_equal(bits(got), bits(reference))


def check_decrypt_response(setups, rows, query_rows, moduli_count, seed, scaling_factor=180):
    """uniform ciphertext words (word equality needs no valid encryption): the entry against he_bfv_decrypt_device, the numpy
    decoder and the restated unpack / compose / scale"""
    import torch

    s0 = setups[0]
    n = s0.degree
    rng = np.random.default_rng(seed)
    count = pnns.plaintext_count(n, rows, query_rows, "denseColumn")
    response = to_device(s0, uniform_words(rng, list(s0.q[:moduli_count]), (len(setups), count, 2), n))
    key = to_device(s0, uniform_words(rng, list(s0.q), (), n))
    keep = response.clone()
    got = heamd.pnns_decrypt_response([s.pnns for s in setups], response, key, rows, query_rows, scaling_factor).cpu().numpy()
    unpacked = []
    for c, s in enumerate(setups):
        plaintexts = s.to_host(s.bfv.decrypt(response[c], key))
        unpacked.append(client.unpack_dense_column(s.encoder.decode(plaintexts), rows, query_rows, n))
    expected = client.distances_from_residues(unpacked, [s.t for s in setups], scaling_factor)
    assert got.shape == (rows, query_rows) and np.array_equal(bits(got), bits(expected))
    assert torch.equal(response, keep)
    return got


@pytest.mark.parametrize("degree,rows,query_rows", DENSE_COLUMN)
def test_decrypt_response_is_decrypt_unpack_compose_scale(oracle, degree, rows, query_rows):
    check_decrypt_response(pair_of_contexts(oracle, degree), rows, query_rows, 1, degree + rows)
    check_decrypt_response(pair_of_contexts(oracle, degree)[:1], rows, query_rows, 1, degree + rows + 1)


def test_decrypt_response_at_any_level_and_on_4_byte_words(oracle):
    setups = pair_of_contexts(oracle, 64)
    for moduli_count in (2, 3):
        check_decrypt_response(setups, 10, 7, moduli_count, moduli_count)
    check_decrypt_response([setup_for(oracle, 64, word32=True)], 10, 7, 1, 32)
    check_decrypt_response([setup_for(oracle, 1024, word32=True)], 100, 5, 1, 33)


def test_plaintext_groups_give_identical_distances(oracle, monkeypatch):
    """HEAMD_PNNS_CLIENT_GROUP: one plaintext to a group, and groups of 4 + 2, on the shape whose columns span plaintexts
    (M = 6) and on the one with a ragged last plaintext (M = 2)"""
    setups = pair_of_contexts(oracle, 64)
    for rows, query_rows in ((70, 3), (10, 7)):
        monkeypatch.delenv("HEAMD_PNNS_CLIENT_GROUP", raising=False)
        whole = check_decrypt_response(setups, rows, query_rows, 1, 77)
        for group in ("1", "4"):
            monkeypatch.setenv("HEAMD_PNNS_CLIENT_GROUP", group)
            assert np.array_equal(bits(check_decrypt_response(setups, rows, query_rows, 1, 77)), bits(whole)), (rows, group)


# ---- end to end: nothing on the host between the floats --------------------------------------------------------------------------
@pytest.mark.parametrize("degree,contexts,rows,cols,query_rows", [(64, 1, 10, 4, 5), (64, 2, 10, 4, 5), (1024, 1, 100, 16, 5)])
def test_float_queries_to_float_distances(oracle, degree, contexts, rows, cols, query_rows):
    import torch

    setups = pair_of_contexts(oracle, degree)[:contexts]
    moduli = [s.t for s in setups]
    q = int(np.prod([int(t) for t in moduli], dtype=object))
    scaling_factor = client.max_scaling_factor(cols, moduli)
    rng = np.random.default_rng(degree + contexts)
    database = rng.standard_normal((rows, cols)).astype(np.float32)
    vectors = rng.standard_normal((query_rows, cols)).astype(np.float32)
    vectors[0], vectors[1] = database[3], -database[4]  # cosines of +1 and -1: the largest products
    s0 = setups[0]
    bfv, L = s0.bfv, s0.bfv.L
    key = secret_key_of(s0, rng)
    count = pnns.plaintext_count(degree, query_rows, cols, "denseRow")
    queries, flag = heamd.pnns_generate_query([s.pnns for s in setups], torch.from_numpy(vectors).cuda(), scaling_factor, key,
                                              device_seeds(rng, contexts, count), device_seeds(rng, contexts, count))
    assert int(flag.item()) == 0
    # the evaluation key: BFV's does not depend on the plaintext modulus (Client.swift:141-146)
    baby_step = pnns.baby_step_giant_step(cols)[0]
    element_of = element_of_for(degree)
    steps = [-1, -baby_step, "swap", pnns.next_power_of_two(cols), rows]
    galois = bfv.generate_galois_keys(key, [element_of(step) for step in steps], device_seeds(rng, len(steps), L),
                                      device_seeds(rng, len(steps), L))
    keys = [[galois[k] for k in range(len(steps))]]
    assert "pack" in pm.needs(degree, rows, cols, query_rows)
    responses = []
    for c, s in enumerate(setups):
        matrix, outside = s.pnns.process_database(torch.from_numpy(database).cuda(), scaling_factor, reduce=contexts > 1)
        assert int(outside.item()) == 0
        responses.append(s.pnns.compute_response_matrix(matrix, rows, cols, queries[c:c + 1], query_rows, [(rows, 1)], keys)[0])
    response = torch.stack(responses).contiguous()
    distances = heamd.pnns_decrypt_response([s.pnns for s in setups], response, key, rows, query_rows, scaling_factor)
    expected = client.fixed_point_cosine_similarity(database, vectors, q, scaling_factor)
    assert distances.dtype == torch.float32 and tuple(distances.shape) == (rows, query_rows)
    assert np.array_equal(bits(distances.cpu().numpy()), bits(expected))
    assert abs(float(expected[3, 0]) - 1) < 0.05 and abs(float(expected[4, 1]) + 1) < 0.05


# ---- streams and scratch ---------------------------------------------------------------------------------------------------------
def test_back_to_back_calls_and_a_side_stream(oracle):
    """generate_query twice and decrypt_response twice on one side stream with no host synchronisation in between (they share
    the stream-ordered scratch) give what the same calls give on the default stream, each followed by a synchronisation"""
    import torch

    setups = pair_of_contexts(oracle, 1024)
    contexts = [s.pnns for s in setups]
    rng = np.random.default_rng(9)
    key = secret_key_of(setups[0], rng)
    shapes = [(5, 16), (70, 3)]
    inputs = []
    for query_rows, cols in shapes:
        count = pnns.plaintext_count(1024, query_rows, cols, "denseRow")
        inputs.append((torch.from_numpy(rng.standard_normal((query_rows, cols)).astype(np.float32)).cuda(),
                       device_seeds(rng, 2, count), device_seeds(rng, 2, count)))
    rows, query_rows = 100, 5
    responses = [to_device(setups[0], uniform_words(rng, list(setups[0].q[:1]),
                                                    (2, pnns.plaintext_count(1024, rows, query_rows, "denseColumn"), 2), 1024))
                 for _ in range(2)]
    torch.cuda.synchronize()
    apart = []
    for vectors, a_seeds, error_seeds in inputs:
        apart.append(heamd.pnns_generate_query(contexts, vectors, 100, key, a_seeds, error_seeds)[0])
        torch.cuda.synchronize()
    for response in responses:
        apart.append(heamd.pnns_decrypt_response(contexts, response, key, rows, query_rows, 100))
        torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    together = [heamd.pnns_generate_query(contexts, vectors, 100, key, a_seeds, error_seeds, stream=stream)[0]
                for vectors, a_seeds, error_seeds in inputs]
    together += [heamd.pnns_decrypt_response(contexts, response, key, rows, query_rows, 100, stream=stream)
                 for response in responses]
    stream.synchronize()
    for a, b in zip(apart, together):
        assert bool(a.any()) and torch.equal(a, b)


def test_workspace_is_zeroized_and_changes_nothing(oracle):
    """What the calls park in memory is the query or the distances in the clear: a caller's workspace reads zero once the call
    has drained, the bytes behind it are untouched, and the results are those of stream-ordered scratch"""
    import torch

    setups = pair_of_contexts(oracle, 64)
    contexts = [s.pnns for s in setups]
    rng = np.random.default_rng(3)
    key = secret_key_of(setups[0], rng)
    query_rows, cols, rows = 20, 4, 10
    count = pnns.plaintext_count(64, query_rows, cols, "denseRow")
    vectors = torch.from_numpy(rng.standard_normal((query_rows, cols)).astype(np.float32)).cuda()
    a_seeds, error_seeds = device_seeds(rng, 2, count), device_seeds(rng, 2, count)
    response = to_device(setups[0], uniform_words(rng, list(setups[0].q[:1]),
                                                  (2, pnns.plaintext_count(64, rows, 5, "denseColumn"), 2), 64))
    calls = [
        (heamd.pnns_generate_query_workspace_bytes(contexts, query_rows, cols),
         lambda ws: heamd.pnns_generate_query(contexts, vectors, 180, key, a_seeds, error_seeds, workspace=ws)[0]),
        (heamd.pnns_decrypt_response_workspace_bytes(contexts, rows, 5),
         lambda ws: heamd.pnns_decrypt_response(contexts, response, key, rows, 5, 180, workspace=ws)),
    ]
    for needed, call in calls:
        assert needed > 0 and needed % 16 == 0
        workspace = torch.full((needed + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        with_workspace = call(workspace)
        torch.cuda.synchronize()
        assert int(workspace[:needed].count_nonzero()) == 0
        assert bool((workspace[needed:] == 0xA5).all())
        assert torch.equal(call(None), with_workspace) and bool(with_workspace.any())
        with pytest.raises(heamd.HeError) as err:
            call(workspace[:needed - 16])
        assert err.value.name == "invalidArgument"
