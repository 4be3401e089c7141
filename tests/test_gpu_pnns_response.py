"""The PNNS server response on the device (he_pnns_mul_transpose_device / he_pnns_compute_response_device and their UInt32
twins) against tests/pnns_reference.py's mulTranspose(vector:) restatement over the CPU oracle, plus the oracle's
modSwitchDown chain: word for word.  Word equality needs no valid encryption, so queries and Galois keys are uniform canonical
words (distinct per query); the decryption test uses real ones.

Shapes: the rows x cols grid of tests/test_gpu_pnns.py at N = 64 and 1024 (L = 3) whole; at N = 4096 and 8192 (L = 4) the
columns below N / 2 with every row count, and one N / 2-column shape each (rows = 1: the oracle is one host thread and the
matrix of a taller one is gigabytes).  L = 2 runs at N = 256.  The grid's 100 columns exceed N / 2 at N = 64: there the entry
returns the reference's invalidMatrixDimensions.  The named cases -- ragged last giant step, baby_step 1, G = 1, rows not a
multiple of N, rows > N, Q = 1, 3, 4, 5 -- are listed in CASES."""
import os
import subprocess
import sys

import numpy as np
import pytest

import heamd
import pnns_reference as pnns
from bfv_helpers import BfvClient
from test_gpu_pnns import Setup, mul_transpose_vector_device, parameters

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_setups = {}


def get_setup(oracle, degree, word32=False, two_moduli=False):
    key = (degree, word32, two_moduli)
    if key not in _setups:
        s = Setup(oracle, degree, word32)
        if two_moduli:  # L = 2: two ciphertext moduli and the key-switching one
            s.q = oracle.generate_primes([40, 40, 41], False, degree)
            s.bfv = heamd.BfvContext(degree, s.t, s.q)
            s.ref = oracle.BfvContext(degree, s.t, s.q)
            s.pnns = heamd.PnnsContext(s.bfv)
        _setups[key] = s
    return _setups[key]


def to_device(s, array):
    return heamd.to_device32(array) if s.word32 else heamd.to_device(array)


def uniform_words(rng, moduli, shape_before, degree):
    """[*shape_before][len(moduli)][N] canonical words."""
    rows = [rng.integers(0, q, size=tuple(shape_before) + (degree,), dtype=np.uint64) for q in moduli]
    return np.stack(rows, axis=len(shape_before))


def random_inputs(s, rng, rows, cols, queries):
    import torch

    L, n = s.ref.L, s.degree
    values = rng.integers(-(s.t >> 1), ((s.t - 1) >> 1) + 1, size=(rows, cols), dtype=np.int64)
    q_moduli, ks_moduli = list(s.q[:L]), list(s.q[:L]) + [s.q[-1]]
    query = uniform_words(rng, q_moduli, (queries, 2), n)
    keys = [[uniform_words(rng, ks_moduli, (L, 2), n) for _ in range(2)] for _ in range(queries)]
    return torch.from_numpy(values).cuda(), query, keys


def expected_words(s, matrix_host, rows, cols, baby_step, query, keys):
    """-> (mulTranspose [Q][C][2][L][N], response [Q][C][2][1][N]) from the restatement and the oracle's mod-switch."""
    n, L = s.degree, s.ref.L
    giant_step = pnns.baby_step_giant_step(cols, baby_step)[1]
    one = heamd.galois_element_rotating_columns(-1, n) if baby_step > 1 else None
    baby = heamd.galois_element_rotating_columns(-baby_step, n) if giant_step > 1 else None
    full, single = [], []
    for q in range(query.shape[0]):
        results = pnns.mul_transpose_vector(s.ref, matrix_host, rows, cols, baby_step, query[q],
                                            lambda ct, q=q: s.ref.apply_galois(ct, one, keys[q][0])[0],
                                            lambda ct, q=q: s.ref.apply_galois(ct, baby, keys[q][1])[0])
        results = np.stack(results)
        full.append(results)
        down = results
        for level in range(L, 1, -1):
            down = s.ref.mod_switch_down(down, 2, level)
        single.append(down)
    return np.stack(full), np.stack(single)


def device_keys(s, keys, baby_step, giant_step):
    """None where the shape does not need the key: the entry must not read it."""
    return [(to_device(s, pair[0]) if baby_step > 1 else None, to_device(s, pair[1]) if giant_step > 1 else None)
            for pair in keys]


def check(s, rows, cols, baby_step, queries, seed):
    rng = np.random.default_rng(seed)
    values, query, keys = random_inputs(s, rng, rows, cols, queries)
    if cols > s.degree // 2:
        with pytest.raises(ValueError):
            pnns.plaintext_count(s.degree, rows, cols, "diagonal")
        with pytest.raises(heamd.HeError) as err:
            s.pnns.matrix_shape(rows, cols, "diagonal", baby_step or 0)
        assert err.value.name == "invalidArgument"
        return
    resolved = baby_step or pnns.baby_step_giant_step(cols)[0]
    giant_step = pnns.baby_step_giant_step(cols, resolved)[1]
    matrix, flag = s.pnns.diagonal_matrix(values, baby_step=resolved)
    assert int(flag.item()) == 0
    device_query = to_device(s, query)
    galois = device_keys(s, keys, resolved, giant_step)
    got_full = s.to_host(s.pnns.mul_transpose(matrix, rows, cols, device_query, galois, baby_step=baby_step))
    got_single = s.to_host(s.pnns.compute_response(matrix, rows, cols, device_query, galois, baby_step=baby_step))
    full, single = expected_words(s, s.to_host(matrix), rows, cols, resolved, query, keys)
    label = (s.degree, s.word32, rows, cols, resolved, giant_step, queries)
    assert got_full.shape == full.shape and got_single.shape == single.shape, label
    assert full.any() and single.any(), label
    assert np.array_equal(got_full, full), label
    assert np.array_equal(got_single, single), label


def grid(degree):
    return [(r, c) for r in (1, degree - 1, degree, degree + 1, 3 * degree + 5) for c in (1, 2, 5, 16, 100, degree // 2)]


@pytest.mark.parametrize("degree", [64, 1024])
def test_words_over_the_grid(oracle, degree):
    s = get_setup(oracle, degree)
    for index, (rows, cols) in enumerate(grid(degree)):
        check(s, rows, cols, None, 1 + index % 2, 1000 * degree + index)


@pytest.mark.parametrize("degree", [4096, 8192])
def test_words_over_the_grid_at_four_moduli(oracle, degree):
    s = get_setup(oracle, degree)
    assert s.ref.L == 4
    for index, (rows, cols) in enumerate(grid(degree)):
        if cols == degree // 2:
            continue
        check(s, rows, cols, None, 1, 1000 * degree + index)
    check(s, 1, degree // 2, None, 1, degree)


@pytest.mark.parametrize("degree", [64, 1024, 4096])
def test_words_u32(oracle, degree):
    s = get_setup(oracle, degree, word32=True)
    for index, (rows, cols) in enumerate(grid(degree)):
        if degree >= 4096 and (cols == degree // 2 or rows not in (1, degree + 1)):
            continue
        check(s, rows, cols, None, 1 + index % 3, 77 * degree + index)
    check(s, degree + 1, 100 if degree > 64 else 30, 16 if degree > 64 else 8, 5, degree + 5)  # Q = 5: two passes


def test_u32_two_queries_share_keys_next_to_a_third(oracle):
    """Q = 3 at N = 64 on 4-byte words, queries 0 and 1 under the same device key tensors and query 2 under its own: a run of
    two equal keys next to a run of one inside each Galois batch.  1 x 3 is the smallest shape with baby_step > 1 and
    giant_step > 1 (P = 4: 2 x 2), so both the rotations by -1 and the sum's rotation by -baby_step see the runs."""
    rows, cols, queries = 1, 3, 3
    s = get_setup(oracle, 64, word32=True)
    rng = np.random.default_rng(643)
    values, query, keys = random_inputs(s, rng, rows, cols, queries)
    keys[1] = keys[0]
    baby_step, giant_step = pnns.baby_step_giant_step(cols)
    assert baby_step > 1 and giant_step > 1
    assert not np.array_equal(query[0], query[1])
    matrix, flag = s.pnns.diagonal_matrix(values)
    assert int(flag.item()) == 0
    own = device_keys(s, [keys[0], keys[2]], baby_step, giant_step)
    galois = [own[0], own[0], own[1]]
    device_query = to_device(s, query)
    got_full = s.to_host(s.pnns.mul_transpose(matrix, rows, cols, device_query, galois))
    got_single = s.to_host(s.pnns.compute_response(matrix, rows, cols, device_query, galois))
    full, single = expected_words(s, s.to_host(matrix), rows, cols, baby_step, query, keys)
    assert got_full.shape == full.shape and got_single.shape == single.shape
    assert full.any() and single.any()
    assert np.array_equal(got_full, full)
    assert np.array_equal(got_single, single)


def test_u32_words_at_four_moduli(oracle):
    """Five 27..29-bit primes at N = 64: L = 4, the smallest level at which modSwitchDownToSingle's step-by-step chain (all a
    4-byte response has) reads back from both of its scratch slabs -- at L = 3 it writes the first one only.  rows > N: C = 2."""
    degree = 64
    q = oracle.generate_primes([27, 28, 28, 29, 29], False, degree, word_bits=32)
    assert len(set(q)) == 5
    s = Setup(oracle, degree, word32=True, q=q)
    assert s.ref.L == s.bfv.L == 4
    check(s, 65, 5, None, 2, 6504)


# (degree, rows, cols, baby_step, queries)
CASES = [
    (256, 300, 100, 12, 1),      # L = 2 below; P = 128, G = 11, the last giant step sums 8: ragged
    (1024, 1500, 100, 12, 3),    # ragged, rows > N and not a multiple of N, three queries in one pass
    (1024, 2049, 5, 8, 4),       # G = 1 (baby_step = P): no sum, the key of -baby_step is not read; C = 3; four queries
    (1024, 700, 1, 1, 5),        # baby_step = 1 and G = 1: no rotation at all, no key read; five queries: two passes
    (1024, 1024, 100, 128, 5),   # G = 1 with a baby step whose rotated rows exceed LDS: the general form of the kernel
    (64, 150, 7, 4, 5),          # N = 64: below one wavefront of 16-byte lanes; five queries
    (64, 64, 2, 2, 3),           # baby_step 2, G = 1
    (4096, 4097, 100, 16, 4),    # L = 4, P = 128, G = 8, C = 2, four queries in one pass
    (8192, 8193, 100, 12, 5),    # the benched packing (b = 12, G = 11, ragged) at C = 2, five queries
    (8192, 3 * 8192 + 5, 16, 4, 3),
]


@pytest.mark.parametrize("degree,rows,cols,baby_step,queries", CASES)
def test_words_of_the_named_cases(oracle, degree, rows, cols, baby_step, queries):
    for two_moduli in ((False, True) if degree == 256 else (False,)):
        s = get_setup(oracle, degree, two_moduli=two_moduli)
        assert s.ref.L == (2 if two_moduli else 4 if degree >= 4096 else 3)
        check(s, rows, cols, baby_step, queries, degree + rows)


def test_baby_step_one_with_a_sum(oracle):
    """cols = 1 is the only shape with baby_step = 1 the reference admits (babyStep >= giantStep); it has G = 1.  baby_step
    = 1 therefore never meets a sum, and G > 1 always meets rotations by -1: both keys, one key and no key are the cases."""
    with pytest.raises(ValueError):
        pnns.baby_step_giant_step(2, 1)
    s = get_setup(oracle, 64)
    with pytest.raises(heamd.HeError) as err:
        s.pnns.matrix_shape(10, 2, "diagonal", 1)
    assert err.value.name == "invalidArgument"


def test_missing_keys_on_the_device(oracle):
    s = get_setup(oracle, 64)
    rng = np.random.default_rng(3)
    values, query, keys = random_inputs(s, rng, 50, 16, 2)
    matrix, _ = s.pnns.diagonal_matrix(values)
    device_query = to_device(s, query)
    full = device_keys(s, keys, 4, 4)
    for broken in ([(None, full[0][1]), full[1]], [full[0], (full[1][0], None)], None):
        with pytest.raises(heamd.HeError) as err:
            s.pnns.mul_transpose(matrix, 50, 16, device_query, broken)
        assert err.value.name == "missingGaloisKey", broken
    with pytest.raises(heamd.HeError) as err:  # the query's column count does not match the matrix
        s.pnns.mul_transpose(matrix, 50, 32, device_query, full)
    assert err.value.name == "invalidArgument"


# ---- decryption -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(50, 16), (150, 7), (64, 30)])
def test_decrypted_response_is_the_matrix_vector_product(oracle, rows, cols):
    import torch

    s = get_setup(oracle, 64)
    degree, t = 64, s.t
    rng = np.random.default_rng(rows)
    bound = 40
    data = rng.integers(-bound, bound + 1, size=(rows, cols))
    baby_step, giant_step = pnns.baby_step_giant_step(cols)
    matrix, flag = s.pnns.diagonal_matrix(torch.from_numpy(data.astype(np.int64)).cuda())
    assert int(flag.item()) == 0
    clients = [BfvClient(oracle, s.ref, seed=rows + k) for k in range(2)]  # two clients: own secret keys, own Galois keys
    vectors = [rng.integers(-bound, bound + 1, size=cols) for _ in clients]
    queries, keys = [], []
    for client, vector in zip(clients, vectors):
        slots = pnns.dense_row_vector_slots(np.mod(vector, t), degree)
        queries.append(client.encrypt([int(v) for v in s.encoder.encode(slots)[0]]))
        keys.append((heamd.to_device(client.galois_key(heamd.galois_element_rotating_columns(-1, degree))),
                     heamd.to_device(client.galois_key(heamd.galois_element_rotating_columns(-baby_step, degree)))
                     if giant_step > 1 else None))
    device_query = heamd.to_device(np.stack(queries))
    full = heamd.to_host(s.pnns.mul_transpose(matrix, rows, cols, device_query, keys))
    single = heamd.to_host(s.pnns.compute_response(matrix, rows, cols, device_query, keys))
    for k, (client, vector) in enumerate(zip(clients, vectors)):
        product = np.mod(data @ vector, t).astype(np.uint64)
        for result, moduli_count in ((full[k], None), (single[k], 1)):
            decoded = np.concatenate([s.encoder.decode(np.array(client.decrypt(ct, moduli_count), dtype=np.uint64))[0]
                                      for ct in result])
            assert decoded.shape[0] >= rows
            assert np.array_equal(decoded[:rows], product), (k, moduli_count)  # every row


# ---- composition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree,rows,cols", [(64, 150, 7), (1024, 1500, 100)])
def test_entry_equals_the_composition_of_existing_entry_points(oracle, degree, rows, cols):
    s = get_setup(oracle, degree)
    rng = np.random.default_rng(degree)
    queries = 3
    values, query, keys = random_inputs(s, rng, rows, cols, queries)
    baby_step, giant_step = pnns.baby_step_giant_step(cols)
    assert giant_step > 1
    matrix, _ = s.pnns.diagonal_matrix(values)
    galois = device_keys(s, keys, baby_step, giant_step)
    device_query = to_device(s, query)
    got = s.pnns.mul_transpose(matrix, rows, cols, device_query, galois)
    response = s.pnns.compute_response(matrix, rows, cols, device_query, galois)
    for q in range(queries):
        composed = mul_transpose_vector_device(s, matrix, rows, cols, baby_step, device_query[q], galois[q][0], galois[q][1])
        assert len(composed) == got.shape[1]
        for c, ct in enumerate(composed):
            assert np.array_equal(heamd.to_host(ct), heamd.to_host(got[q, c])), (q, c)
            down = s.bfv.mod_switch_down_to_single(ct.reshape(1, 2, s.bfv.L, degree), 2)
            assert np.array_equal(heamd.to_host(down).reshape(2, 1, degree), heamd.to_host(response[q, c])), (q, c)


def compose_u32(s, matrix, rows, cols, baby_step, query, key_one, key_baby):
    """mul_transpose_vector_device of tests/test_gpu_pnns.py on packed 4-byte words: the same sequence through the _u32 entry
    points (that helper's transforms and additions are the 8-byte ones) -> (result ciphertexts, their mod-switch to q_0)."""
    import torch

    bfv, degree, L = s.bfv, s.degree, s.bfv.L
    ring = bfv.ciphertext_context()
    dimension = pnns.next_power_of_two(cols)
    giant_step = -(-dimension // baby_step)
    element_one = heamd.galois_element_rotating_columns(-1, degree)
    element_baby = heamd.galois_element_rotating_columns(-baby_step, degree)
    states, state = [], query.reshape(1, 2, L, degree)
    for step in range(baby_step):
        states.append(state)
        if step != baby_step - 1:
            state = bfv.apply_galois(state, element_one, key_one)
    rotated = ring.forward_ntt_u32_(torch.cat(states).contiguous())
    result_count = -(-rows // degree)
    results, singles = [], []
    for result_index in range(result_count):
        products = []
        for giant in range(giant_step):
            count = min(baby_step, dimension - baby_step * giant)
            indices = [result_count * (j + baby_step * giant) + result_index for j in range(count)]
            product = bfv.inner_product_plain_resident(rotated[:count].contiguous(), matrix[indices].contiguous())
            products.append(ring.inverse_ntt_u32_(product.reshape(2, L, degree)))
        accumulator = products.pop()
        for product in reversed(products):
            accumulator = bfv.apply_galois(accumulator.reshape(1, 2, L, degree), element_baby, key_baby).reshape(2, L, degree)
            accumulator = ring.elementwise_u32_("add", accumulator, product)
        results.append(accumulator)
        down = accumulator.reshape(1, 2, L, degree)
        for level in range(L, 1, -1):
            down = bfv.mod_switch_down(down, 2, moduli_count=level)
        singles.append(down.reshape(2, 1, degree))
    return results, singles


def test_u32_entry_equals_the_composition_of_existing_entry_points(oracle):
    degree, rows, cols, queries = 1024, 1500, 100, 3
    s = get_setup(oracle, degree, word32=True)
    rng = np.random.default_rng(32)
    values, query, keys = random_inputs(s, rng, rows, cols, queries)
    baby_step, giant_step = pnns.baby_step_giant_step(cols)
    assert giant_step > 1
    matrix, _ = s.pnns.diagonal_matrix(values)
    galois = device_keys(s, keys, baby_step, giant_step)
    device_query = to_device(s, query)
    got = s.pnns.mul_transpose(matrix, rows, cols, device_query, galois)
    response = s.pnns.compute_response(matrix, rows, cols, device_query, galois)
    for q in range(queries):
        composed, singles = compose_u32(s, matrix, rows, cols, baby_step, device_query[q], galois[q][0], galois[q][1])
        assert len(composed) == got.shape[1] == 2
        for c in range(len(composed)):
            assert np.array_equal(heamd.to_host32(composed[c]), heamd.to_host32(got[q, c])), (q, c)
            assert np.array_equal(heamd.to_host32(singles[c]), heamd.to_host32(response[q, c])), (q, c)


# ---- groups and stream order ------------------------------------------------------------------------------------------------------
_GROUP_SCRIPT = r"""
import sys
import numpy as np, torch
sys.path[:0] = [{root!r}, {pkg!r}]
import heamd
degree, t, q = {degree}, {t}, {q}
bfv = heamd.BfvContext(degree, t, q)
ctx = heamd.PnnsContext(bfv)
rng = np.random.default_rng(11)
L = bfv.L
def words(moduli, before):
    return np.stack([rng.integers(0, m, size=before + (degree,), dtype=np.uint64) for m in moduli], axis=len(before))
out = {{}}
for rows, cols, queries in ((3 * degree + 5, 100, 3), (5 * degree, 5, 5)):
    values = rng.integers(-(t >> 1), ((t - 1) >> 1) + 1, size=(rows, cols), dtype=np.int64)
    matrix, _ = ctx.diagonal_matrix(torch.from_numpy(values).cuda())
    query = heamd.to_device(words(q[:L], (queries, 2)))
    keys = [tuple(heamd.to_device(words(q[:L] + q[-1:], (L, 2))) for _ in range(2)) for _ in range(queries)]
    out["full%d" % rows] = ctx.mul_transpose(matrix, rows, cols, query, keys).cpu().numpy()
    out["single%d" % rows] = ctx.compute_response(matrix, rows, cols, query, keys).cpu().numpy()
np.savez(sys.argv[1], **out)
"""


def test_result_groups_give_identical_words(oracle, tmp_path):
    """HEAMD_PNNS_RESPONSE_GROUP = 1, 2, 3 result ciphertexts per group (C = 4 and 5: whole and ragged groups) give the words
    of one group (a fresh process each: the override is read from the environment)."""
    degree = 256
    t, q = parameters(oracle, degree)
    script = tmp_path / "groups.py"
    script.write_text(_GROUP_SCRIPT.format(root=ROOT, pkg=os.path.join(ROOT, "swift-homomorphic-encryption_amd"),
                                           degree=degree, t=t, q=list(q)))
    results = []
    for group in (None, "1", "2", "3"):
        env = dict(os.environ)
        env.pop("HEAMD_PNNS_RESPONSE_GROUP", None)
        if group:
            env["HEAMD_PNNS_RESPONSE_GROUP"] = group
        path = tmp_path / f"out_{group}.npz"
        subprocess.run([sys.executable, str(script), str(path)], check=True, env=env, timeout=300)
        results.append(np.load(path))
    assert len(results[0].files) == 4
    for name in results[0].files:
        assert results[0][name].any()
        for other in results[1:]:
            assert np.array_equal(results[0][name], other[name]), name


def test_back_to_back_calls_on_one_stream(oracle):
    """Two calls enqueued on one stream with no host synchronisation between them (they share the stream-ordered scratch)
    give the words of the same calls each followed by a synchronisation."""
    import torch

    s = get_setup(oracle, 4096)
    rng = np.random.default_rng(8)
    rows, cols, queries = 4097, 100, 2
    values, query_a, keys_a = random_inputs(s, rng, rows, cols, queries)
    _, query_b, keys_b = random_inputs(s, rng, rows, cols, queries)
    baby_step, giant_step = pnns.baby_step_giant_step(cols)
    matrix, _ = s.pnns.diagonal_matrix(values)
    inputs = [(to_device(s, query), device_keys(s, keys, baby_step, giant_step))
              for query, keys in ((query_a, keys_a), (query_b, keys_b))]
    torch.cuda.synchronize()
    apart = []
    for query, galois in inputs:
        apart.append(heamd.to_host(s.pnns.compute_response(matrix, rows, cols, query, galois)))
        torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    together = [s.pnns.compute_response(matrix, rows, cols, query, galois, stream=stream) for query, galois in inputs]
    stream.synchronize()
    for a, b in zip(apart, together):
        assert a.any() and np.array_equal(a, heamd.to_host(b))
    assert not np.array_equal(apart[0], apart[1])
