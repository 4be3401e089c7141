"""The PNNS server database on the device (he_pnns_*) against tests/pnns_reference.py, word for word: quantize_rows against
normalizedScaledAndRounded, diagonal_matrix against plaintext_to_eval(encodeSimd(diagonalPlaintexts)), group splitting, the
out-of-range word, stream order, and mulTranspose(vector:) composed here from the library's entry points, decrypted and
compared with the integer matrix-vector product.

Every N runs the whole rows x cols grid with the default baby step, reduce off and moduli_count L; the other baby steps,
reduce on and moduli_count 1 run over the whole grid at N = 64 and 1024 and, at N = 4096 and 8192, over the grid's shapes
below N / 2 columns plus one N / 2-column shape each (a full cross product there is hundreds of GiB of expected words).  The
grid's 100 columns exceed the SIMD column count at N = 64: there the case is the reference's invalidMatrixDimensions."""
import os
import subprocess
import sys

import numpy as np
import pytest

import heamd
import pnns_reference as pnns
from bfv_helpers import BfvClient
from conftest import host_threads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parameters(oracle, degree, word32=False):
    if word32:
        t = oracle.generate_primes([17], True, degree)[0]
        q = oracle.generate_primes([27, 28, 28, 29], False, degree, word_bits=32)
        return t, q
    if degree >= 4096:
        return oracle.generate_primes([20], False, degree)[0], oracle.generate_primes([55] * 5, False, degree)
    return oracle.generate_primes([17], True, degree)[0], oracle.generate_primes([40, 40, 40, 41], False, degree)


class Setup:
    def __init__(self, oracle, degree, word32=False, t=None, q=None):
        """t / q: a plaintext modulus / coefficient moduli other than parameters()'."""
        self.degree, self.word32 = degree, word32
        self.t, self.q = parameters(oracle, degree, word32)
        if t is not None:
            self.t = t
        if q is not None:
            self.q = list(q)
        if word32:
            self.bfv = heamd.BfvContext32(degree, self.t, self.q)
            self.ref = oracle.BfvContext(degree, self.t, self.q, word_bits=32)
        else:
            self.bfv = heamd.BfvContext(degree, self.t, self.q)
            self.ref = oracle.BfvContext(degree, self.t, self.q)
        self.pnns = heamd.PnnsContext(self.bfv)
        self.encoder = pnns.SimdEncoder(oracle, degree, self.t, threads=host_threads())

    def to_host(self, matrix):
        return heamd.to_host32(matrix) if self.word32 else heamd.to_host(matrix)


_setups = {}


@pytest.fixture
def setup(oracle):
    def get(degree, word32=False):
        key = (degree, word32)
        if key not in _setups:
            _setups[key] = Setup(oracle, degree, word32)
        return _setups[key]

    return get


def signed_values(rng, rows, cols, t, reduce):
    if reduce:  # anything far outside the centred range, and the multiples of t
        values = rng.integers(-(1 << 62), 1 << 62, size=(rows, cols), dtype=np.int64)
        edge = [t, -t, -1, 0]
    else:
        values = rng.integers(-(t >> 1), ((t - 1) >> 1) + 1, size=(rows, cols), dtype=np.int64)
        edge = [-(t >> 1), (t - 1) >> 1, 0, -1]
    flat = values.reshape(-1)
    flat[:min(4, flat.size)] = edge[:min(4, flat.size)]
    return values


def check_matrix(s, rng, rows, cols, baby_step, reduce, moduli_count):
    import torch

    values = signed_values(rng, rows, cols, s.t, reduce)
    if cols > s.degree // 2:  # N = 64 with 100 columns: the reference throws invalidMatrixDimensions, and so do both sides here
        with pytest.raises(ValueError):
            pnns.plaintext_count(s.degree, rows, cols, "diagonal")
        with pytest.raises(heamd.HeError) as err:
            s.pnns.diagonal_matrix(torch.from_numpy(values).cuda(), baby_step=baby_step or 0, reduce=reduce,
                                   moduli_count=moduli_count)
        assert err.value.name == "invalidArgument"
        return
    matrix, flag = s.pnns.diagonal_matrix(torch.from_numpy(values).cuda(), baby_step=baby_step or 0, reduce=reduce,
                                          moduli_count=moduli_count)
    resolved = baby_step or pnns.baby_step_giant_step(cols)[0]
    expected, outside = pnns.diagonal_matrix(s.ref, s.encoder, values.reshape(-1), rows, cols, resolved, reduce, moduli_count)
    assert not outside and int(flag.item()) == 0
    got = s.to_host(matrix)
    assert got.shape == expected.shape == (pnns.plaintext_count(s.degree, rows, cols, "diagonal"),
                                           moduli_count or s.ref.L, s.degree)
    assert np.array_equal(got, expected), (s.degree, rows, cols, baby_step, reduce, moduli_count)


def grid(degree):
    return [(r, c) for r in (1, degree - 1, degree, degree + 1, 3 * degree + 5) for c in (1, 2, 5, 16, 100, degree // 2)]


def baby_steps(cols):
    """default, P (one giant step) and one other admissible divisor of P (None where P has none: P <= 2)."""
    padded = pnns.next_power_of_two(cols)
    default = pnns.baby_step_giant_step(cols)[0]
    others = [d for d in (padded // 2, padded // 4, 2 * default) if d not in (default, padded) and d >= 1 and
              padded % d == 0 and d * d >= padded]
    return [None, padded] + others[:1]


# ---- quantize_rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [1, 3, 128, 384])
def test_quantize_rows_matches_the_restatement(setup, cols):
    import torch

    s = setup(64)
    rng = np.random.default_rng(cols)
    rows = 4000
    vectors = rng.standard_normal((rows, cols)).astype(np.float32)
    vectors[5] = 0                       # a zero norm
    vectors[6] = -0.0
    vectors[7] = 1e-30                   # squares underflow to zero: norm 0 with non-zero entries
    vectors[8] = 1e-20                   # subnormal squares
    vectors[9] = 1e-3                    # one huge and many tiny entries
    vectors[9, 0] = 3e18
    vectors[10] = rng.standard_normal(cols).astype(np.float32) * np.float32(1e-12)
    vectors[10, -1] = -7e15
    vectors[11:400] *= np.float32(1e4)   # large quotients
    for scale in (1.0, 100.0, 4095.0, -77.5):
        got = s.pnns.quantize_rows(torch.from_numpy(vectors).cuda(), scale).cpu().numpy()
        assert np.array_equal(got, pnns.normalized_scaled_and_rounded(vectors, scale)), (cols, scale)


def test_quantize_rows_exact_ties(setup):
    import torch

    s = setup(64)
    # rows (3 k, 4 k) have norm exactly 5 k: scaling by 2.5 gives 1.5 and 2, by 7.5 gives 4.5 and 6, ... -- halves in both signs
    k = np.arange(1, 2049, dtype=np.float32)
    vectors = np.stack([3 * k, -4 * k], axis=1).astype(np.float32)
    for scale in (2.5, 7.5, -2.5, 12.5, 0.8333333):
        got = s.pnns.quantize_rows(torch.from_numpy(vectors).cuda(), scale).cpu().numpy()
        expected = pnns.normalized_scaled_and_rounded(vectors, scale)
        assert np.array_equal(got, expected), scale
    assert pnns.normalized_scaled_and_rounded(vectors, 2.5)[0].tolist() == [2, -2]
    assert pnns.normalized_scaled_and_rounded(vectors, 7.5)[0].tolist() == [5, -6]
    # one-element rows: v / |v| = +-1, so scaling factors k + 0.5 are ties
    ones = np.array([[1.0], [-1.0], [3.0], [-0.125]], dtype=np.float32)
    for scale in (0.5, 1.5, 2.5, 1000.5):
        got = s.pnns.quantize_rows(torch.from_numpy(ones).cuda(), scale).cpu().numpy()
        assert np.array_equal(got, pnns.normalized_scaled_and_rounded(ones, scale)), scale


def test_quantize_rows_hundred_thousand_rows(setup):
    import torch

    s = setup(64)
    rng = np.random.default_rng(100000)
    vectors = rng.standard_normal((100000, 128)).astype(np.float32)
    got = s.pnns.quantize_rows(torch.from_numpy(vectors).cuda(), 4096.0).cpu().numpy()
    assert np.array_equal(got, pnns.normalized_scaled_and_rounded(vectors, 4096.0))


# ---- diagonal_matrix ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [64, 1024, 4096, 8192])
def test_diagonal_matrix_over_the_grid(setup, degree):
    s = setup(degree)
    rng = np.random.default_rng(degree)
    for rows, cols in grid(degree):
        check_matrix(s, rng, rows, cols, None, False, None)


@pytest.mark.parametrize("degree", [64, 1024, 4096, 8192])
def test_diagonal_matrix_baby_steps_reduce_and_moduli_counts(setup, degree):
    s = setup(degree)
    rng = np.random.default_rng(degree + 1)
    wide = 0
    for rows, cols in grid(degree):
        if degree >= 4096 and cols == degree // 2:
            wide += 1
            if wide != 3:  # rows = N: one N / 2-column shape runs every variant
                continue
        for baby_step in baby_steps(cols):
            for reduce in (False, True):
                for moduli_count in (1, None):
                    if baby_step is None and not reduce and moduli_count is None:
                        continue  # test_diagonal_matrix_over_the_grid
                    check_matrix(s, rng, rows, cols, baby_step, reduce, moduli_count)


@pytest.mark.parametrize("degree", [64, 1024, 4096])
def test_diagonal_matrix_u32(setup, degree):
    s = setup(degree, word32=True)
    rng = np.random.default_rng(degree + 2)
    for rows, cols in grid(degree):
        if degree >= 4096 and cols == degree // 2 and rows != degree + 1:
            continue
        variants = [(None, False, None), (pnns.next_power_of_two(cols), True, 1)]
        for baby_step, reduce, moduli_count in variants:
            check_matrix(s, rng, rows, cols, baby_step, reduce, moduli_count)


def test_process_database_at_the_bench_shape(setup):
    """2^20 rows x 128 columns at N = 8192, L = 4: every word of the 4 GiB matrix, compared in blocks of diagonals."""
    import torch

    s = setup(8192)
    rows, cols, scale = 1 << 20, 128, float((s.t - 1) >> 1) - 1.0
    rng = np.random.default_rng(20)
    vectors = rng.standard_normal((rows, cols), dtype=np.float32)
    device_vectors = torch.from_numpy(vectors).cuda()
    matrix, flag = s.pnns.process_database(device_vectors, scale)
    rounded = pnns.normalized_scaled_and_rounded(vectors, scale)
    assert np.array_equal(s.pnns.quantize_rows(device_vectors, scale).cpu().numpy(), rounded)
    assert int(flag.item()) == 0
    baby_step = pnns.baby_step_giant_step(cols)[0]
    per_column = rows // 8192
    assert matrix.shape == (128 * per_column, 4, 8192)
    block = 16
    for first in range(0, 128, block):
        expected, outside = pnns.diagonal_matrix(s.ref, s.encoder, rounded, rows, cols, baby_step, False,
                                                 first_diagonal=first, diagonal_count=block)
        assert not outside
        got = heamd.to_host(matrix[first * per_column:(first + block) * per_column])
        assert np.array_equal(got, expected), first


_GROUP_SCRIPT = r"""
import sys
import numpy as np, torch
sys.path[:0] = [{root!r}, {pkg!r}]
import heamd
degree, t, q = {degree}, {t}, {q}
ctx = heamd.PnnsContext(heamd.BfvContext(degree, t, q))
rng = np.random.default_rng(9)
out = {{}}
for rows, cols, baby in ((3 * degree + 5, 5, 0), (degree + 1, 16, 8), (7, 100, 0)):
    values = rng.integers(-(t >> 1), ((t - 1) >> 1) + 1, size=(rows, cols), dtype=np.int64)
    matrix, flag = ctx.diagonal_matrix(torch.from_numpy(values).cuda(), baby_step=baby)
    out["m%d_%d" % (rows, cols)] = matrix.cpu().numpy()
    assert int(flag.item()) == 0
np.savez(sys.argv[1], **out)
"""


def test_group_splitting_gives_identical_output(oracle, tmp_path):
    """HEAMD_PNNS_PROCESS_GROUP=3: groups that end inside a diagonal, inside a run of diagonals and across giant steps give
    the words of one group (a fresh process each: the override is read from the environment)."""
    degree = 256
    t, q = parameters(oracle, degree)
    script = tmp_path / "group.py"
    script.write_text(_GROUP_SCRIPT.format(root=ROOT, pkg=os.path.join(ROOT, "swift-homomorphic-encryption_amd"),
                                           degree=degree, t=t, q=q))
    results = []
    for group in (None, "3", "7"):
        env = dict(os.environ)
        env.pop("HEAMD_PNNS_PROCESS_GROUP", None)
        if group:
            env["HEAMD_PNNS_PROCESS_GROUP"] = group
        path = tmp_path / f"out_{group}.npz"
        subprocess.run([sys.executable, str(script), str(path)], check=True, env=env, timeout=300)
        results.append(np.load(path))
    assert len(results[0].files) == 3
    for name in results[0].files:
        assert results[0][name].any()
        for other in results[1:]:
            assert np.array_equal(results[0][name], other[name]), name


def test_out_of_range_word(setup):
    import torch

    for word32 in (False, True):
        s = setup(1024, word32)
        t = s.t
        rng = np.random.default_rng(4)
        values = signed_values(rng, 1500, 100, t, False)
        _, flag = s.pnns.diagonal_matrix(torch.from_numpy(values).cuda())
        assert int(flag.item()) == 0
        for bad, where in (((t - 1) // 2 + 1, (1499, 99)), (-(t >> 1) - 1, (0, 0)), (t, (700, 50))):
            spoiled = values.copy()
            spoiled[where] = bad
            assert pnns.centered_to_remainder(spoiled, t)[1]
            _, flag = s.pnns.diagonal_matrix(torch.from_numpy(spoiled).cuda())
            assert int(flag.item()) == 1, (bad, where)
            # with reduce the same values are in range by definition, and the word is left alone
            matrix, flag = s.pnns.diagonal_matrix(torch.from_numpy(spoiled).cuda(), reduce=True, moduli_count=1)
            assert int(flag.item()) == 0
            expected, _ = pnns.diagonal_matrix(s.ref, s.encoder, spoiled.reshape(-1), 1500, 100,
                                               pnns.baby_step_giant_step(100)[0], True, 1)
            assert np.array_equal(s.to_host(matrix), expected)
        # NULL is accepted
        entry = "he_pnns_diagonal_matrix_device_u32" if word32 else "he_pnns_diagonal_matrix_device"
        device_values = torch.from_numpy(values).cuda()
        matrix = torch.empty((128 * 2, 1, 1024), dtype=torch.int32 if word32 else torch.int64, device="cuda")
        status = getattr(heamd.load_library(), entry)(s.pnns.h, device_values.data_ptr(), 1500, 100, 0, 0, 1,
                                                      matrix.data_ptr(), None, None)
        assert status == 0
        torch.cuda.synchronize()


def test_argument_errors_on_the_device(setup):
    import torch

    s = setup(64)
    values = torch.zeros((10, 5), dtype=torch.int64, device="cuda")
    for kwargs in ({"baby_step": 2}, {"moduli_count": 0}, {"moduli_count": s.ref.L + 1}):
        with pytest.raises(heamd.HeError) as err:
            s.pnns.diagonal_matrix(values, **kwargs)
        assert err.value.name == "invalidArgument", kwargs
    with pytest.raises(heamd.HeError) as err:
        s.pnns.diagonal_matrix(torch.zeros((10, 33), dtype=torch.int64, device="cuda"))
    assert err.value.name == "invalidArgument"


def test_result_of_a_side_stream_is_consumed_after_an_event_wait(setup):
    import torch

    s = setup(4096)
    rows, cols = 3 * 4096 + 5, 100
    rng = np.random.default_rng(6)
    vectors = rng.standard_normal((rows, cols)).astype(np.float32)
    device_vectors = torch.from_numpy(vectors).cuda()
    scale = 500.0
    load = torch.randn(8192, 8192, device="cuda")
    load @ load  # library start-up outside the ordered part
    torch.cuda.synchronize()
    first, second = torch.cuda.Stream(), torch.cuda.Stream()
    done = torch.cuda.Event()
    with torch.cuda.stream(first):
        for _ in range(20):
            load @ load
    matrix, flag = s.pnns.process_database(device_vectors, scale, stream=first)
    done.record(first)
    pending = not done.query()
    second.wait_event(done)
    with torch.cuda.stream(second):
        copy = matrix.clone()
        coeff = s.bfv.plaintext_to_coeff(matrix[:8], stream=second)
    second.synchronize()
    assert pending, "process_database did not return before its stream had drained: not enqueue-only"
    rounded = pnns.normalized_scaled_and_rounded(vectors, scale)
    baby_step = pnns.baby_step_giant_step(cols)[0]
    expected, _ = pnns.diagonal_matrix(s.ref, s.encoder, rounded, rows, cols, baby_step, False)
    assert np.array_equal(heamd.to_host(copy), expected) and int(flag.item()) == 0
    assert np.array_equal(heamd.to_host(coeff), s.ref.plaintext_to_coeff(expected[:8]))
    torch.cuda.synchronize()


# ---- end to end: mulTranspose(vector:) from the library's entry points ----------------------------------------------------------
def mul_transpose_vector_device(s, matrix, rows, cols, baby_step, query, key_one, key_baby):
    """MatrixMultiplication.swift:131-226 with heamd: rotate (apply_galois), forward NTT, inner_product_plain_resident over
    the device-built matrix, inverse NTT, rotate-and-sum.  query [2][L][N] Coeff on the device -> result ciphertexts."""
    import torch

    bfv, degree = s.bfv, s.degree
    ring = bfv.ciphertext_context()
    dimension = pnns.next_power_of_two(cols)
    giant_step = -(-dimension // baby_step)
    element_one = heamd.galois_element_rotating_columns(-1, degree)
    states, state = [], query.reshape(1, 2, bfv.L, degree)
    for step in range(baby_step):
        states.append(state)
        if step != baby_step - 1:
            state = bfv.apply_galois(state, element_one, key_one)
    rotated = ring.forward_ntt_(torch.cat(states).contiguous())
    result_count = -(-rows // degree)
    results = []
    for result_index in range(result_count):
        products = []
        for giant in range(giant_step):
            count = min(baby_step, dimension - baby_step * giant)
            indices = [result_count * (j + baby_step * giant) + result_index for j in range(count)]
            plaintexts = matrix[indices].contiguous()
            product = bfv.inner_product_plain_resident(rotated[:count].contiguous(), plaintexts)
            products.append(ring.inverse_ntt_(product))
        accumulator = products.pop()
        for product in reversed(products):
            accumulator = bfv.apply_galois(accumulator, heamd.galois_element_rotating_columns(-baby_step, degree), key_baby)
            accumulator = ring.add_(accumulator.reshape(2, bfv.L, degree), product.reshape(2, bfv.L, degree))
        results.append(accumulator.reshape(2, bfv.L, degree))
    return results


@pytest.mark.parametrize("rows,cols", [(50, 16), (150, 7)])  # one result ciphertext; rows > N: three
def test_mul_transpose_end_to_end(oracle, setup, rows, cols):
    import torch

    s = setup(64)
    degree, t = 64, s.t
    client = BfvClient(oracle, s.ref, seed=rows)
    rng = np.random.default_rng(rows)
    bound = 40
    data = rng.integers(-bound, bound + 1, size=(rows, cols))
    vector = rng.integers(-bound, bound + 1, size=cols)
    baby_step, giant_step = pnns.baby_step_giant_step(cols)
    assert giant_step > 1
    matrix, flag = s.pnns.diagonal_matrix(torch.from_numpy(data.astype(np.int64)).cuda())
    assert int(flag.item()) == 0
    query_slots = pnns.dense_row_vector_slots(np.mod(vector, t), degree)
    query = client.encrypt([int(v) for v in s.encoder.encode(query_slots)[0]])
    key_one = heamd.to_device(client.galois_key(heamd.galois_element_rotating_columns(-1, degree)))
    key_baby = heamd.to_device(client.galois_key(heamd.galois_element_rotating_columns(-baby_step, degree)))
    results = mul_transpose_vector_device(s, matrix, rows, cols, baby_step, heamd.to_device(query), key_one, key_baby)
    assert len(results) == -(-rows // degree)
    decoded = np.concatenate([s.encoder.decode(np.array(client.decrypt(heamd.to_host(ct)), dtype=np.uint64))[0]
                              for ct in results])
    assert np.array_equal(decoded[:rows], np.mod(data @ vector, t).astype(np.uint64))
