"""tests/simple_pir_client_reference.py held to what can be said of it without a device, and csrc/simple_pir_client_plan.hpp held
to it from a host compiler (tests/c/simple_pir_client_plan_probe.cpp): the Array2d binomial sampler on hand-built stream bytes,
encryptZero without error against modSwitch(secret x A) on the materialised A, the plan over the shapes of
tests/test_gpu_simple_pir.py, the fold cadence of the hint product against the accumulator's capacity, the finishing kernel's
division at its decision thresholds, and the whole client against the numpy server on every case the device's end-to-end test
uses -- so that a failure there is the device's."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import encrypt_reference as E
import simple_pir_client_cases as cases
import simple_pir_client_reference as C
import simple_pir_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "swift-homomorphic-encryption_amd", "csrc")


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("std_dev,k,words,mask", [("stdDev32", 21, 2, (1 << 21) - 1), ("stdDev64", 82, 4, (1 << 18) - 1)])
def test_sampler_on_hand_built_bytes(std_dev, k, words, mask):
    assert C.binomial_layout(std_dev) == (k, words, mask)
    assert C.stream_bytes_per_coefficient(std_dev) == 8 * words
    modulus, count = 1 << 28, 3
    ones, zeros = b"\xff" * (4 * words), b"\x00" * (4 * words)
    assert C.centered_binomial((ones + ones) * count, count, std_dev, modulus) == [0] * count
    assert C.centered_binomial((ones + zeros) * count, count, std_dev, modulus) == [k] * count  # the positive half alone
    assert C.centered_binomial((zeros + ones) * count, count, std_dev, modulus) == [modulus - k] * count
    # one bit just inside and one just outside the mask of the last word of the positive half
    inside = bytearray(8 * words)
    inside[8 * (words // 2 - 1) + (k % 64 - 1) // 8] = 1 << ((k % 64 - 1) % 8)
    outside = bytearray(8 * words)
    outside[8 * (words // 2 - 1) + (k % 64) // 8] = 1 << ((k % 64) % 8)
    assert C.centered_binomial(bytes(inside) + bytes(outside), 2, std_dev, modulus) == [1, 0]


def test_sampler_stddev32_is_the_polynomial_sampler():
    stream = bytes(np.random.default_rng(5).integers(0, 256, size=16 * 40, dtype=np.uint8))
    assert C.centered_binomial(stream, 40, "stdDev32", 1 << 42) == [v % (1 << 42) for v in E.binomial_values(stream, 40)]


# ---- encryptZero -----------------------------------------------------------------------------------------------------------------------
def test_vector_schoolbook_is_the_schoolbook():
    rng = np.random.default_rng(11)
    for p in ((1 << 61) - 1, (1 << 29) + 11):
        a = rng.integers(0, p, size=32, dtype=np.uint64)
        s = rng.integers(-1, 2, size=32, dtype=np.int64)
        assert C.negacyclic_product(a, s, p) == R.negacyclic_product(a, s, p)
    worst = np.full(64, (1 << 61) - 2, dtype=np.uint64)
    assert C.negacyclic_product(worst, np.ones(64, dtype=np.int64), (1 << 61) - 1) == \
        R.negacyclic_product(worst, np.ones(64, dtype=np.int64), (1 << 61) - 1)


@pytest.mark.parametrize("name", ["three-polys-u64", "one-entry-u32"])
def test_encrypt_zero_without_error_is_the_mod_switch_of_secret_times_a(name):
    import oracle

    params = cases.params_of(oracle, name)
    _, seed, secret_seeds, error_seeds = cases.inputs_of(name, params, 1)
    polys = R.a_polynomials(oracle, params, seed)
    a_matrix = R.materialize_a(params, polys)
    secrets = C.secret_polynomials(params, secret_seeds[0], E.oracle_stream(oracle))
    assert set(np.unique(secrets)) <= {-1, 0, 1} and len(np.unique(secrets)) == 3

    def zero_error(seed, count):
        return bytes(count)

    queries = C.encrypt_zero(params, polys, secrets, error_seeds[0], "stdDev64", zero_error)
    assert np.array_equal(queries, R.mod_switch(params, R.secret_times_matrix(params, secrets, a_matrix)))
    assert np.array_equal(C.secret_times_matrix(secrets, a_matrix, params["modulus"]),
                          R.secret_times_matrix(params, secrets, a_matrix))
    # with the error: the query differs from the sample by the stream's draws, row q taking coefficients q D ...
    stream = E.oracle_stream(oracle)
    noisy = C.encrypt_zero(params, polys, secrets, error_seeds[0], "stdDev32", stream)
    count = params["chunks_per_entry"] * params["database_columns"]
    draws = E.binomial_values(stream(error_seeds[0], 16 * count), count)
    mask = (1 << params["ciphertext_bits"]) - 1
    assert [(int(a) - int(b)) & mask for a, b in zip(noisy.ravel(), queries.ravel())] == [d & mask for d in draws]


# ---- the plan header -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    binary = tmp_path_factory.mktemp("simple_pir_client_plan") / "simple_pir_client_plan_probe"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "c", "simple_pir_client_plan_probe.cpp"), "-o", str(binary)], check=True)

    def ask(*args):
        return subprocess.run([str(binary), *map(str, args)], capture_output=True, text=True, check=True).stdout.splitlines()

    return ask


def test_header_includes_nothing_of_hip():
    # (workspace_layout.hpp: plain C++ too, held to the same by tests/test_workspace_layout.py and read here as well)
    for name in ("simple_pir_client_plan.hpp", "workspace_layout.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        includes = re.findall(r'#include\s*[<"]([^>"]+)[>"]', text)
        assert includes and all(i in ("cstddef", "cstdint", "workspace_layout.hpp") for i in includes), (name, includes)


PLAN_FIELDS = ("chunk_size", "query_words", "result_words", "k", "words_per_side", "error_stream_bytes", "last_word_mask",
               "error_chunks", "secret_rows_per_pass", "fold_terms", "row_block", "hint_product_lds_bytes",
               "a_polynomials_workspace_bytes", "encrypt_zero_workspace_bytes", "secret_times_hint_workspace_bytes",
               "precompute_workspace_bytes", "decrypt_responses_workspace_bytes")


def test_host_program_agrees_with_the_python_plan(probe):
    import oracle

    count = 0
    for name, shape in cases.SHAPES.items():
        params = cases.params_of(oracle, name)
        for code, std_dev in enumerate(cases.STD_DEVS):
            for batch, forced in ((0, 0), (1, 0), (3, 0), (3, 1), (3, 2), (128, 0)):
                line = probe("plan", params["plaintext_bits"], params["ciphertext_bits"], params["lattice_dimension"], shape[5],
                             params["entry_count"], params["entry_size_in_bytes"], params["entry_size_in_scalar"],
                             params["entries_per_column"], params["chunks_per_entry"], params["database_columns"],
                             params["column_size"], params["a_poly_count"], params["modulus"], code, batch, forced)[0]
                got = dict(zip(PLAN_FIELDS, map(int, line.split())))
                expected = C.plan(params, std_dev, batch, shape[5], forced)
                k, words, mask = C.binomial_layout(std_dev)
                expected.update(k=k, words_per_side=words // 2, last_word_mask=mask,
                                error_chunks=-(-expected["query_words"] * expected["error_stream_bytes"] // 4096))
                assert got == expected, (name, std_dev, batch, forced)
                count += 1
    assert count == len(cases.SHAPES) * 2 * 6
    params = cases.params_of(oracle, "ref-small-u64")
    bad = probe("plan", 14, 42, 1024, 64, 600, 20, params["entry_size_in_scalar"], params["entries_per_column"], 1,
                params["database_columns"], params["column_size"], 1, params["modulus"], 2, 1, 0)
    assert bad == ["-"]  # an unknown standard deviation


def test_fold_cadence_against_the_accumulator(probe):
    """A lane's 64-bit word holds fold_terms terms of at most p and not one more: the reported cadence is the bound itself,
    nowhere looser.  Every term p - 1 (the worst hint word under a secret +1) or p (a zero hint word under a secret -1)."""
    import oracle

    capacity, seen = (1 << 64) - 1, 0
    for n in (64, 1024, 8192):
        for word_bits, top in ((32, 29), (64, 60)):
            for c in range(2, top + 1):
                try:
                    p = oracle.generate_primes([c + 1], True, n)[0]
                except Exception:
                    continue  # no NTT-friendly prime of c + 1 bits at this degree: he_simple_pir_shape refuses the shape
                terms = int(probe("fold", p)[0])
                assert terms == C.plan({"lattice_dimension": n, "chunks_per_entry": 1, "database_columns": 1, "a_poly_count": 1,
                                        "column_size": 1, "entry_size_in_scalar": 1, "modulus": p}, "stdDev32", 1)["fold_terms"]
                assert terms * (p - 1) < terms * p <= capacity < (terms + 1) * p, (n, c, p)
                assert terms >= 16 // (word_bits // 8) + 1, (n, c)  # a fold and the words of one 16-byte load fit
                if c <= 53:
                    assert terms >= 1023  # N = 1024: at most one fold, and none at a quarter of the columns per wavefront
                seen += 1
    assert seen > 150


def test_division_at_its_decision_thresholds(probe):
    import oracle

    for c in (28, 29, 42, 60):
        p = oracle.generate_primes([c + 1], True, 1024)[0]
        assert p.bit_length() == c + 1
        top = 1 << c
        xs, expected = [0, 1, p - 1], None
        for j in (1, 2, 3, top // 2, top // 2 + 1, top - 2, top - 1):
            x = -(-(j * p - (p >> 1)) // top)  # the least x whose quotient reaches j
            assert C.divide_and_round(x, p, c) == j and C.divide_and_round(x - 1, p, c) == j - 1, (c, j)
            xs += [x, x - 1]
        rng = np.random.default_rng(c)
        xs += [int(v) for v in rng.integers(0, p, size=64, dtype=np.uint64)]
        got = [int(line) for line in probe("divide", p, c, *xs)]
        expected = [C.divide_and_round(x, p, c) for x in xs]
        assert got == expected, c
        assert C.divide_and_round(p - 1, p, c) == top - 1  # the quotient never reaches 2^c


# ---- the whole client against the numpy server ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.END_TO_END)
def test_python_client_returns_the_entries(name):
    import oracle

    params = cases.params_of(oracle, name)
    word_bits = cases.SHAPES[name][5]
    entries, seed, secret_seeds, error_seeds = cases.inputs_of(name, params, len(cases.STD_DEVS))
    database = R.process_database(oracle, entries, params)
    polys = R.a_polynomials(oracle, params, seed)
    hint = R.hint(params, database, R.materialize_a(params, polys))
    stream = E.oracle_stream(oracle)
    for b, std_dev in enumerate(cases.STD_DEVS):
        queries, results, _ = C.precompute(params, polys, hint, secret_seeds[b], error_seeds[b], std_dev, stream)
        for index in cases.end_to_end_indices(name, params):
            responses = R.compute_response(params, database, C.add(params, queries, index), word_bits).astype(np.uint64)
            assert C.decrypt(params, responses, results, index, word_bits) == entries[index].tobytes(), (std_dev, index)
            values = C.integrate(params, responses, results, index, word_bits)
            assert bytes(oracle.coefficients_to_bytes(values, params["plaintext_bits"]))[:params["entry_size_in_bytes"]] == \
                entries[index].tobytes()


def test_python_stream_is_the_oracle_stream():
    import oracle

    seed = bytes(range(32))
    assert C.python_stream(seed, 4096 + 48) == E.oracle_stream(oracle)(seed, 4096 + 48)
