"""tests/simple_pir_reference.py held to the reference's own acceptance tests before anything is compared with it
(Tests/PrivateInformationRetrievalTests/SimplePirTests.swift): the four encrypt / decrypt round trips (:23-46) with the
restated server AND the restated client, and noiselessSample == secret x A for the four computingParams cases (:164-222)."""
import numpy as np
import pytest

import simple_pir_reference as R


@pytest.mark.parametrize("entry_count,entry_size", [(600, 20), (20, 600)])
@pytest.mark.parametrize("pbits,cbits,word_bits", [(7, 28, 32), (14, 42, 64)])
def test_round_trip(oracle, entry_count, entry_size, pbits, cbits, word_bits):
    """runEncryptDecryptRoundTripTest (_TestUtilities/PirUtilities/SimplePirTests.swift:70-108)."""
    rng = np.random.default_rng(entry_count + pbits)
    raw = R.make_database(entry_count, entry_size)
    params = R.shape(oracle, pbits, cbits, 1024, entry_count, entry_size, word_bits)
    database = R.process_database(oracle, raw, params)
    assert database.shape == (params["column_size"], params["database_columns"])
    assert int(database.max()) < (1 << pbits)
    seed = bytes(rng.integers(0, 256, size=32, dtype=np.uint8))
    a_matrix = R.materialize_a(params, R.a_polynomials(oracle, params, seed))
    assert a_matrix.shape == (params["database_columns"], 1024)
    hint = R.hint(params, database, a_matrix)
    client = R.Client(oracle, params, hint, a_matrix, rng)
    for _ in range(5):
        index = int(rng.integers(0, entry_count))
        responses = R.compute_response(params, database, client.query(index), word_bits)
        assert responses.shape == (params["chunks_per_entry"], params["column_size"])
        assert client.decrypt(responses, index) == raw[index].tobytes()


def test_a_polynomials_are_the_seeded_stream(oracle):
    """One polynomial over one modulus is PolyRq.random(context:using: NistAes128Ctr(seed:)), which the oracle pins."""
    params = R.shape(oracle, 7, 28, 1024, 600, 20, 32)
    seed = bytes(range(32))
    ours = R.a_polynomials(oracle, params, seed)
    ring = oracle.PolyContext(1024, [params["modulus"]])
    assert np.array_equal(ours, ring.random_from_seeds(np.frombuffer(seed, dtype=np.uint8))[0])


@pytest.mark.parametrize("pbits,cbits,n,entry_count,entry_size,chunks_above_one,polys_above_one", [
    (8, 9, 16, 1, 1, False, False),   # singleBoth
    (8, 9, 8, 10, 1, False, True),    # multipleAPolynomials
    (4, 8, 8, 1, 1, True, False),     # multipleSecretKeys
    (4, 8, 8, 10, 62, True, True),    # multipleBoth
])
def test_noiseless_sample(oracle, pbits, cbits, n, entry_count, entry_size, chunks_above_one, polys_above_one):
    """noiselessSampleHelper (SimplePirTests.swift:147-162): the polynomial route equals secret x A."""
    params = R.shape(oracle, pbits, cbits, n, entry_count, entry_size, 32)
    assert (params["chunks_per_entry"] > 1) == chunks_above_one
    assert (params["a_poly_count"] > 1) == polys_above_one
    rng = np.random.default_rng(n + entry_count)
    polys = R.a_polynomials(oracle, params, bytes(32))
    assert len(polys) == -(-params["database_columns"] // n)
    a_matrix = R.materialize_a(params, polys)
    secrets = R.ternary_secrets(params, rng)
    assert len(secrets) == params["chunks_per_entry"]
    by_matrix = R.secret_times_matrix(params, secrets, a_matrix)
    p = params["modulus"]
    exact = [[sum(int(s) % p * int(a) for s, a in zip(secret, row)) % p for row in a_matrix] for secret in secrets]
    assert np.array_equal(by_matrix, np.array(exact, dtype=np.uint64))
    assert np.array_equal(R.noiseless_sample_polynomial(params, polys, secrets), by_matrix)


def test_mod_switch_keeps_ternary(oracle):
    """ternarySecretKeyMapsCorrectlyAfterModSwitch (SimplePirTests.swift:127-145): 0, 1, p - 1 -> 0, 1, 2^c - 1."""
    params = R.shape(oracle, 5, 42, 2048, 5, 1, 64)
    p = params["modulus"]
    assert R.mod_switch(params, np.array([0, 1, p - 1], dtype=np.uint64)).tolist() == [0, 1, (1 << 42) - 1]
