"""Holds word32_cases.py itself to Python integers before test_gpu_word32_edges.py and test_gpu_bfv.py hold the device to
it: every prime set it names is obtainable, its rows carry the patterns they claim on every modulus, the oracle's
transforms of them agree with a direct O(N^2) evaluation at the odd powers of psi (no butterflies) for N <= 64, and its
element-wise tables hold every operand pair at 0, 1 and p - 1."""
import numpy as np
import pytest

import word32_cases as cases


def test_every_degree_has_its_five_moduli(oracle):
    for degree in cases.DEGREES:
        moduli = cases.degree_moduli(oracle, degree)
        assert len(set(moduli)) == 5, degree
        for p in moduli:
            assert oracle.is_prime(p) and p % (2 * degree) == 1, (degree, p)
        large, small = moduli[0::2], moduli[1::2]
        assert all(p.bit_length() == 30 for p in large) and large == sorted(large, reverse=True), degree
        assert all(p.bit_length() == cases.small_prime_bits(degree) for p in small), degree
        # the three LARGEST: no NTT prime of the degree lies between them and 2^30
        candidate = ((1 << 30) - 1) // (2 * degree) * (2 * degree) + 1
        found = []
        while len(found) < 3:
            if oracle.is_prime(candidate):
                found.append(candidate)
            candidate -= 2 * degree
        assert found == large, degree
    # the top of the butterflies' range: 4 p - 1 within 140 of 2^32 at N = 2
    assert 4 * cases.degree_moduli(oracle, 2)[0] == 0xFFFFFF74


def test_every_modulus_meets_every_pattern(oracle):
    for degree in (2, 64, 4096):
        moduli, slabs = cases.edge_slabs(oracle, degree)
        assert [s.shape for s in slabs] == [(7, 5, degree), (1, 5, degree)]
        for mi, p in enumerate(moduli):
            seen = {cases.pattern_of(poly, mi) for poly in range(cases.EDGE_POLYS + 1)}
            assert seen == set(cases.PATTERNS), (degree, mi)
            rows = {cases.pattern_of(poly, mi): (slabs[0][poly, mi] if poly < 7 else slabs[1][0, mi]) for poly in range(8)}
            assert not rows["zero"].any() and (rows["full"] == p - 1).all()
            assert (rows["even"][0::2] == p - 1).all() and not rows["even"][1::2].any()
            assert (rows["odd"][1::2] == p - 1).all() and not rows["odd"][0::2].any()
            assert rows["last"][-1] == p - 1 and rows["last"].sum() == p - 1
            assert rows["x"][1] == 1 and rows["x"].sum() == 1
            assert (rows["half"][:degree // 2] == p - 1).all() and not rows["half"][degree // 2:].any()
            assert (rows["uniform"] < p).all() and (degree < 64 or len(set(rows["uniform"].tolist())) > degree // 2)


@pytest.mark.parametrize("degree", [d for d in cases.DEGREES if d <= 64])
def test_expected_transforms_against_direct_evaluation(oracle, degree):
    moduli, slabs = cases.edge_case(oracle, degree)
    ref = oracle.PolyContext(degree, moduli)
    for slab, forward, inverse in slabs:
        for mi, p in enumerate(moduli):
            psi = cases.psi_of(ref.ntt_tables(mi), degree, p)
            for poly in range(slab.shape[0]):
                assert forward[poly, mi].tolist() == cases.direct_forward(slab[poly, mi], p, psi), (poly, mi)
                assert inverse[poly, mi].tolist() == cases.direct_inverse(slab[poly, mi], p, psi), (poly, mi)


def test_expected_transforms_round_trip_at_every_degree(oracle):
    """Above N = 64 the direct evaluation is too slow to repeat on every run; there the oracle's two transforms are held to
    each other, and the monomial x to its closed form X[i] = psi^(2 bitrev(i) + 1)."""
    for degree in cases.DEGREES:
        moduli, slabs = cases.edge_case(oracle, degree)
        ref = oracle.PolyContext(degree, moduli)
        bits = degree.bit_length() - 1
        for slab, forward, inverse in slabs:
            assert np.array_equal(ref.inverse_ntt(forward), slab) and np.array_equal(ref.forward_ntt(inverse), slab), degree
        for mi, p in enumerate(moduli):
            poly = next(k for k in range(8) if cases.pattern_of(k, mi) == "x")
            forward = slabs[0][1][poly, mi] if poly < 7 else slabs[1][1][0, mi]
            psi = cases.psi_of(ref.ntt_tables(mi), degree, p)
            for i in (0, 1, degree // 2, degree - 1):
                assert int(forward[i]) == pow(psi, 2 * cases.bit_reverse(i, bits) + 1, p), (degree, mi, i)


def test_period_and_crowded_prime_sets(oracle):
    for degree in cases.PERIOD_DEGREES:
        for period in cases.PERIODS:
            moduli = oracle.generate_primes([cases.PERIOD_BITS] * period, False, degree, word_bits=32)
            assert len(set(moduli)) == period and all(p.bit_length() == 28 and p % (2 * degree) == 1 for p in moduli)
    for degree, bits, polys in cases.CROWDED:
        moduli = oracle.generate_primes(list(bits), False, degree, word_bits=32)
        assert len(set(moduli)) == len(bits) and [p.bit_length() for p in moduli] == list(bits)
        assert all(p % (2 * degree) == 1 for p in moduli)
    assert cases.CROWDED[0][2] * len(cases.CROWDED[0][1]) == 1200 and cases.CROWDED[2][2] % 2 == 1
    assert oracle.is_prime(cases.REFUSED_MODULUS) and cases.REFUSED_MODULUS % (2 * cases.REFUSED_DEGREE) == 1


def test_product_case_against_the_transforms(oracle):
    """The schoolbook product is the one the oracle's transforms give: inverse(forward(x) * forward(y))."""
    p, x, y, product = cases.product_case(oracle)
    ref = oracle.PolyContext(cases.PRODUCT_DEGREE, [p])
    assert np.array_equal(ref.inverse_ntt(ref.mul(ref.forward_ntt(x), ref.forward_ntt(y))), product)
    assert (x[1] == p - 1).all() and (y[1] == p - 1).all()
    # x^(N-1) y rotates y by N - 1 places, negating what wraps: coefficient 0 of y lands on N - 1, the others come back negated
    assert product[2, 0, -1] == y[2, 0, 0] and product[2, 0, 0] == (p - int(y[2, 0, 1])) % p


@pytest.mark.parametrize("degree", cases.ELEMENTWISE_DEGREES)
def test_elementwise_tables(oracle, degree):
    moduli, lhs, rhs = cases.elementwise_case(oracle, degree)
    assert moduli[0] == cases.degree_moduli(oracle, degree)[0]  # the largest 30-bit NTT prime of the degree
    assert moduli[1].bit_length() == 20 and moduli[2] == min(cases.degree_moduli(oracle, degree))
    ref = oracle.PolyContext(degree, moduli)
    for mi, p in enumerate(moduli):
        tables = degree // 49
        pairs = set(zip(lhs[0, mi, :49 * tables].tolist(), rhs[0, mi, :49 * tables].tolist()))
        assert pairs == set(cases.edge_pairs(p)) and len(pairs) == 49
        assert {0, 1, p - 1} <= set(cases.edge_values(p)) and (lhs[:, mi] < p).all() and (rhs[:, mi] < p).all()
    # the oracle agrees with the Python integers on the same operands
    for op, fn in (("add", ref.add), ("sub", ref.sub), ("mul", ref.mul)):
        assert np.array_equal(cases.elementwise_expected(op, moduli, lhs, rhs), fn(lhs, rhs)), op
    assert np.array_equal(cases.elementwise_expected("neg", moduli, lhs), ref.neg(lhs))
    negated = cases.elementwise_expected("neg", moduli, lhs)
    for mi, p in enumerate(moduli):  # neg(0) = 0, not p
        assert (negated[0, mi][lhs[0, mi] == 0] == 0).all() and (lhs[0, mi] == 0).any()
    for scalars in cases.edge_scalars(moduli):
        assert np.array_equal(cases.elementwise_expected("mul_scalar", moduli, lhs, scalars=scalars), ref.mul_scalar(lhs, scalars))


def test_many_moduli_sets(oracle):
    """Every set of test_many_moduli_at_a_tiled_degree exists, is admitted by the reference's Context (the oracle builds it),
    and lies on the side of each term-count decision it is listed for."""
    degree = cases.MANY_MODULI_DEGREE
    sides = {}
    for name, word_bits, bits, _ in cases.MANY_MODULI_SETS:
        bits_of, t, q = cases.many_moduli_set(oracle, name)
        assert bits_of == word_bits and len(set(q)) == len(bits) and [p.bit_length() for p in q] == bits
        ref = oracle.BfvContext(degree, t, q, word_bits=word_bits)
        L = ref.L
        assert L == len(bits) - 1
        if word_bits == 32:
            # Context.swift:122-124: L + 1 moduli must stay below the lazy product count of the key-switching context
            assert L + 1 < ref.key_switching_context().max_lazy_product_accumulation_count(32), name
            sides[name] = L > 15
            assert L * (max(q) - 1) ** 2 < 1 << 64 or L > 15, name  # the fused load's 64-bit sum
        else:
            sides[name] = not (L <= 8 and all(L * p < 1 << 63 for p in q))
        polys = cases.batch_above_finish_threshold(word_bits, L)
        threshold = cases.FINISH_IN_STORE_ROWS[word_bits]
        assert (polys - 1) * 2 * (L + 1) <= threshold < polys * 2 * (L + 1), name
        assert 3 * 2 * (L + 1) <= threshold, name
    assert sides == {"w32_30x14": False, "w32_26x16": True, "w64_60x8": False, "w64_55x9": True, "w64_61x4": False,
                     "w64_61x5": True, "w64_50x16": True}
    assert cases.batch_above_finish_threshold(32, 14) == 69 and cases.batch_above_finish_threshold(64, 8) == 57
    # one more 30-bit modulus is past what the reference admits
    t = oracle.generate_primes([17], True, degree)[0]
    q15 = oracle.generate_primes([30] * 16, False, degree, word_bits=32)
    with pytest.raises(oracle.OracleError):
        oracle.BfvContext(degree, t, q15, word_bits=32)
    # the largest 64-bit product sum: 14 (p - 1)^2 starts with 0xE0
    _, _, q = cases.many_moduli_set(oracle, "w32_30x14")
    assert (14 * (max(q) - 1) ** 2) >> 56 in (0xDF, 0xE0)
    # the smallest 61-bit primes are the Bsk base, and four 61-bit moduli never reach 2^63
    for bits, small in cases.INADMISSIBLE_SETS:
        q = oracle.generate_primes(bits, small, degree)
        assert all(4 * p < 1 << 63 for p in q)
        with pytest.raises(oracle.OracleError):
            oracle.BfvContext(degree, t, q)


def test_many_moduli_slab_layout():
    rng = np.random.default_rng(0)
    moduli = [97, 193, 257]
    ct = cases.many_moduli_slab(rng, (4, 2), moduli, degree=8)
    assert ct.shape == (4, 2, 3, 8) and (ct[0] == np.array([96, 192, 256], dtype=np.uint64)[None, :, None]).all()
    assert not ct[1].any() and ct[2:].any() and all((ct[:, :, i] < m).all() for i, m in enumerate(moduli))
    key = cases.many_moduli_slab(rng, (2, 2), moduli, zero_second=False, degree=8)
    assert (key[0] == np.array([96, 192, 256], dtype=np.uint64)[None, :, None]).all() and key[1].any()
