"""The reference's 17 PredefinedRlweParameters without a device: the fixture is what its names say, the CPU oracle runs every set
through fresh encryption and mul -> relinearize -> applyGalois -> modSwitchDownToSingle to what the plaintext ring gives in
Python integers, and the library's host-only contexts construct for every set on every word size it supports.
tests/test_gpu_predefined_sets.py holds the device to the same chain."""
import ctypes
import math

import pytest

import heamd
import predefined_sets as sets


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
def test_there_are_seventeen_sets():
    assert len(sets.NAMES) == len(set(sets.NAMES)) == 17
    assert len(sets.CASES) == 17 + sum(s.scalar32 for s in sets.load())
    assert all(s.error_std_dev == "stdDev32" and s.source.startswith("Sources/HomomorphicEncryption/EncryptionParameters.swift:")
               for s in sets.load())


@pytest.mark.parametrize("name", sets.NAMES)
def test_names_state_the_bit_lengths(name):
    pset = sets.BY_NAME[name]
    degree, logq, logt = sets.name_fields(name)
    assert degree == pset.degree and degree & (degree - 1) == 0
    assert logq == [q.bit_length() for q in pset.moduli]
    assert logt == pset.t.bit_length()
    assert len(set(pset.moduli)) == len(pset.moduli)
    for q in pset.moduli:
        assert sets.is_ntt_modulus(q, degree) and q > pset.t, q
    assert sets.is_prime(pset.t)
    # Bfv<UInt32> holds moduli up to 2^30 - 1 (ModularArithmetic/Scalar.swift): the flag is set exactly where they fit
    assert pset.scalar32 == all(q < 1 << 30 for q in pset.moduli)


def test_ntt_unfriendly_plaintext_moduli_are_the_named_ones():
    """Six sets: logt_4, _5, _6 and _13 of n_4096_logq_27_28_28, n_4096_logq_16_33_33_logt_4 and n_8192_logq_29_60_60_logt_15,
    with t = 11, 17, 37, 4099, 11 and 16411 -- the six enum cases the reference marks `NTT-unfriendly plaintext modulus`."""
    unfriendly = {s.name: s.t for s in sets.load() if not sets.is_ntt_modulus(s.t, s.degree)}
    assert sorted(unfriendly) == sorted(sets.NTT_UNFRIENDLY)
    assert sorted(unfriendly.values()) == [11, 11, 17, 37, 4099, 16411]
    above_41_bits = [s.name for s in sets.load() if s.t >= 1 << 41]
    assert above_41_bits == ["n_8192_logq_3x55_logt_42"] and sets.BY_NAME[above_41_bits[0]].t == 2199023288321


def test_packing_classes():
    classes = sets.packing_classes()
    assert sorted(classes) == [3, 4, 5, 12, 14, 15, 16, 19, 23, 25, 28, 29, 41]
    assert classes[4].name == "insecure_n_8_logq_5x18_logt_5" and classes[14].degree == 16 and classes[19].degree == 512


# ---- the oracle against Python integers ----------------------------------------------------------------------------------------
def test_sparse_product_is_the_negacyclic_product():
    from bfv_helpers import negacyclic_multiply

    pset = sets.BY_NAME["insecure_n_16_logq_60_logt_15"]
    a, b, terms = sets.messages(pset)
    assert len(terms) == 8 and a[:4] == [0, pset.t - 1, (pset.t + 1) // 2, (pset.t + 1) // 2 - 1]
    assert sets.sparse_negacyclic_product(a, terms, pset.t) == negacyclic_multiply(a, b, pset.t)


@pytest.mark.parametrize("case", sets.CASES, ids=sets.case_id)
def test_oracle_chain_decrypts_to_the_plaintext_ring_model(case):
    chain = sets.chain(*case)
    pset = chain.pset
    a, b, terms = sets.messages(pset)
    assert all(0 <= v < pset.t for v in a + b) and {c for _, c in terms} >= {1, pset.t - 1}
    for m in sorted({chain.L, 1}):
        fresh = chain.fresh(m)
        for index, message in enumerate(chain.messages):
            assert chain.decrypt_exact(fresh[index]) == [int(v) for v in message], (m, index)
            assert chain.noise_budget(fresh[index]) > 0
    stages = chain.stages()
    expected = list(stages)
    if len(pset.moduli) == 1:
        assert expected == ["mul"]
    else:
        assert expected[:3] == ["mul", "relinearize", "apply_galois"] and expected[-1] == "single"
        assert stages["single"].shape == (1, 2, 1, pset.degree)
    product = sets.product_model(pset)
    for name, ct in stages.items():
        model = product if name in ("mul", "relinearize") else sets.chain_model(pset)
        assert chain.decrypt_exact(ct[0]) == model, name
        assert [int(v) for v in chain.decrypt(ct[0])] == model, name
        budget = chain.noise_budget(ct[0])
        assert budget > 0 and math.isfinite(budget), (name, budget)


@pytest.mark.parametrize("case", sets.CASES, ids=sets.case_id)
def test_oracle_roundings_equal_the_restatement_at_every_level(case):
    """scaleAndRound on the gamma thresholds and plaintextTranslate on 0, 1, (t + 1) / 2 - 1, (t + 1) / 2, t - 1 and the message
    whose Barrett estimate falls one short, with the set's own t: the oracle's words are rns_threshold_cases.Level's.  The device
    test takes the oracle's words for whole polynomials of these."""
    import numpy as np

    import rns_threshold_cases as cases

    chain = sets.chain(*case)
    ref, n, t = chain.ref, chain.pset.degree, chain.pset.t
    for m, level in cases.levels_of(ref, case[1]).items():
        assert (level.t, level.q) == (t, chain.moduli(m))
        threshold = cases.scale_threshold_columns(level, seed=300 + m)
        data = cases.rows(threshold, n)
        for factor in (1, 2, t - 1):
            restated = cases.expected_rows(threshold, n, lambda x: level.scale_and_round(x, factor))
            assert np.array_equal(ref.rns_tool(m).scale_and_round(data, factor), restated[0]), (m, factor)
        messages = cases.translate_messages(level, n)
        assert {level.plaintext_translate([0] * m, v)[1] for v in messages[:min(n, 24)]} == {False, True}
        rng = np.random.default_rng(m)
        ct = np.stack([rng.integers(0, q, size=(1, 2, n), dtype=np.uint64) for q in chain.moduli(m)], axis=2)
        for subtract in (False, True):
            got = ref.plaintext_translate(ct, np.array([messages], dtype=np.uint64), 2, subtract, moduli_count=m)
            for k in range(min(n, 24)):
                words = level.plaintext_translate([int(v) for v in ct[0, 0, :, k]], messages[k], subtract)[0]
                assert [int(v) for v in got[0, 0, :, k]] == words, (m, subtract, k)


def test_threshold_sets_take_a_plaintext_modulus_by_value(oracle):
    import rns_threshold_cases as cases

    ctx, levels = cases.build_set(oracle, "q40x3", t_value=11)  # not an NTT modulus for N = 64
    assert ctx.t == 11 and not sets.is_ntt_modulus(11, ctx.degree) and all(level.t == 11 for level in levels.values())
    assert cases.build_set(oracle, "q40x3")[0].t == cases.build_set(oracle, "q40x3", t_bits=17)[0].t != 11


@pytest.mark.parametrize("case", sets.ROUND_TRIPS, ids=sets.case_id)
def test_oracle_mulpir_round_trip(case):
    """What the reference's protocol itself makes of one query over a 4 x 3 database at t = 11 and at the 42-bit t: at t = 11 the
    response has some 15 bits of budget left and decrypts to the queried entry; at t = 2^41 + 32769 a database plaintext times a
    selection ciphertext uses up the 110-bit Q (a budget of a thousandth of a bit) and the entry comes back wrong.  The device
    test asserts the entry only where this one finds it."""
    trip = sets.round_trip(*case)
    assert trip.plan["entries_per_plaintext"] == 3 and trip.plan["reply_ciphertext_count"] == 1
    assert trip.plan["query_ciphertext_count"] == 1 and trip.plan["expanded_query_count"] == trip.INPUTS
    assert trip.present.all() and trip.size > 0
    assert trip.decrypts == sets.ROUND_TRIP_DECRYPTS[case[0]], trip.budget
    assert (trip.budget > 1) == trip.decrypts, trip.budget


# ---- host-side ABI -------------------------------------------------------------------------------------------------------------
class HostBfv32:
    """a host-only Context<Bfv<UInt32>> (heamd.BfvContext32's constructor wants a device)"""

    word_bits = 32

    def __init__(self, degree, t, moduli):
        lib = heamd.load_library()
        self.h, self.degree, self.t = ctypes.c_void_p(), degree, t
        array = (ctypes.c_uint64 * len(moduli))(*moduli)
        code = lib.he_bfv_context_create_u32_host_only(degree, t, array, len(moduli), ctypes.byref(self.h))
        assert code == 0, heamd.binding.STATUS_NAMES[code]
        self.L = int(lib.he_bfv_ciphertext_moduli_count(self.h))

    def bsk_moduli(self):
        out = (ctypes.c_uint64 * (self.L + 1))()
        assert heamd.load_library().he_bfv_copy_bsk_moduli(self.h, out) == 0
        return [int(v) for v in out]

    def __del__(self):
        if self.h:
            heamd.load_library().he_bfv_context_destroy(self.h)


def host_context(pset, word):
    if word == 32:
        return HostBfv32(pset.degree, pset.t, list(pset.moduli))
    return heamd.BfvContext(pset.degree, pset.t, list(pset.moduli), host_only=True)


@pytest.mark.parametrize("case", sets.CASES, ids=sets.case_id)
def test_host_only_contexts_construct(oracle, case):
    name, word = case
    pset = sets.BY_NAME[name]
    ours = host_context(pset, word)
    ref = oracle.BfvContext(pset.degree, pset.t, list(pset.moduli), word_bits=word)
    assert ours.L == ref.L == max(1, len(pset.moduli) - 1)
    assert ours.bsk_moduli() == ref.rns_tool().bsk
    if word == 64:
        for k in range(1, ours.L + 1):
            assert ours.ciphertext_context(k).moduli == ref.ciphertext_context(k).moduli == list(pset.moduli[:k])
            assert ours.qbsk_context(k).moduli == ref.qbsk_context(k).moduli
    if not pset.scalar32:  # a modulus of 2^30 or more is no Bfv<UInt32> modulus
        with pytest.raises(AssertionError, match="invalidEncryptionParameters"):
            HostBfv32(pset.degree, pset.t, list(pset.moduli))


@pytest.mark.parametrize("case", sets.CASES, ids=sets.case_id)
def test_simd_encoding_needs_an_ntt_friendly_plaintext_modulus(case):
    name, word = case
    ours = host_context(sets.BY_NAME[name], word)
    if name in sets.NTT_UNFRIENDLY:
        with pytest.raises(heamd.HeError) as err:
            heamd.PnnsContext(ours)
        assert err.value.name == "simdEncodingNotSupported"
    else:
        assert heamd.PnnsContext(ours).h
