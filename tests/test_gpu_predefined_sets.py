"""Every PredefinedRlweParameters set of the reference (tests/golden/predefined_parameter_sets.json) on the device, on 8-byte
words and, where the set supports Bfv<UInt32>, on packed 4-byte words -- bit-exact against the CPU oracle, the Python-integer
restatements (encrypt_reference.py, decrypt_reference.py, rns_threshold_cases.py) and the plaintext-ring model of
tests/predefined_sets.py, which tests/test_predefined_sets.py holds the oracle to without a device:

  context     the exported constants (moduli of every level's contexts, the Bsk primes, NTT tables)
  chain       secret key -> encryptions at every moduli count -> relinearization and Galois keys -> mul -> relinearize ->
              applyGalois -> modSwitchDown .. -> one modulus -> decrypt and noise budget, every stage made on the device from the
              stage before and compared word for word; the last plaintext is the model's
  roundings   plaintext <-> Eval, add / subtract a plaintext, scaleAndRound on 0, 1, (t + 1) / 2 - 1, (t + 1) / 2, t - 1 in
              every lane, on the gamma thresholds and on 0 and q_i - 1
  ct x ct     uniform words with the extremes of every residue, unfused and through the row-fused kernels
  packing     once per floor(log2 t): database processing from raw bytes and the client's reply extraction
  MulPIR      indices -> query -> response -> entry on the device for t = 11 and for the 42-bit t

The degrees are the sets' own; batches are 2-3 ciphertexts.  A set with one coefficient modulus (insecure_n_16_logq_60_logt_15)
has no key-switching modulus: it runs the stages that exist there."""
import functools

import numpy as np
import pytest
import torch

import decrypt_reference
import encrypt_reference
import heamd
import pir_client_reference as client
import pir_database_reference as refdb
import predefined_sets as sets
import rns_threshold_cases as cases
from bfv_helpers import galois_plain
from test_gpu_decrypt import _budgets_agree
from test_gpu_encrypt import Case, _device_seeds

pytestmark = pytest.mark.gpu


class SetCase(Case):
    """test_gpu_encrypt.Case on a predefined set, with the key of the oracle's chain (predefined_sets.Chain)"""

    def __init__(self, name, word):
        self.chain = sets.chain(name, word)
        self.pset = self.chain.pset
        self.setup(self.chain.host)
        self.levels = cases.levels_of(self.ref_ctx, word)

    def uniform(self, rng, prefix, moduli):
        rows = [rng.integers(0, q, size=tuple(prefix) + (self.degree,), dtype=np.uint64) for q in moduli]
        return np.ascontiguousarray(np.stack(rows, axis=len(prefix)))


@functools.lru_cache(maxsize=None)
def set_case(name, word):
    return SetCase(name, word)


@pytest.fixture(params=sets.CASES, ids=sets.case_id)
def case(request):
    return set_case(*request.param)


# ---- context -------------------------------------------------------------------------------------------------------------------
def test_context_matches_the_oracle(case):
    ours, ref = case.ctx, case.ref_ctx
    assert ours.L == ref.L == case.chain.L and ours.t == case.pset.t
    assert ours.bsk_moduli() == ref.rns_tool().bsk
    for k in range(1, ours.L + 1):
        assert ours.ciphertext_context(k).moduli == ref.ciphertext_context(k).moduli == list(case.pset.moduli[:k])
        assert ours.qbsk_context(k).moduli == ref.qbsk_context(k).moduli
        if case.L_all > 1:
            assert ours.key_switching_context(k).moduli == ref.key_switching_context(k).moduli
    rows = len(ref.qbsk_context().moduli)
    for row in (0, ours.L - 1, ours.L, rows - 1):
        a, b = ours.qbsk_context().ntt_tables(row), ref.qbsk_context().ntt_tables(row)
        assert np.array_equal(a["root_powers"], b["root_powers"]), row
        assert np.array_equal(a["inv_root_factors"], b["inv_root_factors"]), row


# ---- the chain -----------------------------------------------------------------------------------------------------------------
def _encryptions(case, m=None):
    chain = case.chain
    return case.ctx.encrypt(case.to_device(chain.messages), case.s_device, _device_seeds(chain.a_seeds),
                            _device_seeds(chain.error_seeds), m)


def _evaluation_keys(case):
    chain = case.chain
    relin = case.ctx.generate_relinearization_key(case.s_device, _device_seeds(chain.relin_seeds[0]),
                                                  _device_seeds(chain.relin_seeds[1]))
    galois = case.ctx.generate_galois_keys(case.s_device, chain.elements, _device_seeds(chain.galois_seeds[0]),
                                           _device_seeds(chain.galois_seeds[1]))
    return relin, galois


def test_secret_keys_and_encryptions_at_every_moduli_count(case):
    chain, t = case.chain, case.t
    got = case.to_host(case.keys_device)
    for b, seed in enumerate(case.key_seeds):
        assert np.array_equal(got[b], encrypt_reference.generate_secret_key(case.secret_ctx, bytes(seed), case.stream)), b
    for m in range(1, case.L + 1):
        cts = _encryptions(case, m)
        assert np.array_equal(case.to_host(cts), chain.fresh(m)), m
        assert np.array_equal(case.to_host(case.ctx.decrypt(cts, case.s_device)), chain.messages), m
        norms = case.ctx.noise_norm(cts, case.s_device)
        assert norms == [chain.noise_norm(ct) for ct in chain.fresh(m)], m
        assert all(norm <= 21 * t + (t + 1) // 2 for norm in norms), m  # as tests/test_gpu_encrypt.py derives it


def test_evaluation_keys(case):
    if case.L_all == 1:  # Context.supportsEvaluationKey is false without a key-switching modulus
        seeds = _device_seeds(sets.seeds(1, 9))
        for call in (lambda: case.ctx.generate_relinearization_key(case.s_device, seeds, seeds),
                     lambda: case.ctx.generate_galois_keys(case.s_device, [3], seeds, seeds)):
            with pytest.raises(heamd.HeError) as caught:
                call()
            assert caught.value.name == "unsupportedHeOperation"
        return
    relin, galois = _evaluation_keys(case)
    assert np.array_equal(case.to_host(relin), case.chain.relinearization_key())
    assert np.array_equal(case.to_host(galois), case.chain.galois_keys())


def _decrypts_as(case, device_ct, reference_ct, model):
    """plaintext, exact noise norm and budget of one device ciphertext [1][polys][m][N] against the restatements"""
    chain = case.chain
    plain = case.to_host(case.ctx.decrypt(device_ct, case.s_device))[0]
    assert [int(v) for v in plain] == model
    assert decrypt_reference.decrypt(chain.dot(reference_ct[0]), chain.moduli(reference_ct.shape[2]), case.t) == model
    norm = chain.noise_norm(reference_ct[0])
    assert case.ctx.noise_norm(device_ct, case.s_device) == [norm]
    budget = case.ctx.noise_budget(device_ct, case.s_device)
    # (the budget is log2 of a double quotient: the library's and Python's log2 may round differently, by an ulp at most)
    _budgets_agree(budget, [decrypt_reference.noise_budget(norm, chain.moduli(reference_ct.shape[2]))])
    assert budget[0] > 0
    return budget[0]


def test_chain_on_the_device_stage_by_stage(case):
    chain, ctx, pset = case.chain, case.ctx, case.pset
    stages = chain.stages()
    cts = _encryptions(case)
    a = [int(v) for v in chain.messages[0]]
    _decrypts_as(case, cts[:1].contiguous(), chain.fresh(case.L)[:1], a)
    product = ctx.mul(cts[:1].contiguous(), cts[1:2].contiguous())
    assert np.array_equal(case.to_host(product), stages["mul"])
    _decrypts_as(case, product, stages["mul"], sets.product_model(pset))  # three polynomials
    if case.L_all == 1:
        assert list(stages) == ["mul"]
        return
    relin_key, galois = _evaluation_keys(case)
    relin = ctx.relinearize(product, relin_key)
    assert np.array_equal(case.to_host(relin), stages["relinearize"])
    rotated = ctx.apply_galois(relin, sets.GALOIS_ELEMENT, galois[0].contiguous())
    assert np.array_equal(case.to_host(rotated), stages["apply_galois"])
    current = rotated
    for level in range(case.L, 1, -1):
        current = ctx.mod_switch_down(current, 2, level)
        assert np.array_equal(case.to_host(current), stages["mod_switch_down_%d" % level]), level
    wide = heamd.widen_u32(rotated) if case.word == 32 else rotated  # modSwitchDownToSingle takes 8-byte slabs
    assert np.array_equal(heamd.to_host(ctx.mod_switch_down_to_single(wide, 2)), stages["single"])
    _decrypts_as(case, current, stages["single"], sets.chain_model(pset))
    # the other key: x -> x^(2N - 1) on the fresh encryption of A
    element = chain.elements[1]
    swapped = ctx.apply_galois(cts[:1].contiguous(), element, galois[1].contiguous())
    expected = case.ref_ctx.apply_galois(chain.fresh(case.L)[:1], element, chain.galois_keys()[1])
    assert np.array_equal(case.to_host(swapped), expected)
    _decrypts_as(case, swapped, expected, galois_plain(a, element, case.t))


# ---- roundings that depend on t ------------------------------------------------------------------------------------------------
def _edge_plaintexts(case, rng):
    """[3][N]: 0, 1, (t + 1) / 2 - 1, (t + 1) / 2, t - 1 cycled so that each meets each lane of a pair and of a quad (from
    N = 32 on), the same one coefficient on, and uniform values"""
    t, n = case.t, case.degree
    five = [0, 1, (t + 1) // 2 - 1, (t + 1) // 2, t - 1]
    row = np.array([five[i] for i in cases.cycled(5, n)], dtype=np.uint64)
    return np.stack([row, np.roll(row, 1), rng.integers(0, t, n).astype(np.uint64)])


def test_plaintext_conversions_and_translation_at_every_level(case):
    ours, ref, t, n = case.ctx, case.ref_ctx, case.t, case.degree
    rng = np.random.default_rng(n + t % 9973)
    values = _edge_plaintexts(case, rng)
    for m in range(1, case.L + 1):
        moduli, level = case.chain.moduli(m), case.levels[m]
        lifted = ours.plaintext_to_eval(case.to_device(values), m)
        expected = ref.plaintext_to_eval(values, m)
        assert np.array_equal(case.to_host(lifted).reshape(expected.shape), expected), m
        # Plaintext.convertToEvalFormat lifts v to v + (Q - t) above the centre (Plaintext.swift:149-170): the rows, restated
        q = cases.prod(moduli)
        centred = [[(int(v) + (q - t if int(v) >= (t + 1) // 2 else 0)) % qi for v in values[0]] for qi in moduli]
        assert np.array_equal(ref.ciphertext_context(m).inverse_ntt(expected[:1])[0], np.array(centred, dtype=np.uint64)), m
        back = ours.plaintext_to_coeff(lifted, m)
        assert np.array_equal(case.to_host(back).reshape(values.shape), values), m
        assert np.array_equal(ref.plaintext_to_coeff(expected, m), values), m
        for polys in (2, 3):
            ct = case.uniform(rng, (3, polys), moduli)
            for subtract in (False, True):
                got = case.to_host(ours.add_plain_(case.to_device(ct), case.to_device(values), polys, subtract, moduli_count=m))
                assert np.array_equal(got, ref.plaintext_translate(ct, values, polys, subtract, moduli_count=m)), (m, polys)
                for k in range(min(n, 20)):  # the five values in Python integers (rns_threshold_cases.Level)
                    words = level.plaintext_translate([int(v) for v in ct[0, 0, :, k]], int(values[0, k]), subtract)[0]
                    assert [int(v) for v in got[0, 0, :, k]] == words, (m, polys, subtract, k)
                assert np.array_equal(got[:, 1:], ct[:, 1:])


# Where mod_gamma can be steered onto its thresholds (rns_threshold_cases.scale_threshold_columns: only a level with
# Q > gamma t).  Every other (case, level) gets 64 random columns in their place, for which only "both sides of gamma / 2 occur" is
# asserted: with the 8-byte gamma of 2^62 that is every level of n_4096_logq_27_28_28_* and n_4096_logq_16_33_33_logt_4 on 8-byte
# words (so t = 11, 17, 37 and 4099 meet constructed thresholds on packed 4-byte words only, and 16_33_33's t = 11 nowhere),
# every level of one modulus, and the lower levels of the two small test sets.
CONSTRUCTED_THRESHOLD_LEVELS = {
    ("insecure_n_512_logq_4x60_logt_20", 64): [2, 3], ("insecure_n_8_logq_5x18_logt_5", 64): [4],
    ("insecure_n_8_logq_5x18_logt_5", 32): [3, 4],
    **{(s.name, 32): [2] for s in sets.load() if s.scalar32 and s.degree == 4096},
    **{(s.name, 64): [2] for s in sets.load() if s.degree == 8192},
}


def test_scale_and_round_at_every_level(case):
    """scaleAndRound with factors 1, 2 and t - 1 on uniform rows with 0 and q_i - 1 columns and on the gamma-threshold columns,
    against the oracle and (the threshold columns) the Python-integer restatement.  CONSTRUCTED_THRESHOLD_LEVELS says where those
    columns sit ON the six thresholds of mod_gamma and where they are random."""
    ours, ref, t, n = case.ctx, case.ref_ctx, case.t, case.degree
    rng = np.random.default_rng(n + t % 9967)
    constructed = CONSTRUCTED_THRESHOLD_LEVELS.get((case.pset.name, case.word), [])
    for m in range(1, case.L + 1):
        moduli, level, tool = case.chain.moduli(m), case.levels[m], ref.rns_tool(m)
        threshold = cases.scale_threshold_columns(level, seed=300 + m)
        assert level.scale_and_round_reaches_targets() == (m in constructed), m
        if m in constructed:
            assert {level.scale_and_round(column)[1] for column in threshold} == set(level.scale_and_round_targets()), m
        data = np.concatenate([case.uniform(rng, (2,), moduli), cases.rows(threshold, n)[None]])
        data[0, :, 0], data[0, :, 1 % n] = 0, np.array(moduli, dtype=np.uint64) - np.uint64(1)
        data[1, :, ::2] = (np.array(moduli, dtype=np.uint64) - np.uint64(1))[:, None]
        sides = {level.scale_and_round(column)[1] > level.gamma // 2 for column in threshold}
        assert sides == {False, True}, m
        for factor in (1, 2, t - 1):
            got = case.to_host(ours.scale_and_round(case.to_device(data), factor, moduli_count=m))
            assert np.array_equal(got, np.stack([tool.scale_and_round(p, factor) for p in data])), (m, factor)
            restated = cases.expected_rows(threshold, n, lambda x: level.scale_and_round(x, factor))
            assert np.array_equal(got[2], restated[0]), (m, factor)


# ---- ct x ct at random words ---------------------------------------------------------------------------------------------------
def _mul_operands(case, rng, batch):
    moduli = case.chain.moduli(case.L)
    lhs, rhs = case.uniform(rng, (batch, 2), moduli), case.uniform(rng, (batch, 2), moduli)
    top = (np.array(moduli, dtype=np.uint64) - np.uint64(1))[None, :, None]
    lhs[-1], rhs[-1] = top, top  # the extremes of every residue in the last ciphertext
    rhs[-1, 1, :, ::2] = 0
    lhs[-1, 0, :, :2] = 0
    return lhs, rhs


def test_mul_on_uniform_words(case):
    from conftest import host_threads

    rng = np.random.default_rng(case.degree + case.t % 9949 + case.word)
    lhs, rhs = _mul_operands(case, rng, 3)
    got = case.to_host(case.ctx.mul(case.to_device(lhs), case.to_device(rhs)))
    assert np.array_equal(got, case.ref_ctx.mul(lhs, rhs, threads=host_threads()))


# the row-fused kernels exist for 8-byte slabs only (bfv_api.cpp takes them under W = uint64_t): the 14 sets at N = 4096 and
# 8192 with more than one ciphertext modulus, each on 8-byte words
FUSED = [c for c in sets.CASES
         if c[1] == 64 and sets.BY_NAME[c[0]].degree in (4096, 8192) and len(sets.BY_NAME[c[0]].moduli) > 2]


@pytest.mark.parametrize("name,word", FUSED, ids=[sets.case_id(c) for c in FUSED])
def test_mul_through_the_row_fused_kernels(monkeypatch, name, word):
    """HEAMD_BEHZ_FUSED_ABOVE=256 and the smallest batch with more than 256 (item, [Q, Bsk] row) pairs: t N^-1 under every
    butterfly class the set's rows select; the first three products are the unfused pipeline's, too.  8-byte words only: on
    packed 4-byte slabs the library has no row-fused path and the variable changes nothing."""
    from conftest import host_threads

    case = set_case(name, word)
    monkeypatch.setenv("HEAMD_BEHZ_FUSED_ABOVE", "256")
    batch = 256 // (2 * case.L + 1) + 1
    rng = np.random.default_rng(case.degree + case.t % 9941 + word)
    lhs, rhs = _mul_operands(case, rng, batch)
    got = case.to_host(case.ctx.mul(case.to_device(lhs), case.to_device(rhs)))
    assert np.array_equal(got, case.ref_ctx.mul(lhs, rhs, threads=host_threads()))
    few = case.to_host(case.ctx.mul(case.to_device(lhs[:3].copy()), case.to_device(rhs[:3].copy())))
    assert np.array_equal(few, got[:3])


# ---- coefficient packing, once per floor(log2 t) -------------------------------------------------------------------------------
PACKING = [(bits, s.name, word) for bits, s in sorted(sets.packing_classes().items()) for word in ((64, 32) if s.scalar32 else (64,))]
PACKING_IDS = ["bits%d-%s-u%d" % p for p in PACKING]


def _entry_size(bits, width_of, low):
    """the first size from `low` on whose record (prefix included) ends inside a coefficient, where `bits` leaves such a size"""
    for size in range(low, low + 2 * bits):
        if 8 * (width_of(size) + size) % bits != 0:
            return size
    return low


@pytest.mark.parametrize("bits,name,word", PACKING, ids=PACKING_IDS)
def test_database_bytes_to_coefficients(oracle, bits, name, word):
    """MulPirServer.process from raw bytes at `bits` bits per coefficient against pir_database_reference.py: packed and split
    layouts, with and without a size prefix, entry sizes whose records end inside a coefficient (whenever 8 is no multiple of
    `bits`, coefficients also begin and end inside bytes)."""
    case = set_case(name, word)
    assert case.t.bit_length() - 1 == bits
    bpp, dims = case.degree * bits // 8, [4, 3]
    rng = np.random.default_rng(bits + word)
    for mode, encoding in (("pack", True), ("pack", False), ("split", True), ("split", False)):
        width_of = refdb.encoding_width if encoding else (lambda size: 0)
        if mode == "pack":
            entry_size = _entry_size(bits, width_of, max(1, min(37, (bpp - 1) // 3 - 1)))
            per = bpp // (width_of(entry_size) + entry_size)
            assert per >= 2
            count = 12 * per - min(per, 3)  # the last plaintext is short of entries
        else:
            entry_size = _entry_size(bits, width_of, 2 * bpp + bpp // 3 + 1)  # three chunks, the last one a third full
            count = 11  # the last row is nil
        entries, padded, sizes = refdb.varying_entries(rng, count, entry_size)
        want_db, want_present = refdb.process(oracle, case.ref_ctx, entries, dims, entry_size, encoding)
        database, present = case.ctx.pir_process_database(torch.from_numpy(padded).cuda(), dims, entry_size, encoding,
                                                          entry_sizes=sizes)
        assert np.array_equal(present.cpu().numpy(), want_present), (mode, encoding)
        assert np.array_equal(case.to_host(database).reshape(want_db.shape), want_db), (mode, encoding)
        assert want_db.shape[0] == (1 if mode == "pack" else 3)


def _reply_plaintexts(oracle, rng, p, t, index, size):
    """[R][N] coefficients of a reply: random bytes with `index`'s size prefix set, then every third field behind that prefix
    moved into [2^bits, t) -- every such residue where there are at most 64, else the first two, the last and random ones --
    walking the fields that begin a byte and those that do not separately, so that each residue meets both kinds.
    -> (coefficients, number of byte-aligned fields moved, number of the others)"""
    bits, bpp, n = p["bits"], p["bytes_per_plaintext"], p["degree"]
    width, R = p["entry_size_encoding_width"], p["reply_ciphertext_count"]
    data = bytearray(rng.integers(0, 256, R * bpp, dtype=np.uint8).tobytes())
    start = (index % p["entries_per_plaintext"]) * p["encoded"]
    data[start:start + width] = refdb.prefix(size, width)
    coefficients = np.stack([refdb.unpack(oracle, bytes(data[k * bpp:(k + 1) * bpp]), bits, n) for k in range(R)])
    low = 1 << bits
    residues = list(range(low, t)) if t - low <= 64 else [low, low + 1, t - 1] + [int(v) for v in rng.integers(low, t, 13)]
    moved = [0, 0]
    for plaintext in range(R):
        first_bit = ((start + width) * 8 + bits) if plaintext == 0 else bits  # bit `bits` spills into the field in front
        fields = [k for k in range(n) if k * bits >= first_bit]
        for kind, chosen in enumerate(([k for k in fields if k * bits % 8 == 0], [k for k in fields if k * bits % 8 != 0])):
            for j, k in enumerate(chosen[::3]):
                coefficients[plaintext, k] = residues[j % len(residues)]
                moved[kind] += 1
    return coefficients, moved[0], moved[1]


@pytest.mark.parametrize("bits,name,word", PACKING, ids=PACKING_IDS)
def test_reply_coefficients_to_bytes(oracle, bits, name, word):
    """MulPirClient.decrypt's byte string at `bits` bits per coefficient against pir_client_reference.py (the oracle's
    coefficientsToBytes, which leaves bit `bits` of a coefficient unmasked): replies encrypted on the device over one modulus."""
    case = set_case(name, word)
    t, n, dims = case.t, case.degree, [4, 3]
    bpp = n * bits // 8
    rng = np.random.default_rng(100 + bits + word)
    aligned = unaligned = 0
    for mode in ("pack", "split"):
        entry_size = max(1, min(37, (bpp - 1) // 3 - 1)) if mode == "pack" else 2 * bpp + bpp // 3 + 1
        probe = client.plan(n, t, dims, 0, entry_size, True, 2)
        per, R = probe["entries_per_plaintext"], probe["reply_ciphertext_count"]
        assert (R, per >= 2) == ((1, True) if mode == "pack" else (3, False))
        entries = 12 * per
        p = client.plan(n, t, dims, entries, entry_size, True, 2)
        indices = [[0, entries - per]]  # position 0 of a plaintext: the whole plaintext lies behind the prefix
        sizes = [entry_size, entry_size // 2]
        built = [_reply_plaintexts(oracle, rng, p, t, indices[0][i], sizes[i]) for i in range(2)]
        plaintexts = np.stack([b[0] for b in built])
        aligned, unaligned = aligned + sum(b[1] for b in built), unaligned + sum(b[2] for b in built)
        assert (1 << bits) <= int(plaintexts.max()) < t
        flat = case.to_device(plaintexts.reshape(-1, n))
        seeds = _device_seeds(sets.seeds(2 * R, bits)), _device_seeds(sets.seeds(2 * R, bits + 50))
        cts = case.ctx.encrypt(flat, case.s_device, seeds[0], seeds[1], 1)
        assert torch.equal(case.ctx.decrypt(cts, case.s_device), flat)  # one modulus decrypts, residues above 2^bits included
        response = cts.view(1, 2, R, 2, 1, n)
        device_indices = torch.from_numpy(np.array(indices, dtype=np.int64)).cuda()
        got_entries, got_sizes = case.ctx.pir_decrypt_response(response, device_indices, dims, entries, entry_size, True, case.s_device)
        full, full_sizes = case.ctx.pir_decrypt_response(response, None, dims, entries, entry_size, True, case.s_device)
        for i in range(2):
            data = client.reply_bytes(oracle, plaintexts[i], bits)
            assert data == b"".join(client.reply_bytes_closed_form(row, bits) for row in plaintexts[i])
            assert bytes(full[0, i].cpu().numpy()) == data, (mode, i)
            assert int(full_sizes[0, i]) == len(data) == R * bpp
            entry, size = client.entry_of_reply(p, data, indices[0][i])
            assert bytes(got_entries[0, i].cpu().numpy()) == entry, (mode, i)
            assert int(got_sizes[0, i]) == size == sizes[i], (mode, i)
    assert aligned > 0 and (unaligned > 0 or bits % 8 == 0)


# ---- one MulPIR round trip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,word", sets.ROUND_TRIPS, ids=[sets.case_id(c) for c in sets.ROUND_TRIPS])
def test_mulpir_round_trip(name, word):
    """indices -> MulPirClient.generateQuery -> PirUtil.computeResponse -> MulPirClient.decrypt on the device, nothing on the host
    in between, over predefined_sets.RoundTrip's 4 x 3 database of 36 entries.  The database, the query, the keys and every
    response word are the CPU side's (pir_database_reference.py, the restatements on the same seeds, oracle/pir.py's expand and
    chunk response), and the returned entry is what pir_client_reference.py makes of the oracle's response.

    Whether that is the database's entry is a matter of the set's noise budget, not of the device: on the CPU
    (tests/test_predefined_sets.py::test_oracle_mulpir_round_trip) the oracle's own response decrypts to the queried entry for
    t = 11 on both word sizes, with some 15 bits of budget left, and does NOT for n_8192_logq_3x55_logt_42, where a database
    plaintext of 41-bit coefficients uses up the 110-bit Q.  The entry is asserted in the first case; in the second the device
    must return the same wrong bytes as the reference would."""
    case = set_case(name, word)
    trip = sets.round_trip(name, word)
    ours, n, L, dims = case.ctx, case.degree, case.L, trip.DIMENSIONS
    entry_size, entry_count = trip.entry_size, trip.ENTRY_COUNT
    database, present = ours.pir_process_database(torch.from_numpy(trip.padded).cuda(), dims, entry_size, True,
                                                  entry_sizes=trip.sizes)
    assert np.array_equal(case.to_host(database), trip.database) and np.array_equal(present.cpu().numpy(), trip.present)
    plan = ours.pir_client_plan(dims, entry_count, entry_size, True, 1)
    assert all(plan[key] == trip.plan[key] for key in plan)
    elements = ours.pir_evaluation_key_elements(plan["expanded_query_count"], "none")
    assert elements == trip.elements
    galois = ours.generate_galois_keys(case.s_device, elements, _device_seeds(trip.key_seeds[0]), _device_seeds(trip.key_seeds[1]))
    relin = ours.generate_relinearization_key(case.s_device, _device_seeds(case.chain.relin_seeds[0]),
                                              _device_seeds(case.chain.relin_seeds[1]))
    assert np.array_equal(case.to_host(galois), trip.galois) and np.array_equal(case.to_host(relin), trip.relin)
    indices = torch.from_numpy(np.array([[trip.INDEX]], dtype=np.int64)).cuda()
    query, flag = ours.pir_generate_query(indices, dims, entry_count, entry_size, True, case.s_device,
                                          _device_seeds(trip.query_seeds[0]), _device_seeds(trip.query_seeds[1]))
    assert int(flag.item()) == 0 and np.array_equal(case.to_host(query)[0], trip.query)
    galois_wide = heamd.widen_u32(galois) if word == 32 else galois  # the Galois keys are 8-byte tensors on either slab word
    response = ours.pir_compute_response_to_query(dims, query[0], 1, {e: galois_wide[k] for k, e in enumerate(elements)}, relin,
                                                  database, 1, present_devices=present)
    assert np.array_equal(case.to_host(response)[0, 0], trip.response)
    got_entries, got_sizes = ours.pir_decrypt_response(response.view(1, 1, 1, 2, 1, n), indices, dims, entry_count, entry_size,
                                                       True, case.s_device)
    got = bytes(got_entries[0, 0].cpu().numpy()), int(got_sizes[0, 0])
    assert got == (trip.returned_entry, trip.returned_size)
    assert trip.decrypts == sets.ROUND_TRIP_DECRYPTS[name]
    if trip.decrypts:
        assert got == (trip.entry, trip.size)
