"""The reference's PredefinedRlweParameters (tests/golden/predefined_parameter_sets.json) for the tests: the sets, the
messages every set is run on, the plaintext-ring model of ct x ct -> relinearize -> applyGalois in Python integers, and the
oracle's chain on keys and encryptions made from seeds (encrypt_reference.py), stage by stage, so that
tests/test_predefined_sets.py can hold the oracle to the model and tests/test_gpu_predefined_sets.py the device to both."""
import collections
import functools
import json
import os
import re

import numpy as np

import decrypt_reference
import encrypt_reference
from bfv_helpers import galois_plain

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predefined_parameter_sets.json")

ParameterSet = collections.namedtuple("ParameterSet", "name degree t moduli scalar32 error_std_dev source")


@functools.lru_cache(maxsize=None)
def load():
    with open(FIXTURE) as f:
        sets = json.load(f)["sets"]
    return tuple(ParameterSet(s["name"], s["degree"], s["plaintextModulus"], tuple(s["coefficientModuli"]),
                              s["supportsScalar32"], s["errorStdDev"], s["source"]) for s in sets)


NAMES = tuple(s.name for s in load())
BY_NAME = {s.name: s for s in load()}
# the sets whose plaintext modulus is no NTT modulus for their degree (the comment next to each enum case says so)
NTT_UNFRIENDLY = ("n_4096_logq_16_33_33_logt_4", "n_4096_logq_27_28_28_logt_13", "n_4096_logq_27_28_28_logt_4",
                  "n_4096_logq_27_28_28_logt_5", "n_4096_logq_27_28_28_logt_6", "n_8192_logq_29_60_60_logt_15")
# (set, slab word): 8-byte words for every set, packed 4-byte words where the set supports Bfv<UInt32>
CASES = tuple((s.name, word) for s in load() for word in ((64, 32) if s.scalar32 else (64,)))
GALOIS_ELEMENT = 3


def case_id(case):
    return "%s-u%d" % case


def is_prime(n):
    """deterministic Miller-Rabin below 2^64"""
    if n < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in small:
        if n % p == 0:
            return n == p
    d, r = n - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in small:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def is_ntt_modulus(modulus, degree):
    return is_prime(modulus) and modulus % (2 * degree) == 1


def name_fields(name):
    """`n_8192_logq_3x55_logt_42` -> (8192, [55, 55, 55], 42)"""
    match = re.match(r"(?:insecure_)?n_(\d+)_logq_([0-9x_]+)_logt_(\d+)$", name)
    bits = []
    for part in match.group(2).split("_"):
        count, _, width = part.rpartition("x")
        bits += [int(width)] * (int(count) if count else 1)
    return int(match.group(1)), bits, int(match.group(3))


def packing_classes():
    """floor(log2 t) -> the smallest-degree set that packs that many bits per coefficient"""
    out = {}
    for s in sorted(load(), key=lambda s: (s.degree, s.name)):
        out.setdefault(s.t.bit_length() - 1, s)
    return out


# ---- messages and the plaintext-ring model ------------------------------------------------------------------------------------
def messages(pset):
    """(A, B, terms): A dense, uniform mod t behind the words 0, t - 1, (t + 1) / 2, (t + 1) / 2 - 1; B of eight terms
    (position, coefficient) with coefficients from {1, t - 1, random}, the first and the last position among them."""
    n, t = pset.degree, pset.t
    rng = np.random.default_rng(n + t % 1000003)
    a = [int(v) for v in rng.integers(0, t, n)]
    a[:4] = [0, t - 1, (t + 1) // 2, (t + 1) // 2 - 1]
    positions = [0, n - 1] + sorted(int(p) for p in rng.choice(np.arange(1, n - 1), 6, replace=False))
    kinds = [1, t - 1, None, 1, t - 1, None, None, t - 1]
    terms = [(p, int(rng.integers(0, t)) if c is None else c) for p, c in zip(positions, kinds)]
    b = [0] * n
    for p, c in terms:
        b[p] = c
    return a, b, terms


def sparse_negacyclic_product(a, terms, t):
    """a(x) sum_j c_j x^(p_j) in Z_t[x] / (x^N + 1): len(terms) N multiply-adds on Python integers"""
    n = len(a)
    dense = np.array(a, dtype=object)
    total = np.zeros(n, dtype=object)
    for p, c in terms:
        total = total + np.concatenate([-dense[n - p:], dense[:n - p]]) * c
    return [int(v) % t for v in total]


def product_model(pset):
    a, _, terms = messages(pset)
    return sparse_negacyclic_product(a, terms, pset.t)


def chain_model(pset):
    """what mul -> relinearize -> applyGalois(3) -> modSwitchDownToSingle must decrypt to"""
    return galois_plain(product_model(pset), GALOIS_ELEMENT, pset.t)


# ---- the oracle's chain on seeded keys and encryptions --------------------------------------------------------------------------
def seeds(count, salt):
    return np.random.default_rng(7000 + salt).integers(0, 256, (count, 32), dtype=np.uint8)


class Chain:
    """One set on one word size on the CPU oracle: secret key, encryptions at every moduli count, evaluation keys, and where the
    set has a key-switching modulus mul -> relinearize -> applyGalois -> modSwitchDown .. -> one modulus, every stage kept."""

    def __init__(self, oracle, pset, word):
        self.oracle, self.pset, self.word = oracle, pset, word
        n, t = pset.degree, pset.t
        # contexts, stream, key and client: the same object the device test's case is built beside
        self.host = host = encrypt_reference.HostSide(oracle, n, t, pset.moduli, word, seeds(3, n + word))
        self.ref, self.stream, self.secret_ctx, self.client = host.ref_ctx, host.stream, host.secret_ctx, host.client
        self.key_seeds, self.s_eval = host.key_seeds, host.s_eval
        self.L, self.L_all = self.ref.L, host.L_all
        a, b, _ = messages(pset)
        self.messages = np.array([a, b, [t - 1] * n], dtype=np.uint64)
        self.a_seeds, self.error_seeds = seeds(3, 1), seeds(3, 2)
        self.elements = [GALOIS_ELEMENT, 2 * n - 1]
        self.relin_seeds = (seeds(self.L, 3), seeds(self.L, 4))
        self.galois_seeds = (seeds(2 * self.L, 5).reshape(2, self.L, 32), seeds(2 * self.L, 6).reshape(2, self.L, 32))

    def prefix_ctx(self, m):
        return self.oracle.PolyContext(self.pset.degree, list(self.pset.moduli[:m]))

    def moduli(self, m):
        return [int(q) for q in self.pset.moduli[:m]]

    @functools.lru_cache(maxsize=None)
    def fresh(self, m):
        """[3][2][m][N]: the three messages encrypted over the first m moduli"""
        return np.stack([encrypt_reference.encrypt(self.prefix_ctx(m), self.pset.t, self.messages[b], self.s_eval,
                                                   bytes(self.a_seeds[b]), bytes(self.error_seeds[b]), self.stream)
                         for b in range(3)])

    def _key(self, current, a, e):
        return encrypt_reference.key_switch_key(self.prefix_ctx(self.L_all), self.s_eval, current, [bytes(s) for s in a],
                                                [bytes(s) for s in e], self.stream)

    @functools.lru_cache(maxsize=None)
    def relinearization_key(self):
        current = encrypt_reference.relinearization_current_key(self.secret_ctx, self.s_eval)
        return self._key(current, *self.relin_seeds)

    @functools.lru_cache(maxsize=None)
    def galois_keys(self):
        """[2][L][2][L + 1][N]: the keys of elements 3 and 2N - 1"""
        return np.stack([self._key(encrypt_reference.galois_current_key(self.secret_ctx, self.s_eval, element),
                                   self.galois_seeds[0][k], self.galois_seeds[1][k]) for k, element in enumerate(self.elements)])

    @functools.lru_cache(maxsize=None)
    def stages(self):
        """name -> ciphertext [1][polys][m][N] Coeff, in the order the chain runs"""
        top = self.fresh(self.L)
        out = collections.OrderedDict()
        out["mul"] = self.ref.mul(top[:1], top[1:2])
        if self.L_all == 1:  # one modulus: no key-switching modulus, no evaluation keys, nothing to switch down to
            return out
        out["relinearize"] = self.ref.relinearize(out["mul"], self.relinearization_key())
        out["apply_galois"] = self.ref.apply_galois(out["relinearize"], GALOIS_ELEMENT, self.galois_keys()[0])
        current = out["apply_galois"]
        for level in range(self.L, 1, -1):
            current = self.ref.mod_switch_down(current, 2, level)
            out["mod_switch_down_%d" % level] = current
        out["single"] = current
        return out

    def dot(self, ct):
        """c0 + c1 s (+ c2 s^2) of one ciphertext [polys][m][N] -> [m][N] Coeff"""
        return decrypt_reference.dot_product(self.prefix_ctx(ct.shape[1]), ct, self.s_eval)

    def noise_norm(self, ct):
        return decrypt_reference.noise_norm(self.dot(ct), self.moduli(ct.shape[1]), self.pset.t)

    def noise_budget(self, ct):
        return decrypt_reference.noise_budget(self.noise_norm(ct), self.moduli(ct.shape[1]))

    def decrypt_exact(self, ct):
        return self.client.decrypt_exact(ct, ct.shape[1])

    def decrypt(self, ct):
        return self.client.decrypt(ct, ct.shape[1])


class RoundTrip:
    """One MulPIR round trip on the CPU: a 4 x 3 database of 36 entries, three to a plaintext (a two-byte size prefix), one
    index; query and keys by the restatements from seeds, the response by oracle/pir.py, the entry by pir_client_reference.py."""

    DIMENSIONS, ENTRY_COUNT, INDEX, INPUTS = [4, 3], 36, 22, 7  # entry 22: plaintext 7, position 1

    def __init__(self, chain):
        import pir_client_reference as client
        import pir_database_reference as refdb

        oracle, pset, L = chain.oracle, chain.pset, chain.L
        n, t, dims = pset.degree, pset.t, self.DIMENSIONS
        self.entry_size = n * (t.bit_length() - 1) // 8 // 3 - 2
        rng = np.random.default_rng(n + t.bit_length())
        self.entries, self.padded, self.sizes = refdb.varying_entries(rng, self.ENTRY_COUNT, self.entry_size)
        self.database, self.present = refdb.process(oracle, chain.ref, self.entries, dims, self.entry_size, True)
        self.plan = client.plan(n, t, dims, self.ENTRY_COUNT, self.entry_size, True, 1)
        self.elements = client.evaluation_key_elements(self.INPUTS, n, "none")
        count = len(self.elements)
        self.key_seeds = (seeds(count * L, 20).reshape(count, L, 32), seeds(count * L, 21).reshape(count, L, 32))
        self.galois = np.stack([chain._key(encrypt_reference.galois_current_key(chain.secret_ctx, chain.s_eval, element),
                                           self.key_seeds[0][k], self.key_seeds[1][k]) for k, element in enumerate(self.elements)])
        self.relin = chain.relinearization_key()
        self.query_seeds = (seeds(1, 22), seeds(1, 23))
        self.query = client.generate_query(chain.prefix_ctx(L), t, self.plan, [self.INDEX], chain.s_eval,
                                           [bytes(self.query_seeds[0][0])], [bytes(self.query_seeds[1][0])], chain.stream)
        expanded = oracle.pir.expand(chain.ref, self.query, self.INPUTS, {e: self.galois[k] for k, e in enumerate(self.elements)})
        qctx = chain.ref.ciphertext_context()
        dim0 = np.stack([qctx.forward_ntt(ct) for ct in expanded[:dims[0]]])
        self.response = oracle.pir.compute_response_for_one_chunk(chain.ref, dims, dim0, expanded[dims[0]:], self.database[0],
                                                                  self.present[0], self.relin)  # [2][1][N]
        (self.returned_entry, self.returned_size), = client.decrypt_response(
            oracle, chain.prefix_ctx(1), t, self.plan, self.response[None, None], [self.INDEX], chain.s_eval)
        entry = self.entries[self.INDEX]
        self.entry, self.size = entry + bytes(self.entry_size - len(entry)), len(entry)
        self.decrypts = (self.returned_entry, self.returned_size) == (self.entry, self.size)
        self.budget = chain.noise_budget(self.response)


# (set, slab word) of the round trips, and whether the ORACLE's own response decrypts to the queried entry: a matter of the
# set's noise budget (tests/test_predefined_sets.py measures it), not of the device
ROUND_TRIPS = (("n_4096_logq_27_28_28_logt_4", 64), ("n_4096_logq_27_28_28_logt_4", 32), ("n_8192_logq_3x55_logt_42", 64))
ROUND_TRIP_DECRYPTS = {"n_4096_logq_27_28_28_logt_4": True, "n_8192_logq_3x55_logt_42": False}


@functools.lru_cache(maxsize=None)
def round_trip(name, word):
    return RoundTrip(chain(name, word))


@functools.lru_cache(maxsize=None)
def chain(name, word):
    import oracle

    oracle.build()
    return Chain(oracle, BY_NAME[name], word)
