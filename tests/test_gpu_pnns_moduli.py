"""pnns_bsgs_inner_product_kernel at the moduli, words and baby steps tests/test_gpu_pnns_response.py does not reach: the wide
8-byte form (a modulus of 2^56 or more) for one to four queries, the fold inside an item on both word sizes and in the general
form, and sums at their bound -- every term (q_i - 1)^2 -- so that a cadence one too long, a fold that restarts from the wrong
word or a term count carried across an item boundary changes a word.  Then the database build at the same moduli.

Every comparison is word for word against tests/pnns_reference.py's mulTranspose(vector:) over the oracle and the oracle's
modSwitchDown chain (tests/test_gpu_pnns_response.py expected_words), or its diagonal_matrix.  Each response case runs with
uniform words and with the worst-case words of tests/pnns_extremes.py, asserts first -- from the launcher's dispatch restated
there -- that its shape takes the form and crosses the number of folds its id names, and in the worst-case run that the rotated
rows the restatement computes are q_i - 1 in every slot of polynomial 0.  No mismatch was found when these were added; a
library built with the in-loop fold disabled fails the 32-, 64- and 128-term cases and both N = 64 ones."""
from collections import namedtuple

import numpy as np
import pytest

import heamd
import pnns_extremes as extremes
import pnns_reference as pnns
from bfv_helpers import BfvClient
from test_gpu_pnns import Setup, check_matrix
from test_gpu_pnns_response import device_keys, expected_words, to_device

pytestmark = pytest.mark.gpu

_setups = {}


def get_setup(oracle, degree, bits, t_bits=17, word32=False):
    key = (degree, tuple(bits), t_bits, word32)
    if key not in _setups:
        t = oracle.generate_primes([t_bits], True, degree)[0]
        q = oracle.generate_primes(list(bits), False, degree, word_bits=32 if word32 else 64)
        assert len(set(q)) == len(q) and [m.bit_length() for m in q] == list(bits)
        _setups[key] = Setup(oracle, degree, word32, t=t, q=q)
    return _setups[key]


# form: the kernel form every pass takes (pnns_extremes.kernel_form); passes: queries per launch; folds: folds taken inside the
# longest item's sum (0: the case is about something else, named in its id)
Case = namedtuple("Case", "id degree bits word32 rows cols baby_step queries form passes folds")

CASES = [
    # N = 1024, L = 3, 62-bit: P = 128, b = 16, G = 8, C = 2; cadence 8 inside each 16-term item; QN = 4 is the 256-lane form
    Case("wide-QN1-fold8of16", 1024, (62, 62, 62, 62), False, 1025, 100, 16, 1, "wide", [1], 1),
    Case("wide-QN2-fold8of16", 1024, (62, 62, 62, 62), False, 1025, 100, 16, 2, "wide", [2], 1),
    Case("wide-QN3-fold8of16", 1024, (62, 62, 62, 62), False, 1025, 100, 16, 3, "wide", [3], 1),
    Case("wide-QN4-fold8of16", 1024, (62, 62, 62, 62), False, 1025, 100, 16, 4, "wide", [4], 1),
    # b = 12, G = 11: ten items of 12 terms (a fold at 8) and then the ragged one of 8 (none); passes of 4 + 1 queries
    Case("wide-ragged-QN4+1-fold8of12", 1024, (62, 62, 62, 62), False, 1024, 100, 12, 5, "wide", [4, 1], 1),
    # beyond the table: 16 terms of (q - 1)^2 still fit 128 bits, so a fold left out there changes no word; 32 and 64 terms
    # (P = 512, G = 16 and 8) wrap without the folds at every 8th term.  The tile allows two queries at b = 32, one at 64
    Case("wide-QN2-fold8x3of32", 1024, (62, 62, 62, 62), False, 1024, 300, 32, 2, "wide", [2], 3),
    Case("wide-QN1-fold8x7of64", 1024, (62, 62, 62, 62), False, 1024, 300, 64, 1, "wide", [1], 7),
    # the cadence is the minimum over the rows (8, from the 62-bit one); the 45-bit row uses the wide sums too; C = 3
    Case("wide-mixed-62-45-61-QN3-fold8of16", 1024, (62, 45, 61, 62), False, 2049, 100, 16, 3, "wide", [3], 1),
    Case("wide-just-over-2^56-QN2-nofold", 1024, (57, 56, 57, 58), False, 1024, 100, 16, 2, "wide", [2], 0),
    # P = 512, b = 64, G = 8: the narrow sums at their stated limit of 64 worst-case terms; the tile allows one query a pass
    Case("narrow-64of64-QN1+1", 1024, (56, 55, 56, 57), False, 1024, 300, 64, 2, "narrow", [1, 1], 0),
    # G = 1 and a tile beyond LDS: 128-bit sums folded on the reference's own count, 16, seven times inside the item
    Case("general-b128-fold16x7", 1024, (62, 62, 62, 62), False, 1024, 100, 128, 2, "general", [1, 1], 7),
    Case("general-N64-fold16of32", 64, (62, 61, 62, 62), False, 65, 30, 32, 2, "general", [1, 1], 1),
    # L = 4 at a tiled degree, G = 1: the key of -b is not read (device_keys passes None)
    Case("wide-N4096-L4-QN4-fold8of16", 4096, (62, 60, 58, 62, 62), False, 4097, 16, 16, 4, "wide", [4], 1),
    # 4-byte words: 64-bit sums of 15 x (< 2^60); the fold at 15 is one term from the item's end
    Case("u32-fast-QN1-fold15of16", 1024, (30, 30, 30, 30), True, 1025, 100, 16, 1, "fast", [1], 1),
    Case("u32-fast-QN4-fold15of16", 1024, (30, 30, 30, 30), True, 1025, 100, 16, 4, "fast", [4], 1),
    Case("u32-fast-QN2+1-fold15,30of32", 1024, (30, 30, 30, 30), True, 1024, 300, 32, 3, "fast", [2, 1], 2),
    Case("u32-general-N64-fold15,30of32", 64, (30, 29, 30, 30), True, 65, 30, 32, 2, "general", [1, 1], 2),
]


def first_difference(got, expected):
    """(query, result, polynomial, modulus row, slot) of the first differing word, for the failure's label."""
    where = np.argwhere(got != expected)
    return tuple(int(v) for v in where[0]) if where.size else None


@pytest.mark.parametrize("mode", ["uniform", "worst"])
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_response_words(oracle, case, mode):
    """Every baby step of the table is admissible under pnns.baby_step_giant_step(cols, b), so the shapes are the table's."""
    s = get_setup(oracle, case.degree, case.bits, word32=case.word32)
    n, L, b, queries = s.degree, s.ref.L, case.baby_step, case.queries
    assert L == len(case.bits) - 1
    moduli, word_bytes = list(s.q[:L]), 4 if case.word32 else 8
    padded, results = pnns.next_power_of_two(case.cols), -(-case.rows // n)
    assert results <= 3
    giant_step = pnns.baby_step_giant_step(case.cols, b)[1]
    assert s.pnns.matrix_shape(case.rows, case.cols, "diagonal", b) == {
        "plaintext_count": padded * results, "baby_step": b, "giant_step": giant_step}

    # the case reaches what its id says
    per_pass = extremes.queries_per_pass(n, L, b, queries, word_bytes)
    assert [min(per_pass, queries - first) for first in range(0, queries, per_pass)] == case.passes
    longest = min(b, padded)
    for taken in case.passes:
        form, cadence = extremes.kernel_form(n, moduli, b, taken, word_bytes)
        assert form == case.form, (form, cadence)
        assert extremes.in_loop_folds(longest, cadence) == case.folds, (longest, cadence)
        if case.folds:
            assert cadence < longest
        if case.form == "narrow":
            assert cadence == longest == extremes.NARROW_CADENCE
    if padded % b:  # ragged: the last item is shorter
        assert 0 < padded - b * (giant_step - 1) < b

    rng = np.random.default_rng(7919 * CASES.index(case) + (mode == "worst"))
    if mode == "worst":
        query, keys = extremes.worst_case_query(rng, moduli, s.q[-1], n, queries)
        matrix = extremes.worst_case_matrix(rng, moduli, n, padded, results, b)
        element = heamd.galois_element_rotating_columns(-1, n)
        for k in range(queries):
            assert extremes.is_worst_case(extremes.rotated_rows(s.ref, query[k], keys[k][0], element, b), moduli), k
    else:
        query = extremes.uniform_words(rng, moduli, (queries, 2), n)
        keys = [[extremes.uniform_words(rng, moduli + [s.q[-1]], (L, 2), n) for _ in range(2)] for _ in range(queries)]
        matrix = extremes.uniform_words(rng, moduli, (padded * results,), n)

    device_matrix, device_query = to_device(s, matrix), to_device(s, query)
    galois = device_keys(s, keys, b, giant_step)
    got_full = s.to_host(s.pnns.mul_transpose(device_matrix, case.rows, case.cols, device_query, galois, baby_step=b))
    got_single = s.to_host(s.pnns.compute_response(device_matrix, case.rows, case.cols, device_query, galois, baby_step=b))
    full, single = expected_words(s, matrix, case.rows, case.cols, b, query, keys)
    assert got_full.shape == full.shape == (queries, results, 2, L, n)
    assert got_single.shape == single.shape == (queries, results, 2, 1, n)
    assert full.any() and single.any()
    assert np.array_equal(got_full, full), (case.id, mode, first_difference(got_full, full))
    assert np.array_equal(got_single, single), (case.id, mode, first_difference(got_single, single))


# ---- the database build at the same moduli ------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_bits", [17, 30])
@pytest.mark.parametrize("bits", [(62, 45, 61, 58, 62), (57, 56, 57, 58)], ids=["62-45-61-58", "57-56-57"])
@pytest.mark.parametrize("degree", [64, 1024])
def test_diagonal_matrix_at_wide_and_mixed_moduli(oracle, degree, bits, t_bits):
    """The pack kernel, the inverse NTT over t and the forward NTT over q at moduli above 55 bits, of mixed sizes, and at a
    30-bit plaintext modulus; signed_values carries its edge list (the ends of the centred range, or +-t with reduce)."""
    s = get_setup(oracle, degree, bits, t_bits=t_bits)
    assert s.t.bit_length() == t_bits and s.ref.L == len(bits) - 1
    rng = np.random.default_rng(degree + t_bits + len(bits))
    for rows, cols in ((1, 1), (degree + 1, 5), (3 * degree + 5, 100 if degree > 64 else 30)):
        for reduce in (False, True):
            for moduli_count in (None, 1):
                check_matrix(s, rng, rows, cols, None, reduce, moduli_count)


def test_decrypted_response_at_62_bit_moduli(oracle):
    """tests/test_gpu_pnns_response.py's decryption test on the 62, 61, 62-bit set: real ciphertexts and Galois keys through
    the device-built matrix (150 x 30 at N = 64: C = 3, P = 32, b = 6, G = 6, the last giant step sums 2) and the response."""
    import torch

    degree, rows, cols = 64, 150, 30
    s = get_setup(oracle, degree, (62, 61, 62, 62))
    t = s.t
    rng = np.random.default_rng(62)
    bound = 40
    data = rng.integers(-bound, bound + 1, size=(rows, cols))
    baby_step, giant_step = pnns.baby_step_giant_step(cols)
    assert (baby_step, giant_step) == (6, 6)
    matrix, flag = s.pnns.diagonal_matrix(torch.from_numpy(data.astype(np.int64)).cuda())
    assert int(flag.item()) == 0
    clients = [BfvClient(oracle, s.ref, seed=620 + k) for k in range(2)]
    vectors = [rng.integers(-bound, bound + 1, size=cols) for _ in clients]
    queries, keys = [], []
    for client, vector in zip(clients, vectors):
        slots = pnns.dense_row_vector_slots(np.mod(vector, t), degree)
        queries.append(client.encrypt([int(v) for v in s.encoder.encode(slots)[0]]))
        keys.append((heamd.to_device(client.galois_key(heamd.galois_element_rotating_columns(-1, degree))),
                     heamd.to_device(client.galois_key(heamd.galois_element_rotating_columns(-baby_step, degree)))))
    device_query = heamd.to_device(np.stack(queries))
    full = heamd.to_host(s.pnns.mul_transpose(matrix, rows, cols, device_query, keys))
    single = heamd.to_host(s.pnns.compute_response(matrix, rows, cols, device_query, keys))
    for k, (client, vector) in enumerate(zip(clients, vectors)):
        product = np.mod(data @ vector, t).astype(np.uint64)
        for result, moduli_count in ((full[k], None), (single[k], 1)):
            decoded = np.concatenate([s.encoder.decode(np.array(client.decrypt(ct, moduli_count), dtype=np.uint64))[0]
                                      for ct in result])
            assert np.array_equal(decoded[:rows], product), (k, moduli_count)
