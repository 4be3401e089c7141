"""Decryption of resident ciphertexts on the device (he_bfv_secret_dot_product_device, he_bfv_decrypt_device,
he_bfv_noise_norm_device, he_bfv_is_transparent_device), on both slab words wherever the moduli fit:

  * dot product and plaintexts word for word against the oracle composition bfv_helpers.BfvClient.decrypt spells out, and
    against decrypt_exact for the real ciphertexts -- Coeff and Eval input, 1, 2 and 3 polynomials (3: an unrelinearized
    product), every level L .. 1, a secret key with more rows than the level uses;
  * the noise norm as an exact integer against tests/decrypt_reference.py, on constructed ciphertexts whose composed value is
    chosen (decrypt_reference.transparent_ciphertext) and on fresh, multiplied and mod-switched real ones.  The largest limb
    count reached is 13 (w64_50x16: Q of 16 x 50 bits);
  * transparency, one small MulPIR response decrypted end to end, errors and no-ops.

Every case builds its ciphertexts and their expected values once (module-scoped fixture)."""
import ctypes
import math
import random

import numpy as np
import pytest

import decrypt_reference as ref
import heamd
import word32_cases
from bfv_helpers import BfvClient

pytestmark = pytest.mark.gpu

# name: (degree, bits of the ciphertext moduli, preferring_small, batch, bits of t, slab words)
SHAPES = {
    "n8_q20": (8, [20], False, 3, 5, (64, 32)),  # fewer coefficients than a wavefront, one modulus, no key-switching modulus
    "n64_q40_41": (64, [40, 41], False, 3, 17, (64,)),
    "n16_q32_32": (16, [32, 32], False, 2, 17, (64,)),  # Q just below 2^64: one limb
    "n16_q33_33": (16, [33, 33], True, 2, 17, (64,)),  # Q just above 2^64: two limbs
    "n256_q43_43_42": (256, [43, 43, 42], False, 2, 17, (64,)),  # N = the workgroup's lanes; Q just below 2^128
    "n256_q44_44_43": (256, [44, 44, 43], True, 2, 17, (64,)),  # Q a little over 2^128: three limbs
    "n4096_q27_28_28": (4096, [27, 28, 28], False, 2, 17, (64, 32)),
    "n8192_q55x4": (8192, [55] * 4, False, 3, 20, (64,)),
}
MANY_MODULI = ("w64_50x16", "w32_26x16")  # word32_cases.many_moduli_set, N = 4096, batch 2
CASES = [(name, word) for name, shape in SHAPES.items() for word in shape[5]] + [("w64_50x16", 64), ("w32_26x16", 32)]


def _to_device(array, word):
    return heamd.to_device32(array) if word == 32 else heamd.to_device(array)


def _to_host(tensor, word):
    return heamd.to_host32(tensor) if word == 32 else heamd.to_host(tensor)


class Case:
    """One parameter set on one slab word: the contexts, a client, and per level k = L .. 1 the Coeff ciphertexts
    cts[polys][k] = [batch][polys][k][N] -- item 0 real (fresh at the top level, mod-switched below; polys 3: the product of
    two fresh ones, polys 1: c0 alone), the others uniform words -- with their oracle dot products."""

    def __init__(self, oracle, name, word):
        self.name, self.word = name, word
        if name in MANY_MODULI:
            word_bits, t, q = word32_cases.many_moduli_set(oracle, name)
            assert word_bits == word
            degree, batch = word32_cases.MANY_MODULI_DEGREE, 2
        else:
            degree, bits, small, batch, t_bits, _ = SHAPES[name]
            t = oracle.generate_primes([t_bits], True, degree)[0]
            q = oracle.generate_primes(bits + (bits[-1:] if len(bits) > 1 else []), small, degree, word_bits=word)
        self.degree, self.t, self.batch = degree, t, batch
        self.ours = (heamd.BfvContext32 if word == 32 else heamd.BfvContext)(degree, t, q)
        self.ref = oracle.BfvContext(degree, t, q, word_bits=word)
        self.client = BfvClient(oracle, self.ref, seed=len(name) + word)
        self.L = self.ref.L
        self.key = _to_device(self.client.s_eval_all, word)  # every coefficient modulus: more rows than any level uses
        rng = random.Random(degree + word)
        nprng = np.random.default_rng(degree + word)
        self.messages = [[rng.randrange(t) for _ in range(degree)] for _ in range(2)]
        fresh = [self.client.encrypt(m) for m in self.messages]
        product = self.ref.mul(fresh[0][None], fresh[1][None])[0]
        self.cts = {1: {}, 2: {}, 3: {}}
        real = {2: fresh[0], 3: product}
        for k in range(self.L, 0, -1):
            moduli = self.moduli(k)
            for polys in (2, 3):
                if k < self.L:
                    real[polys] = self.ref.mod_switch_down(real[polys][None], polys, moduli_count=k + 1)[0]
                uniform = np.stack([nprng.integers(0, m, size=(batch - 1, polys, degree), dtype=np.uint64) for m in moduli], axis=2)
                self.cts[polys][k] = np.ascontiguousarray(np.concatenate([real[polys][None], uniform]))
            self.cts[1][k] = np.ascontiguousarray(self.cts[2][k][:, :1])
        self._dots = {}

    def moduli(self, k):
        return [int(m) for m in self.ref.ciphertext_context(k).moduli]

    def oracle_dot(self, polys, k):
        """[batch][k][N] Coeff by the composition BfvClient.decrypt spells out"""
        if (polys, k) not in self._dots:
            qctx = self.ref.ciphertext_context(k)
            s = self.client.s_eval_all[:k]
            out = []
            for ct in self.cts[polys][k]:
                ct_eval = qctx.forward_ntt(ct)
                dot, power = ct_eval[0].copy(), s.copy()
                for index in range(1, polys):
                    dot = qctx.add(dot, qctx.mul(ct_eval[index], power))
                    power = qctx.mul(power, s)
                out.append(qctx.inverse_ntt(dot))
            self._dots[(polys, k)] = np.stack(out)
        return self._dots[(polys, k)]

    def device(self, array):
        return _to_device(array, self.word)

    def host(self, tensor):
        return _to_host(tensor, self.word)


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def case(oracle, request):
    return Case(oracle, *request.param)


def test_dot_product_and_plaintexts_match_the_oracle(case):
    t = case.t
    other = 5 % t if 5 % t not in (0, 1) else 2
    for k in range(case.L, 0, -1):
        qctx, tool = case.ref.ciphertext_context(k), case.ref.rns_tool(k)
        ends = k in (case.L, 1)  # every level takes both forms of two polynomials; the top and the bottom one everything
        for polys in (1, 2, 3) if ends else (2,):
            coeff = case.cts[polys][k]
            expected_dot = case.oracle_dot(polys, k)
            for eval_format in (False, True):
                cts = case.device(qctx.forward_ntt(coeff) if eval_format else coeff)
                before = cts.clone()
                got = case.host(case.ours.secret_dot_product(cts, case.key, eval_format))
                assert np.array_equal(got, expected_dot), (k, polys, eval_format)
                for factor in (1, other) if ends else (1,):
                    plain = case.host(case.ours.decrypt(cts, case.key, factor, eval_format))
                    scaling = pow(factor, -1, t)
                    expected = np.stack([tool.scale_and_round(dot, scaling) for dot in expected_dot])
                    assert np.array_equal(plain, expected), (k, polys, eval_format, factor)
                assert bool((cts == before).all())  # the caller's slab is const
    # the real ciphertexts decrypt as the exact client says, and the fresh one to its message
    for k in sorted({case.L, 1}):
        for polys in (2, 3):
            plain = case.host(case.ours.decrypt(case.device(case.cts[polys][k][:1]), case.key))[0]
            assert [int(v) for v in plain] == case.client.decrypt_exact(case.cts[polys][k][0], k), (k, polys)
    plain = case.host(case.ours.decrypt(case.device(case.cts[2][case.L][:1]), case.key))[0]
    assert [int(v) for v in plain] == case.messages[0]


def test_a_product_decrypts_to_the_product_of_its_messages(oracle):
    """3 polynomials, semantically: an unrelinearized ct x ct at N = 64 with budget to spare"""
    from bfv_helpers import negacyclic_multiply

    case = Case(oracle, "n64_q40_41", 64)
    plain = case.host(case.ours.decrypt(case.device(case.cts[3][case.L][:1]), case.key))[0]
    assert [int(v) for v in plain] == negacyclic_multiply(case.messages[0], case.messages[1], case.t)
    assert case.ours.noise_budget(case.device(case.cts[3][case.L][:1]), case.key)[0] > 0


def test_slabs_off_a_16_byte_boundary_take_the_one_word_path(case):
    """a ciphertext slab and a key that start one word behind a 16-byte boundary"""
    import torch

    k = case.L

    def shifted(array):
        tensor = case.device(array)
        holder = torch.zeros(tensor.numel() + 1, dtype=tensor.dtype, device=tensor.device)
        holder[1:] = tensor.reshape(-1)
        view = holder[1:].reshape(tensor.shape)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        return view

    key = shifted(case.client.s_eval_all)
    qctx = case.ref.ciphertext_context(k)
    for polys in (2, 3):
        for eval_format in (False, True):
            cts = shifted(qctx.forward_ntt(case.cts[polys][k]) if eval_format else case.cts[polys][k])
            got = case.host(case.ours.secret_dot_product(cts, key, eval_format))
            assert np.array_equal(got, case.oracle_dot(polys, k)), (polys, eval_format)
        flags = case.ours.is_transparent(shifted(case.cts[polys][k])).cpu().tolist()
        assert flags == [0] * case.batch


def _budgets_agree(got, expected):
    assert len(got) == len(expected)
    for a, b in zip(got, expected):
        assert a == b or abs(a - b) <= math.ulp(b), (a, b)


def test_noise_norm_of_constructed_ciphertexts(case):
    """composed values at the centring's decision points, the maximum in every position that takes another way through the
    reduction, ties, and all zero -- exact integer equality with the restatement"""
    n, word = case.degree, case.word
    for k in sorted({case.L, (case.L + 1) // 2, 1}):
        moduli = case.moduli(k)
        q = ref.product(moduli)
        half = (q + 1) >> 1
        edge = [0, 1, half - 1, half, half + 1, q - 1]
        items = [{0: w} for w in edge] + [{n - 1: w} for w in edge]
        positions = sorted({0, n - 1} | {p for p in (63, 64, 127, 128, 191, 192, 255, 256, n // 2 + 65, n - 64) if 0 <= p < n})
        for p in positions:  # the maximum alone in one lane of one wavefront, smaller values everywhere else
            values = {c: half - 3 - c for c in range(min(n, 300))}
            values.update({n - 1 - c: half + 3 + c for c in range(min(n // 2, 40))})  # (centred: half - 4 - c)
            values[p] = half - 1
            items.append(values)
        items.append({0: half - 2, n - 1: half + 2, n // 2: half - 2})  # ties, from both sides of the centring
        items.append({})  # all zero
        cts = np.stack([ref.transparent_ciphertext(values, n, moduli, case.t) for values in items])
        expected = [ref.noise_norm(ct[0], moduli, case.t) for ct in cts]
        # (the restatement on the construction gives what the construction says)
        assert expected[:6] == [0, 1, half - 1, half, half - 2, 1] and expected[-2:] == [half - 2, 0]
        assert all(e == half - 1 for e in expected[12:12 + len(positions)])
        device_cts = _to_device(cts, word)
        assert case.ours.noise_norm(device_cts, case.key) == expected, k
        assert case.ours.noise_norm(_to_device(case.ref.ciphertext_context(k).forward_ntt(cts), word), case.key, True) == expected
        budgets = case.ours.noise_budget(device_cts, case.key)
        _budgets_agree(budgets, [ref.noise_budget(e, moduli) for e in expected])
        assert budgets[-1] == math.inf and budgets[0] == math.inf
        assert case.ours.noise_norm_limbs(k) == (q.bit_length() + 63) // 64
        assert case.ours.is_transparent(device_cts).cpu().tolist() == [1] * len(items)
    if case.name == "w64_50x16":
        assert case.ours.noise_norm_limbs() == 13  # the largest limb count any case reaches


def test_noise_norm_of_real_ciphertexts(case):
    """fresh (polys 2, top level), multiplied (polys 3) and mod-switched (the levels below) ciphertexts, and uniform words"""
    for k in sorted({case.L, max(case.L - 1, 1), 1}):
        moduli = case.moduli(k)
        qctx = case.ref.ciphertext_context(k)
        for polys in (1, 2, 3):
            cts = case.cts[polys][k][:2]  # the real one and one of uniform words
            dots = [ref.dot_product(qctx, ct, case.client.s_eval_all) for ct in cts]
            assert all(np.array_equal(d, o) for d, o in zip(dots, case.oracle_dot(polys, k)))
            expected = [ref.noise_norm(dot, moduli, case.t) for dot in dots]
            assert case.ours.noise_norm(case.device(cts), case.key) == expected, (k, polys)
            budgets = case.ours.noise_budget(case.device(cts), case.key)
            _budgets_agree(budgets, [ref.noise_budget(e, moduli) for e in expected])
            if polys == 2 and k == case.L:
                assert budgets[0] > 0, budgets[0]  # a fresh ciphertext has budget to spare


def test_transparency(case):
    n, k = case.degree, case.L
    for polys in (1, 2, 3):
        real = case.cts[polys][k][0]
        zero_tail = real.copy()
        zero_tail[1:] = 0
        last_word = zero_tail.copy()
        if polys > 1:
            last_word[polys - 1, k - 1, n - 1] = 1
        first_word = zero_tail.copy()
        if polys > 1:
            first_word[1, 0, 0] = 1
        batch = np.stack([zero_tail, last_word, real, first_word, np.zeros_like(real)])
        flags = case.ours.is_transparent(case.device(batch)).cpu().tolist()
        assert flags == [int(ref.is_transparent(ct)) for ct in batch]
        assert flags == ([1] * 5 if polys == 1 else [1, 0, 0, 0, 1])


def test_a_pir_response_decrypts_on_the_device(oracle):
    """one small MulPIR response built with the existing entries (shapes of test_gpu_pir.py), decrypted and measured on the
    device: the plaintext is the database entry, the budget is positive and the restatement's"""
    degree = 64
    t = oracle.generate_primes([17], True, degree)[0]
    q = oracle.generate_primes([40, 40, 40, 41], False, degree)
    orc = oracle.BfvContext(degree, t, q)
    ours, client = heamd.BfvContext(degree, t, q), BfvClient(oracle, orc, seed=60)
    dims, rng = [4, 3], random.Random(63)
    total = dims[0] * dims[1]
    entries = [[rng.randrange(t) for _ in range(degree)] for _ in range(total)]
    database = orc.plaintext_to_eval(np.array(entries, dtype=np.uint64))
    qctx = orc.ciphertext_context()
    one, zero = [1] + [0] * (degree - 1), [0] * degree
    selection = [2, 1]
    dim0 = np.stack([qctx.forward_ntt(client.encrypt(one if j == selection[0] else zero)) for j in range(dims[0])])
    rest = np.stack([client.encrypt(one if j == selection[1] else zero) for j in range(dims[1])])
    response = ours.pir_compute_response_chunk(dims, heamd.to_device(dim0), heamd.to_device(rest), heamd.to_device(database),
                                               np.ones(total, dtype=np.uint8), heamd.to_device(client.relinearization_key()))
    cts = response.reshape(1, 2, 1, degree)  # [2][1][N] Coeff over q_0
    key = heamd.to_device(client.s_eval_all)
    plain = heamd.to_host(ours.decrypt(cts, key))[0]
    assert [int(v) for v in plain] == entries[selection[0] + selection[1] * dims[0]]
    moduli = [int(q[0])]
    dot = ref.dot_product(orc.ciphertext_context(1), heamd.to_host(response), client.s_eval_all)
    norm = ref.noise_norm(dot, moduli, t)
    assert ours.noise_norm(cts, key) == [norm]
    budget = ours.noise_budget(cts, key)[0]
    assert budget > 0
    _budgets_agree([budget], [ref.noise_budget(norm, moduli)])
    assert ours.is_transparent(cts).cpu().tolist() == [0]


def test_errors_and_no_ops(oracle):
    import torch

    case = Case(oracle, "n64_q40_41", 64)
    ours, L, n, t = case.ours, case.L, case.degree, case.t
    cts, key = case.device(case.cts[2][L]), case.key
    lib = heamd.load_library()
    ptr = lambda tensor: ctypes.c_void_p(tensor.data_ptr())  # noqa: E731
    out = torch.zeros((case.batch, L, n), dtype=torch.int64, device=cts.device)
    limbs = torch.zeros((case.batch, 2), dtype=torch.int64, device=cts.device)
    flags = torch.zeros((case.batch,), dtype=torch.uint8, device=cts.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def status(code):
        return heamd.binding.STATUS_NAMES[code]

    def entries(word_bits, moduli_count, polys, batch=case.batch, workspace=None, workspace_bytes=0, factor=1):
        return [
            lib.he_bfv_secret_dot_product_device(ours.h, word_bits, moduli_count, polys, 0, ptr(cts), ptr(key), ptr(out), batch,
                                                 workspace, workspace_bytes, stream),
            lib.he_bfv_decrypt_device(ours.h, word_bits, moduli_count, polys, 0, ptr(cts), ptr(key), factor, ptr(out), batch,
                                      workspace, workspace_bytes, stream),
            lib.he_bfv_noise_norm_device(ours.h, word_bits, moduli_count, polys, 0, ptr(cts), ptr(key), ptr(limbs), batch,
                                         workspace, workspace_bytes, stream),
            lib.he_bfv_is_transparent_device(ours.h, word_bits, moduli_count, polys, ptr(cts), ptr(flags), batch, stream),
        ]

    assert [status(c) for c in entries(16, L, 2)] == ["invalidArgument"] * 4  # word_bits
    assert [status(c) for c in entries(32, L, 2)] == ["invalidArgument"] * 4  # 4-byte slabs on a Bfv<UInt64> context
    for polys in (0, 4):
        assert [status(c) for c in entries(64, L, polys)] == ["unsupportedHeOperation"] * 4
    for moduli_count in (0, L + 1):
        assert [status(c) for c in entries(64, moduli_count, 2)] == ["invalidArgument"] * 4
    # batch 0 is a no-op, with null slabs too
    assert [status(c) for c in entries(64, L, 2, batch=0)] == ["ok"] * 4
    assert status(lib.he_bfv_decrypt_device(ours.h, 64, L, 2, 0, None, None, 1, None, 0, None, 0, stream)) == "ok"
    torch.cuda.synchronize()
    assert not out.any() and not limbs.any() and not flags.any()
    # the correction factor: 0 has no inverse; t is not reduced
    assert status(entries(64, L, 2, factor=0)[1]) == "notInvertible"
    assert status(entries(64, L, 2, factor=t)[1]) == "invalidArgument"
    with pytest.raises(heamd.HeError) as err:
        ours.decrypt(cts, key, 0)
    assert err.value.name == "notInvertible"
    # a workspace one byte short is refused, one of the stated size is enough
    need = ours.decrypt_workspace_bytes(case.batch, 2, False)
    assert need == (case.batch * L * n + case.batch * L * n) * 8  # the dot product, and the copy of c1 (c0 needs none)
    workspace = torch.zeros(need, dtype=torch.uint8, device=cts.device)
    # (all three entries, as he_amd.h states it: the dot product entry writes into the caller's slab and uses the copy alone,
    # and still takes no workspace below the reported size -- tests/test_gpu_footprint.py holds every entry to that)
    assert [status(c) for c in entries(64, L, 2, workspace=ptr(workspace), workspace_bytes=need - 1)[:3]] == ["invalidArgument"] * 3
    copy_bytes = case.batch * L * n * 8
    assert status(entries(64, L, 2, workspace=ptr(workspace), workspace_bytes=copy_bytes)[0]) == "invalidArgument"
    assert [status(c) for c in entries(64, L, 2, workspace=ptr(workspace), workspace_bytes=need)[:3]] == ["ok"] * 3
    got = heamd.to_host(ours.decrypt(cts, key, workspace=workspace))
    assert np.array_equal(got, heamd.to_host(ours.decrypt(cts, key)))
    assert np.array_equal(heamd.to_host(ours.secret_dot_product(cts, key, workspace=workspace)), case.oracle_dot(2, L))
    # null slabs with a batch
    assert status(lib.he_bfv_decrypt_device(ours.h, 64, L, 2, 0, None, ptr(key), 1, ptr(out), 1, None, 0, stream)) == "invalidArgument"
    assert status(lib.he_bfv_is_transparent_device(ours.h, 64, L, 2, ptr(cts), None, 1, stream)) == "invalidArgument"
