"""Secret keys, encryptions and evaluation keys made on the device from caller-supplied seeds (he_poly_random_ternary_from_
seeds_device, he_poly_random_centered_binomial_from_seeds_device, he_bfv_generate_secret_key_device, he_bfv_encrypt_zero_device,
he_bfv_encrypt_device, he_bfv_generate_key_switch_keys_device, he_bfv_generate_relinearization_key_device,
he_bfv_generate_galois_keys_device) on both slab words:

  * the samplers word for word against tests/encrypt_reference.py at every geometry of the stream: shorter than a chunk
    (N = 8), one chunk (256), the first straddle of a ternary record (512), the whole 3-chunk period (1024: the words at
    k = 340..342 and 681..683 by name), many chunks (4096); 1-4 moduli; batches around the 8 seeds a chain wavefront packs;
    seeds all-zero, all-0xff and with counter carries; the reference's recorded results (randomize_interop_kats.json) at N = 8192;
  * encryptZero in Coeff and Eval form at every moduli count 1 .. L_all, its `a` against the seeded deserializer, Eval against
    the device's own forward transform of Coeff; encrypt against encryptZero + add_plain, decrypted on the device, its exact
    noise norm against the bound that follows from |e| <= 21;
  * relinearization and Galois keys word for word, and used: multiply + relinearize and applyGalois decrypt to what the plain
    ring gives;
  * zeroization of a caller's workspace, empty batches, a context that supports no evaluation key.

Every case builds its contexts, keys and restated values once (module-scoped cache)."""
import functools
import os

import numpy as np
import pytest
import torch

import encrypt_reference as ref
import heamd
import wire_format_reference as wire
from bfv_helpers import galois_plain, negacyclic_multiply
from heamd.binding import WORD32, WORD64

pytestmark = pytest.mark.gpu

WORDS = {64: WORD64, 32: WORD32}


def _to_device(array, word):
    return heamd.to_device32(array) if word == 32 else heamd.to_device(array)


def _to_host(tensor, word):
    return heamd.to_host32(tensor) if word == 32 else heamd.to_host(tensor)


def _seeds(count, salt):
    """[count][32] uint8: all-zero, all-0xff, counter-carry seeds (one per boundary and a few offsets), then random ones"""
    special = [bytes(32), bytes([0xff] * 32)]
    cases = wire.carry_cases()
    special += [cases[i][3] for i in (0, 8, 13, 21, 26, 34, 39, 47)]  # k = 1, 256, 2, 257 at each of the four boundaries
    rng = np.random.default_rng(salt)
    rows = [np.frombuffer(s, dtype=np.uint8) for s in special[:count]]
    rows += [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(count - len(rows))]
    return np.stack(rows)


def _device_seeds(seeds):
    return torch.from_numpy(np.array(seeds, dtype=np.uint8, order="C")).cuda()


# ---- the samplers -----------------------------------------------------------------------------------------------------------

# (degree, bits of the moduli, slab word, batch)
SAMPLER_CASES = [
    (8, [30], 64, 1), (8, [28, 29], 32, 7), (256, [40, 41, 42], 64, 9), (256, [28], 32, 70), (512, [45, 46], 64, 7),
    (512, [27, 28, 29, 30], 32, 9), (1024, [50, 51, 52, 53], 64, 70), (1024, [29, 30], 32, 9), (4096, [55], 64, 7),
    (4096, [27, 28, 28], 32, 1),
]


@functools.lru_cache(maxsize=None)
def _sampler_case(degree, bits, word, batch):
    import oracle

    oracle.build()
    moduli = heamd.generate_primes(list(bits), False, degree)
    seeds = _seeds(batch, degree + word + batch)
    stream = ref.oracle_stream(oracle)
    streams = [stream(bytes(seed), 16 * degree) for seed in seeds]
    ternary = np.stack([ref.ternary(s, degree, moduli) for s in streams])
    binomial = np.stack([ref.centered_binomial(s, degree, moduli) for s in streams])
    return moduli, seeds, streams, ternary, binomial


@pytest.mark.parametrize("degree,bits,word,batch", SAMPLER_CASES)
def test_samplers_word_for_word(degree, bits, word, batch):
    moduli, seeds, streams, ternary, binomial = _sampler_case(degree, tuple(bits), word, batch)
    ctx = heamd.PolyContext(degree, moduli)
    device_seeds = _device_seeds(seeds)
    got_ternary = _to_host(ctx.random_ternary_from_seeds(device_seeds, WORDS[word]), word)
    got_binomial = _to_host(ctx.random_centered_binomial_from_seeds(device_seeds, WORDS[word]), word)
    assert got_ternary.shape == got_binomial.shape == (batch, len(moduli), degree)
    assert np.array_equal(got_ternary, ternary)
    assert np.array_equal(got_binomial, binomial)
    if degree == 1024:
        # 4096 = 341 * 12 + 4: coefficient 341 has 4 bytes of its UInt64 in chunk 0, coefficient 682 its UInt64 in chunk 1 and
        # its UInt32 in chunk 2
        for b in range(batch):
            values = ref.ternary_values(streams[b], degree)
            for k in (340, 341, 342, 681, 682, 683):
                for i, q in enumerate(moduli):
                    assert int(got_ternary[b, i, k]) == (values[k] - 1) % q, (b, i, k)
    # the draws are what they should be as numbers, too
    for i, q in enumerate(moduli):
        assert set(np.unique(got_ternary[:, i]).tolist()) <= {0, 1, q - 1}
        centred = np.where(got_binomial[:, i] > q // 2, got_binomial[:, i].astype(np.int64) - q, got_binomial[:, i].astype(np.int64))
        assert np.abs(centred).max() <= ref.TRIAL_BITS


def test_samplers_reproduce_the_interop_kats_on_the_device():
    """The reference's known answers are polynomials 0, 1001 and 2002 of degree 4 of one generator: coefficients 0..3, 4004..4007
    and 8008..8011 of the stream, all below N = 8192."""
    import json

    import oracle

    oracle.build()
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "randomize_interop_kats.json")) as f:
        kats = json.load(f)
    degree = 8192
    device_seed = _device_seeds(np.frombuffer(bytes.fromhex(kats["seed"]), dtype=np.uint8)[None])
    friendly = heamd.generate_primes([30, 31], False, degree)
    for sampler, kat in (("ternary", kats["ternary"]), ("centered_binomial", kats["centered_binomial"])):
        draw = heamd.PolyContext.random_ternary_from_seeds if sampler == "ternary" else \
            heamd.PolyContext.random_centered_binomial_from_seeds
        try:
            ctx = heamd.PolyContext(degree, kat["moduli"])
            direct = True
        except heamd.HeError:
            ctx = heamd.PolyContext(degree, friendly)
            direct = False
        got = heamd.to_host(draw(ctx, device_seed))[0]
        print(f"{sampler}: the polynomial context {'accepts' if direct else 'refuses'} the KAT moduli {kat['moduli']}: compared "
              f"{'directly' if direct else 'as signed values at NTT-friendly moduli'}")
        for position, expected in zip(kats["polynomial_positions"], kat["polynomials"]):
            rows = np.array(expected).reshape(len(kat["moduli"]), kats["degree"])
            window = slice(kats["degree"] * position, kats["degree"] * (position + 1))
            if direct:
                assert np.array_equal(got[:, window], rows.astype(np.uint64)), (sampler, position)
                continue
            # the signed value: ternary from the row mod 11; binomial from both rows by CRT (23 * 29 > 2 * 21 + 1)
            q0, q1 = kat["moduli"]
            if sampler == "ternary":
                signed = [int(v) - q0 if int(v) > q0 // 2 else int(v) for v in rows[0]]
            else:
                signed = []
                for r0, r1 in zip(rows[0], rows[1]):
                    x = next(x for x in range(q0 * q1) if x % q0 == r0 and x % q1 == r1)
                    signed.append(x - q0 * q1 if x > q0 * q1 // 2 else x)
            for i, q in enumerate(friendly):
                assert [int(v) for v in got[i, window]] == [s % q for s in signed], (sampler, position, i)


# ---- BFV: keys, encryption ------------------------------------------------------------------------------------------------------

# name: (degree, bits of every coefficient modulus (the last one is the key-switching modulus), slab word, bits of t)
BFV_CASES = {
    "n8_w64": (8, [30, 31, 32], 64, 5),
    "n8_w32": (8, [28, 29, 30], 32, 5),
    "n512_w64": (512, [40, 41], 64, 17),
    "n512_w32": (512, [27, 28, 28], 32, 17),
    "n4096_w64": (4096, [50, 51, 52, 53], 64, 17),
    "n4096_w32": (4096, [27, 28, 28], 32, 17),
}


class Case:
    def __init__(self, name):
        import oracle

        oracle.build()
        degree, bits, word, t_bits = BFV_CASES[name]
        key_seeds = _seeds(3, 1000 + degree)[::-1].copy()  # a random seed first: key 0 is THE key of the case
        self.setup(ref.HostSide(oracle, degree, heamd.generate_primes([t_bits], True, degree)[0],
                                heamd.generate_primes(bits, False, degree), word, key_seeds))

    def setup(self, host):
        """the device context and keys beside an encrypt_reference.HostSide, whose fields the case takes over
        (tests/test_gpu_predefined_sets.py builds its cases of the reference's own parameter sets through this)"""
        vars(self).update(vars(host))
        cls = heamd.BfvContext32 if self.word == 32 else heamd.BfvContext
        self.ctx = cls(self.degree, self.t, self.moduli)
        self.keys_device = self.ctx.generate_secret_key(_device_seeds(self.key_seeds))
        self.s_device = self.keys_device[0].contiguous()
        self.L = self.ctx.L

    def to_host(self, tensor):
        return _to_host(tensor, self.word)

    def to_device(self, array):
        return _to_device(array, self.word)

    def prefix_ctx(self, m):
        return self.oracle.PolyContext(self.degree, self.moduli[:m])


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(name)


@pytest.fixture(params=list(BFV_CASES))
def case(request):
    return _case(request.param)


def test_secret_keys(case):
    got = case.to_host(case.keys_device)
    assert got.shape == (3, case.L_all, case.degree)
    for b, seed in enumerate(case.key_seeds):
        assert np.array_equal(got[b], ref.generate_secret_key(case.secret_ctx, bytes(seed), case.stream)), b


def test_encrypt_zero_every_moduli_count(case):
    for m in range(1, case.L_all + 1):
        batch = (1, 3, 9)[m % 3]
        a_seeds, e_seeds = _seeds(batch, 10 * m), _seeds(batch, 10 * m + 1)[::-1].copy()
        poly_ctx = case.prefix_ctx(m)
        expected = np.stack([ref.encrypt_zero(poly_ctx, case.s_eval, bytes(a), bytes(e), case.stream)
                             for a, e in zip(a_seeds, e_seeds)])
        coeff = case.ctx.encrypt_zero(case.s_device, _device_seeds(a_seeds), _device_seeds(e_seeds), m)
        evaluated = case.ctx.encrypt_zero(case.s_device, _device_seeds(a_seeds), _device_seeds(e_seeds), m, eval_out=True)
        assert tuple(coeff.shape) == (batch, 2, m, case.degree)
        assert np.array_equal(case.to_host(coeff), expected), m
        assert np.array_equal(case.to_host(evaluated), poly_ctx.forward_ntt(expected)), m
        # against the entries that existed before: `a` as the seeded deserializer regenerates it, Eval as the transform of Coeff
        ours = heamd.PolyContext(case.degree, case.moduli[:m])
        seeded = ours.ciphertexts_deserialize_seeded(None, _device_seeds(a_seeds), batch, True, word_bits=case.word)
        assert torch.equal(seeded[:, 1], coeff[:, 1]), m
        forward = ours.forward_ntt_u32_ if case.word == 32 else ours.forward_ntt_
        assert torch.equal(forward(coeff.clone()), evaluated), m


def test_encrypt_is_encrypt_zero_plus_add_plain_and_decrypts(case):
    rng = np.random.default_rng(case.degree)
    n, t = case.degree, case.t
    messages = np.stack([np.zeros(n, dtype=np.uint64), np.full(n, t - 1, dtype=np.uint64),
                         rng.integers(0, t, n).astype(np.uint64)])
    a_seeds, e_seeds = _seeds(3, 77)[::-1].copy(), _seeds(3, 78)
    for m in range(1, case.L + 1):
        plaintexts = case.to_device(messages)
        cts = case.ctx.encrypt(plaintexts, case.s_device, _device_seeds(a_seeds), _device_seeds(e_seeds), m)
        composed = case.ctx.encrypt_zero(case.s_device, _device_seeds(a_seeds), _device_seeds(e_seeds), m)
        case.ctx.add_plain_(composed, plaintexts, moduli_count=m)
        assert torch.equal(cts, composed), m
        expected = np.stack([ref.encrypt(case.prefix_ctx(m), t, messages[b], case.s_eval, bytes(a_seeds[b]), bytes(e_seeds[b]),
                                         case.stream) for b in range(3)])
        assert np.array_equal(case.to_host(cts), expected), m
        assert np.array_equal(case.to_host(case.ctx.decrypt(cts, case.s_device)), messages), m
        # t (c0 + c1 s) = t (Delta m + adjust - e) = -(Q mod t) m + t adjust - t e (mod Q) with t adjust = (Q mod t) m + r,
        # |r| <= (t + 1) / 2 by the rounding of plaintextTranslate, and |e| <= 21: at most 21 t + (t + 1) / 2
        for norm in case.ctx.noise_norm(cts, case.s_device):
            assert norm <= 21 * t + (t + 1) // 2, (m, norm)


def _key_seeds(case, keys, salt):
    a = _seeds(keys * case.L, salt).reshape(keys, case.L, 32)
    e = _seeds(keys * case.L, salt + 1)[::-1].copy().reshape(keys, case.L, 32)
    return a, e


def _galois_elements(case):
    n = case.degree
    return [3, 2 * n - 1, n + 1] if n > 8 else [3, 2 * n - 1, 5]


def test_evaluation_keys_word_for_word(case):
    ks_ctx = case.prefix_ctx(case.L_all)
    a, e = _key_seeds(case, 1, 300)
    current = ref.relinearization_current_key(case.secret_ctx, case.s_eval)
    expected = ref.key_switch_key(ks_ctx, case.s_eval, current, [bytes(s) for s in a[0]], [bytes(s) for s in e[0]], case.stream)
    got = case.ctx.generate_relinearization_key(case.s_device, _device_seeds(a), _device_seeds(e))
    assert tuple(got.shape) == (case.L, 2, case.L + 1, case.degree)
    assert np.array_equal(case.to_host(got), expected)
    # the same key through the entry that takes current keys, and several Galois keys at once
    direct = case.ctx.generate_key_switch_keys(case.s_device, case.to_device(current[None]), _device_seeds(a), _device_seeds(e))
    assert torch.equal(direct[0], got)
    elements = _galois_elements(case)
    a, e = _key_seeds(case, len(elements), 400)
    got = case.to_host(case.ctx.generate_galois_keys(case.s_device, elements, _device_seeds(a), _device_seeds(e)))
    assert got.shape == (len(elements), case.L, 2, case.L + 1, case.degree)
    for k, element in enumerate(elements):
        current = ref.galois_current_key(case.secret_ctx, case.s_eval, element)
        expected = ref.key_switch_key(ks_ctx, case.s_eval, current, [bytes(s) for s in a[k]], [bytes(s) for s in e[k]],
                                      case.stream)
        assert np.array_equal(got[k], expected), element


@pytest.mark.parametrize("name", ["n8_w64", "n8_w32"])
def test_more_galois_elements_than_one_launch_carries(name):
    """The rotated keys of 64 elements travel in one launch's arguments: 70 elements (repeats are allowed) take two, and the
    keys on both sides of the seam are the restatement's."""
    case = _case(name)
    valid = [3, 5, 7, 9, 11, 13, 15]
    elements = [valid[(3 * k) % len(valid)] for k in range(70)]
    a, e = _key_seeds(case, len(elements), 700)
    got = case.to_host(case.ctx.generate_galois_keys(case.s_device, elements, _device_seeds(a), _device_seeds(e)))
    ks_ctx = case.prefix_ctx(case.L_all)
    for k in (0, 1, 62, 63, 64, 65, 69):
        current = ref.galois_current_key(case.secret_ctx, case.s_eval, elements[k])
        expected = ref.key_switch_key(ks_ctx, case.s_eval, current, [bytes(s) for s in a[k]], [bytes(s) for s in e[k]],
                                      case.stream)
        assert np.array_equal(got[k], expected), (k, elements[k])


@pytest.mark.parametrize("name", ["n8_w64", "n512_w32", "n4096_w64"])
def test_device_made_keys_work(name):
    case = _case(name)
    n, t = case.degree, case.t
    rng = np.random.default_rng(n + 1)
    messages = rng.integers(0, t, (2, n)).astype(np.uint64)
    cts = case.ctx.encrypt(case.to_device(messages), case.s_device, _device_seeds(_seeds(2, 500)[::-1].copy()),
                           _device_seeds(_seeds(2, 501)))
    a, e = _key_seeds(case, 1, 510)
    relin = case.ctx.generate_relinearization_key(case.s_device, _device_seeds(a), _device_seeds(e))
    product = case.ctx.relinearize(case.ctx.mul(cts[:1].contiguous(), cts[1:].contiguous()), relin)
    want = negacyclic_multiply([int(v) for v in messages[0]], [int(v) for v in messages[1]], t)
    assert [int(v) for v in case.to_host(case.ctx.decrypt(product, case.s_device))[0]] == want
    elements = _galois_elements(case)
    a, e = _key_seeds(case, len(elements), 520)
    keys = case.ctx.generate_galois_keys(case.s_device, elements, _device_seeds(a), _device_seeds(e))
    for k, element in enumerate(elements):
        rotated = case.ctx.apply_galois(cts[:1].contiguous(), element, keys[k].contiguous())
        got = [int(v) for v in case.to_host(case.ctx.decrypt(rotated, case.s_device))[0]]
        assert got == galois_plain([int(v) for v in messages[0]], element, t), element


@pytest.mark.parametrize("name", ["n8_w32", "n512_w64", "n4096_w32"])
def test_workspace_is_zeroized_and_changes_nothing(name):
    case = _case(name)
    ctx, s = case.ctx, case.s_device
    n = case.degree
    elements = _galois_elements(case)[:2]
    a1, e1 = _device_seeds(_seeds(3, 600)), _device_seeds(_seeds(3, 601)[::-1].copy())
    ak, ek = (_device_seeds(x) for x in _key_seeds(case, 2, 610))
    ar, er = (_device_seeds(x) for x in _key_seeds(case, 1, 620))
    plaintexts = case.to_device(np.random.default_rng(5).integers(0, case.t, (3, n)).astype(np.uint64))
    current = case.to_device(np.stack([ref.relinearization_current_key(case.secret_ctx, case.s_eval)] * 2))
    calls = [
        ("secret_key", 3, None, False, lambda ws: ctx.generate_secret_key(a1, workspace=ws)),
        ("encrypt_zero", 3, case.L_all, False, lambda ws: ctx.encrypt_zero(s, a1, e1, case.L_all, workspace=ws)),
        ("encrypt_zero", 3, 1, True, lambda ws: ctx.encrypt_zero(s, a1, e1, 1, eval_out=True, workspace=ws)),
        ("encrypt", 3, case.L, False, lambda ws: ctx.encrypt(plaintexts, s, a1, e1, workspace=ws)),
        ("key_switch_keys", 2, None, False, lambda ws: ctx.generate_key_switch_keys(s, current, ak, ek, workspace=ws)),
        ("relinearization_key", 1, None, False, lambda ws: ctx.generate_relinearization_key(s, ar, er, workspace=ws)),
        ("galois_keys", 2, None, False, lambda ws: ctx.generate_galois_keys(s, elements, ak, ek, workspace=ws)),
    ]
    for operation, count, m, eval_out, call in calls:
        needed = ctx.encrypt_workspace_bytes(operation, count, m, eval_out)
        assert needed > 0, operation
        workspace = torch.full((needed + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        with_workspace = call(workspace)
        torch.cuda.synchronize()
        assert int(workspace[:needed].count_nonzero()) == 0, operation
        assert bool((workspace[needed:] == 0xA5).all()), operation
        assert torch.equal(call(None), with_workspace), operation
        with pytest.raises(heamd.HeError) as caught:
            call(workspace[:needed - 16])
        assert caught.value.name == "invalidArgument", operation


def test_empty_batches_and_unsupported_contexts():
    case = _case("n8_w64")
    none = torch.empty((0, 32), dtype=torch.uint8, device="cuda")
    assert tuple(case.ctx.generate_secret_key(none).shape) == (0, 3, 8)
    assert tuple(case.ctx.encrypt_zero(case.s_device, none, none, 2).shape) == (0, 2, 2, 8)
    assert tuple(case.ctx.encrypt(torch.empty((0, 8), dtype=torch.int64, device="cuda"), case.s_device, none, none).shape) == \
        (0, 2, 2, 8)
    assert tuple(case.ctx.generate_galois_keys(case.s_device, [], none, none).shape) == (0, 2, 2, 3, 8)
    poly = heamd.PolyContext(8, heamd.generate_primes([28, 29, 30], False, 8))
    assert tuple(poly.random_ternary_from_seeds(none).shape) == (0, 3, 8)
    assert tuple(poly.random_centered_binomial_from_seeds(none, WORD32).shape) == (0, 3, 8)
    # one coefficient modulus: encryption works, key generation is what the reference refuses (supportsEvaluationKey)
    q = heamd.generate_primes([30], False, 8)
    single = heamd.BfvContext(8, case.t, q)
    key = single.generate_secret_key(_device_seeds(_seeds(1, 9)))
    seeds = _device_seeds(_seeds(2, 10))
    message = heamd.to_device(np.arange(16, dtype=np.uint64).reshape(2, 8) % case.t)
    cts = single.encrypt(message, key[0].contiguous(), seeds, seeds.flip(0).contiguous())
    assert torch.equal(single.decrypt(cts, key[0].contiguous()), message)
    for call in (lambda: single.generate_relinearization_key(key[0].contiguous(), seeds[:1], seeds[:1]),
                 lambda: single.generate_galois_keys(key[0].contiguous(), [3], seeds[:1], seeds[:1]),
                 lambda: single.generate_key_switch_keys(key[0].contiguous(), key, seeds[:1], seeds[:1])):
        with pytest.raises(heamd.HeError) as caught:
            call()
        assert caught.value.name == "unsupportedHeOperation"
