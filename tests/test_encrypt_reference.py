"""tests/encrypt_reference.py held to what is known without a device: the reference's recorded sampler results
(tests/golden/randomize_interop_kats.json, PolyRq+RandomizeTests.swift:150-196), the exact client of bfv_helpers, and the shape
of a key-switch key.  Then the host side of the new entries: argument errors, workspace sizes, header and exports."""
import json
import math
import os
import re

import numpy as np
import pytest

import encrypt_reference as ref
import heamd
from bfv_helpers import BfvClient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("he_bfv_encrypt_workspace_bytes", "he_bfv_generate_secret_key_device", "he_bfv_encrypt_zero_device",
               "he_bfv_encrypt_device", "he_bfv_generate_key_switch_keys_device", "he_bfv_generate_relinearization_key_device",
               "he_bfv_generate_galois_keys_device", "he_poly_random_ternary_from_seeds_device",
               "he_poly_random_centered_binomial_from_seeds_device")


@pytest.fixture(scope="module")
def kats():
    with open(os.path.join(ROOT, "tests", "golden", "randomize_interop_kats.json")) as f:
        return json.load(f)


def test_trial_bits_in_doubles():
    assert math.ceil(2 * 3.2 * 3.2) == 21 == ref.TRIAL_BITS
    assert 2 * 3.2 * 3.2 > 20.0  # (not a rounding accident at the boundary: 20.48)


@pytest.mark.parametrize("sampler", ["ternary", "centered_binomial"])
def test_restatement_reproduces_the_interop_kats(oracle, kats, sampler):
    seed, n = bytes.fromhex(kats["seed"]), kats["degree"]
    kat = kats[sampler]
    per_coefficient = 12 if sampler == "ternary" else 16
    last = max(kats["polynomial_positions"])
    stream = ref.oracle_stream(oracle)(seed, per_coefficient * n * (last + 1))
    draw = ref.ternary if sampler == "ternary" else ref.centered_binomial
    for position, expected in zip(kats["polynomial_positions"], kat["polynomials"]):
        got = draw(stream, n, kat["moduli"], first=n * position)
        assert got.reshape(-1).tolist() == expected, (sampler, position)


def test_oracle_stream_is_the_python_drbg(oracle):
    import wire_format_reference as wire

    seed = bytes(range(32))
    drbg = wire.CtrDrbg(seed)
    assert ref.oracle_stream(oracle)(seed, 4096 + 40) == (bytes(drbg.generate(4096)) + bytes(drbg.generate(4096)))[:4096 + 40]


def _client(oracle, degree, bits, t_bits=17):
    moduli = oracle.generate_primes(bits, False, degree)
    t = oracle.generate_primes([t_bits], True, degree)[0]
    ctx = oracle.BfvContext(degree, t, moduli)
    client = BfvClient(oracle, ctx)
    # the restated secret key takes the place of the client's own
    client.s_eval_all = ref.generate_secret_key(client.secret_ctx, bytes([7] * 32), ref.oracle_stream(oracle))
    return ctx, client


@pytest.mark.parametrize("degree,bits", [(8, [30, 30, 30]), (512, [40, 41, 42])])
def test_restated_encryption_decrypts_exactly(oracle, degree, bits):
    ctx, client = _client(oracle, degree, bits)
    stream = ref.oracle_stream(oracle)
    coefficients = client.secret_ctx.inverse_ntt(client.s_eval_all)
    for row, q in zip(coefficients, client.all_moduli):
        assert set(int(v) for v in row) <= {0, 1, q - 1}
    rng = np.random.default_rng(degree)
    for moduli_count in range(1, ctx.L + 1):
        message = [int(v) for v in rng.integers(0, ctx.t, degree)]
        ct = ref.encrypt(ctx.ciphertext_context(moduli_count), ctx.t, message, client.s_eval_all, bytes([moduli_count] * 32),
                         bytes([0x80 + moduli_count] * 32), stream)
        assert client.decrypt_exact(ct, moduli_count) == message
        assert client.decrypt(ct, moduli_count) == message


def test_restated_relinearization_key_has_the_helpers_structure(oracle):
    """bfv_helpers._key_switch_key: ciphertext j is an Eval encryption of zero under s over all moduli with
    (q_ks mod q_j) currentKey added to row j -- so c0 + c1 s, inverse-transformed, is -e everywhere but in row j."""
    degree = 64
    ctx, client = _client(oracle, degree, [40, 41, 42])
    stream = ref.oracle_stream(oracle)
    ks_ctx = ctx.key_switching_context()
    s = client.s_eval_all
    current = ref.relinearization_current_key(client.secret_ctx, s)
    assert np.array_equal(current, ks_ctx.mul(s, s))
    a_seeds = [bytes([j] * 32) for j in range(ctx.L)]
    e_seeds = [bytes([0x40 + j] * 32) for j in range(ctx.L)]
    key = ref.key_switch_key(ks_ctx, s, current, a_seeds, e_seeds, stream)
    helper = client._key_switch_key(current)
    assert key.shape == helper.shape == (ctx.L, 2, ctx.L + 1, degree)
    moduli = ks_ctx.moduli
    for j in range(ctx.L):
        noise = ks_ctx.inverse_ntt(ks_ctx.add(key[j, 0], ks_ctx.mul(key[j, 1], s)))
        payload = ks_ctx.inverse_ntt(ks_ctx.mul_scalar(current, [moduli[-1] % q for q in moduli]))
        expected_e = ref.binomial_values(stream(e_seeds[j], 16 * degree), degree)
        for row, q in enumerate(moduli):
            rest = (noise[row].astype(object) - (payload[row].astype(object) if row == j else 0)) % q
            assert [int(v) for v in rest] == [(-e) % q for e in expected_e], (j, row)


# ---- the host side of the entries ----------------------------------------------------------------------------------------

def _status(code):
    return heamd.binding.STATUS_NAMES[code]


class _HostContext:
    """a host-only Context<Bfv<UInt64>> or Context<Bfv<UInt32>> (no device tables: every device entry ends in deviceError)"""

    def __init__(self, bits, degree=8, scheme_bits=64):
        import ctypes

        lib = heamd.load_library()
        moduli = heamd.generate_primes(bits, False, degree)
        t = heamd.generate_primes([17], True, degree)[0]
        create = lib.he_bfv_context_create_u32_host_only if scheme_bits == 32 else lib.he_bfv_context_create_host_only
        array = (ctypes.c_uint64 * len(moduli))(*moduli)
        self.h = ctypes.c_void_p()
        assert create(degree, t, array, len(moduli), ctypes.byref(self.h)) == 0
        self.L = int(lib.he_bfv_ciphertext_moduli_count(self.h))

    def __del__(self):
        if getattr(self, "h", None):
            heamd.load_library().he_bfv_context_destroy(self.h)
            self.h = None


def _host_context(bits, degree=8, scheme_bits=64):
    return _HostContext(bits, degree, scheme_bits)


# (the scheme's scalar, the slab word): Bfv<UInt32> constants serve 8-byte slabs as well as packed 4-byte ones
HOST_WORDS = [(64, 64), (32, 64), (32, 32)]


def _all_entries(lib, ctx, word_bits, moduli_count=1, elements=(3,), count=1):
    """every device entry with non-null dummy pointers (none is dereferenced before the device check)"""
    import ctypes

    a, b, c, d, e = (ctypes.c_void_p(n << 24) for n in range(1, 6))  # a slab each, far apart: slabs of a call must not overlap
    element_array = (ctypes.c_uint64 * max(len(elements), 1))(*elements)
    return {
        "secret_key": lib.he_bfv_generate_secret_key_device(ctx, word_bits, a, b, count, None, 0, None),
        "encrypt_zero": lib.he_bfv_encrypt_zero_device(ctx, word_bits, moduli_count, 0, a, b, c, d, count, None, 0, None),
        "encrypt": lib.he_bfv_encrypt_device(ctx, word_bits, moduli_count, a, b, c, d, e, count, None, 0, None),
        "key_switch_keys": lib.he_bfv_generate_key_switch_keys_device(ctx, word_bits, a, b, c, d, e, count, None, 0, None),
        "relinearization_key": lib.he_bfv_generate_relinearization_key_device(ctx, word_bits, a, b, c, d, None, 0, None),
        "galois_keys": lib.he_bfv_generate_galois_keys_device(ctx, word_bits, a, element_array, len(elements), b, c, d, None, 0,
                                                              None),
    }


def test_word_and_context_errors():
    lib = heamd.load_library()
    for scheme_bits in (64, 32):
        ctx = _host_context([28, 29, 30], scheme_bits=scheme_bits)
        for word_bits in (0, 16, 48, 128):
            assert {_status(v) for v in _all_entries(lib, ctx.h, word_bits).values()} == {"invalidArgument"}
            assert lib.he_bfv_encrypt_workspace_bytes(ctx.h, word_bits, 1, 1, 0, 1) == 0
    for word_bits in (64, 32):
        assert {_status(v) for v in _all_entries(lib, None, word_bits).values()} == {"invalidArgument"}
    # a 4-byte call on a Bfv<UInt64> context: what the decryption entries answer on a device
    ctx = _host_context([28, 29, 30])
    assert {_status(v) for v in _all_entries(lib, ctx.h, 32).values()} == {"invalidArgument"}
    assert b"Bfv<UInt32>" in lib.he_last_error_message()


@pytest.mark.parametrize("scheme_bits,word_bits", HOST_WORDS)
def test_argument_errors_come_before_the_device(scheme_bits, word_bits):
    lib = heamd.load_library()
    ctx = _host_context([28, 29, 30], scheme_bits=scheme_bits)
    assert ctx.L == 2
    # moduli_count: encrypt_zero takes 1 .. L_all, encrypt 1 .. L
    for entry, bad in (("encrypt_zero", (0, 4)), ("encrypt", (0, 3))):
        for moduli_count in bad:
            assert _status(_all_entries(lib, ctx.h, word_bits, moduli_count)[entry]) == "invalidArgument", (entry, moduli_count)
    ok = _all_entries(lib, ctx.h, word_bits, 2)
    assert {_status(v) for v in ok.values()} == {"deviceError"}  # valid arguments reach the host-only context's refusal
    assert _status(_all_entries(lib, ctx.h, word_bits, 3)["encrypt_zero"]) == "deviceError"  # m = L_all
    # Galois elements: even, 1, 2N and beyond
    for element in (2, 1, 0, 16, 17, 2**40 + 1):
        assert _status(_all_entries(lib, ctx.h, word_bits, elements=(3, element))["galois_keys"]) == "invalidArgument", element
    assert _status(_all_entries(lib, ctx.h, word_bits, elements=(3, 15))["galois_keys"]) == "deviceError"
    # a count of 0 does nothing, whatever the pointers
    assert lib.he_bfv_generate_secret_key_device(ctx.h, word_bits, None, None, 0, None, 0, None) == 0
    assert lib.he_bfv_encrypt_zero_device(ctx.h, word_bits, 1, 0, None, None, None, None, 0, None, 0, None) == 0
    assert lib.he_bfv_encrypt_device(ctx.h, word_bits, 1, None, None, None, None, None, 0, None, 0, None) == 0
    assert lib.he_bfv_generate_key_switch_keys_device(ctx.h, word_bits, None, None, None, None, None, 0, None, 0, None) == 0
    assert lib.he_bfv_generate_galois_keys_device(ctx.h, word_bits, None, None, 0, None, None, None, None, 0, None) == 0


@pytest.mark.parametrize("scheme_bits,word_bits", HOST_WORDS)
def test_one_modulus_context_supports_no_evaluation_key(scheme_bits, word_bits):
    lib = heamd.load_library()
    ctx = _host_context([30], scheme_bits=scheme_bits)
    got = {name: _status(v) for name, v in _all_entries(lib, ctx.h, word_bits).items()}
    assert got == {"secret_key": "deviceError", "encrypt_zero": "deviceError", "encrypt": "deviceError",
                   "key_switch_keys": "unsupportedHeOperation", "relinearization_key": "unsupportedHeOperation",
                   "galois_keys": "unsupportedHeOperation"}
    for operation in (3, 4, 5):
        assert lib.he_bfv_encrypt_workspace_bytes(ctx.h, word_bits, operation, 1, 0, 1) == 0
    assert lib.he_bfv_encrypt_workspace_bytes(ctx.h, word_bits, 1, 1, 0, 1) != 0


def test_workspace_bytes():
    lib = heamd.load_library()
    n, L = 512, 2
    ctx = _host_context([30, 30, 30], n)
    record = 192
    uniform = lambda m, count: count * (m * n // 256) * record  # noqa: E731  the DRBG records of `a`
    error = lambda count: count * (n // 256) * record  # noqa: E731
    for bits, word in ((64, 8), (32, 4)):
        size = lambda *args: lib.he_bfv_encrypt_workspace_bytes(ctx.h, bits, *args)  # noqa: E731
        assert size(0, 0, 0, 5) == 5 * 2 * record  # ternary: ceil(12 * 512 / 4096) chunks
        for m in (1, 2, 3):
            assert size(1, m, 0, 3) == uniform(m, 3) + error(3)
            assert size(1, m, 1, 3) == uniform(m, 3) + error(3) + 3 * m * n * word
        assert size(2, 2, 0, 3) == size(2, 2, 1, 3) == uniform(2, 3) + error(3)
        assert size(2, 3, 0, 3) == 0 == size(1, 4, 0, 3) == size(1, 0, 0, 3) == size(6, 1, 0, 3) == size(-1, 1, 0, 3)
        keys = 4
        key_switch = uniform(L + 1, keys * L) + error(keys * L) + keys * L * (L + 1) * n * word
        assert size(3, 0, 0, keys) == key_switch
        assert size(5, 0, 0, keys) == key_switch + keys * (L + 1) * n * word
        assert size(4, 0, 0, 77) == uniform(L + 1, L) + error(L) + L * (L + 1) * n * word + (L + 1) * n * word
    assert lib.he_bfv_encrypt_workspace_bytes(None, 64, 1, 1, 0, 1) == 0
    # degrees below a chunk: one record per seed
    small = _host_context([30, 30], 8)
    assert lib.he_bfv_encrypt_workspace_bytes(small.h, 64, 1, 1, 0, 2) == 2 * record + 2 * record
    assert lib.he_bfv_encrypt_workspace_bytes(small.h, 64, 0, 0, 0, 2) == 2 * record


def test_polynomial_sampler_argument_errors():
    import ctypes

    lib = heamd.load_library()
    fake, other = ctypes.c_void_p(16), ctypes.c_void_p(1 << 24)  # seeds and polynomials must not overlap
    host = heamd.PolyContext(8, heamd.generate_primes([40, 41], False, 8), host_only=True)
    for entry in (lib.he_poly_random_ternary_from_seeds_device, lib.he_poly_random_centered_binomial_from_seeds_device):
        assert _status(entry(host.h, 16, fake, 1, fake, None)) == "invalidArgument"
        assert _status(entry(None, 64, fake, 1, fake, None)) == "invalidArgument"
        assert _status(entry(host.h, 32, fake, 1, fake, None)) == "invalidModulus"  # 40 bits do not fit a 4-byte word
        assert entry(host.h, 64, None, 0, None, None) == 0
        assert _status(entry(host.h, 64, None, 1, fake, None)) == "invalidArgument"
        assert _status(entry(host.h, 64, fake, 1, other, None)) == "deviceError"


def test_header_exports_and_binding_name_the_entries():
    header = open(os.path.join(ROOT, "include", "he_amd.h")).read()
    copy = open(os.path.join(ROOT, "swift", "Sources", "CHeAmd", "include", "he_amd.h")).read()
    assert header == copy
    exports = open(os.path.join(ROOT, "swift-homomorphic-encryption_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*he_\*;", exports)  # the map exports the he_ prefix
    lib = heamd.load_library()
    bound = {name for name, _, _ in heamd.binding.SIGNATURES}
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in bound and name + "_u32" not in bound, name
        assert not re.search(r"\b%s_u32\b" % name, header), name
