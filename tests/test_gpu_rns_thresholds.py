"""The device's RNS roundings at their decision thresholds, bit-exact against the Python-integer restatement of
rns_threshold_cases.py (which test_rns_threshold_cases.py holds the CPU oracle to on the same inputs):

  lift_kernel                      below    = r < mTilde/2          test_lift_*
  floor_kernel                     exceeds  = alpha > m_sk/2        test_floor_*
  scale_and_round_kernel           above    = mod_gamma > gamma/2   test_scale_and_round_*
  plaintext_translate_kernel       the +1 fix-up of the estimate    test_add_plain_*
  divide_and_round_q_last*_kernel,
  mod_switch_down_to_single_kernel negative = r < q_last/2          test_mod_switch_*
  key_switch_finish_kernel         negative = r < q_last/2          test_key_switch_finish_*

Every input sits ON a threshold or one to either side of it (uniform residues land there with probability 2^-32 .. 2^-61),
or is the residue vector of a structured integer (0, 1, Q - 1, Q/2 +- 1, k Q +- 1, k q_last + h)."""
import ctypes
import random

import numpy as np
import pytest

import heamd
import rns_threshold_cases as cases
from rns_threshold_cases import SETS, build_set, expected_rows, rows

pytestmark = pytest.mark.gpu

WIDE = [s[0] for s in cases.PARAMETER_SETS if s[1] == 64]
NARROW = [s[0] for s in cases.PARAMETER_SETS if s[1] == 32]


class Device:
    """A parameter set on the device: 8-byte slabs through BfvContext, packed 4-byte ones through BfvContext32."""

    def __init__(self, oracle, name, t_bits=None):
        self.name = name
        self.ref, self.levels = build_set(oracle, name, t_bits)
        narrow = SETS[name][1] == 32
        self.ours = (heamd.BfvContext32 if narrow else heamd.BfvContext)(self.ref.degree, self.ref.t, self.ref.coefficient_moduli)
        self.up, self.down = (heamd.to_device32, heamd.to_host32) if narrow else (heamd.to_device, heamd.to_host)
        self.degree = self.ref.degree
        assert self.ours.bsk_moduli() == self.levels[self.ours.L].bsk

    def shifted(self, array):
        """The same words one word into their allocation: no row starts on a 16-byte boundary, so the kernels take their
        one-word-per-lane form."""
        import torch

        aligned = self.up(array)
        slab = torch.empty(aligned.numel() + 1, dtype=aligned.dtype, device=aligned.device)[1:]
        slab.copy_(aligned.reshape(-1))
        assert aligned.data_ptr() % 16 == 0 and slab.data_ptr() % 16 != 0
        return slab


@pytest.fixture(scope="module")
def devices(oracle):
    cache = {}

    def get(name, t_bits=None):
        if (name, t_bits) not in cache:
            cache[name, t_bits] = Device(oracle, name, t_bits)
        return cache[name, t_bits]

    return get


def both_forms(dev, run, data, *args):
    """run() on the aligned slab (two or four words per lane where the kernel has such a form) and on the shifted one."""
    aligned = dev.down(run(dev.up(data), *args))
    assert np.array_equal(aligned, dev.down(run(dev.shifted(data), *args)).reshape(aligned.shape))
    return aligned


@pytest.mark.parametrize("name", WIDE + NARROW)
def test_lift_at_the_mtilde_threshold(devices, name):
    dev = devices(name)
    for L, level in dev.levels.items():
        threshold = cases.lift_threshold_columns(level, seed=100 + L)
        integers, _ = cases.lift_integer_columns(level)
        data = np.stack([rows(threshold, dev.degree), rows(integers, dev.degree)])
        expected = np.stack([expected_rows(threshold, dev.degree, level.lift), expected_rows(integers, dev.degree, level.lift)])
        assert np.array_equal(both_forms(dev, dev.ours.lift_q_to_qbsk, data, L), expected), (name, L)


@pytest.mark.parametrize("name", WIDE + NARROW)
def test_floor_at_the_alpha_threshold(devices, name):
    dev = devices(name)
    for L, level in dev.levels.items():
        threshold = cases.floor_threshold_columns(level, seed=200 + L)
        integers = cases.floor_integer_columns(level, seed=250 + L)
        data = np.stack([rows(threshold, dev.degree), rows(integers, dev.degree)])
        expected = np.stack([expected_rows(threshold, dev.degree, level.floor), expected_rows(integers, dev.degree, level.floor)])
        assert np.array_equal(both_forms(dev, dev.ours.floor_qbsk_to_q, data, L), expected), (name, L)


@pytest.mark.parametrize("name", WIDE + NARROW)
def test_scale_and_round_at_the_gamma_threshold(devices, name):
    dev = devices(name)
    for L, level in dev.levels.items():
        threshold = cases.scale_threshold_columns(level, seed=300 + L)
        genuine, messages = cases.scale_genuine_columns(level, seed=350 + L)
        data = np.stack([rows(threshold, dev.degree), rows(genuine, dev.degree)])
        for factor in (1, 2, level.t - 1):
            restate = lambda x: level.scale_and_round(x, factor)
            expected = np.concatenate([expected_rows(threshold, dev.degree, restate), expected_rows(genuine, dev.degree, restate)])
            got = dev.down(dev.ours.scale_and_round(dev.up(data), factor, moduli_count=L))
            assert np.array_equal(got, expected), (name, L, factor)
            if level.noise_bound_applies():
                assert got[1, :cases.DISTINCT].tolist() == [m * factor % level.t for m in messages], (name, L, factor)


@pytest.mark.parametrize("name,t_bits", [("q40x3", 17), ("q60x8", 41), ("q60x8", 60), ("w32_27_28_28_n64", 10),
                                         ("w32_27_28_28_n1024", 17)])
def test_add_plain_on_both_sides_of_the_fix_up(devices, name, t_bits):
    dev = devices(name, t_bits)
    rng = random.Random(500 + t_bits)
    for L, level in dev.levels.items():
        messages = cases.translate_messages(level, dev.degree)
        assert {level.plaintext_translate([0] * L, m)[1] for m in messages} == {False, True}
        c0 = [[rng.randrange(qi) for qi in level.q] for _ in range(dev.degree)]
        for polys in (2, 3):
            ct = np.full((1, polys, L, dev.degree), 7, dtype=np.uint64)
            ct[0, 0] = np.array(cases.columns_to_rows(c0), dtype=np.uint64)
            for subtract in (False, True):
                expected = ct.copy()
                expected[0, 0] = np.array(cases.columns_to_rows(
                    [level.plaintext_translate(c, m, subtract)[0] for c, m in zip(c0, messages)]), dtype=np.uint64)
                got = dev.ours.add_plain_(dev.up(ct), dev.up(np.array([messages], dtype=np.uint64)), polys, subtract, moduli_count=L)
                assert np.array_equal(dev.down(got), expected), (name, L, polys, subtract)


@pytest.mark.parametrize("name", WIDE + NARROW)
def test_mod_switch_at_the_q_last_threshold(devices, name):
    """One step from every level (the unrolled kernel for 2..8 moduli, the rolled one for 9, the 4-byte one), through the
    PolyContext entry and through modSwitchDown on two polynomials; then the chain to a single modulus."""
    dev = devices(name)
    narrow = SETS[name][1] == 32
    for L in range(2, dev.ours.L + 1):
        moduli = dev.levels[L].q
        columns, integers = cases.mod_switch_columns(moduli, seed=400 + L)
        expected = rows([[cases.divide_and_round_q_last(x, moduli)[0] % m for m in moduli[:-1]] for x in integers], dev.degree)
        data = rows(columns, dev.degree)
        poly_ctx = dev.ours.ciphertext_context(L)
        step = poly_ctx.divide_and_round_q_last_u32 if narrow else poly_ctx.divide_and_round_q_last
        assert np.array_equal(dev.down(step(dev.up(data)))[0], expected), (name, L)
        pair = np.stack([data, np.roll(data, 1, axis=1)])[None]  # the second polynomial: every case on the other lane of its pair
        got = dev.down(dev.ours.mod_switch_down(dev.up(pair), 2, L))
        assert np.array_equal(got[0, 0], expected) and np.array_equal(got[0, 1], np.roll(expected, 1, axis=1)), (name, L)
        columns, integers = cases.mod_switch_chain_columns(moduli, seed=450 + L)
        finals = rows([[cases.mod_switch_chain(x, moduli)[0] % moduli[0]] for x in integers], dev.degree)
        chain = rows(columns, dev.degree)
        pair = np.stack([chain, np.roll(chain, 1, axis=1)])[None]
        if not narrow:  # (modSwitchDownToSingle has 8-byte slabs only)
            got = heamd.to_host(dev.ours.mod_switch_down_to_single(heamd.to_device(pair), 2, L))
            assert np.array_equal(got[0, 0], finals) and np.array_equal(got[0, 1], np.roll(finals, 1, axis=1)), (name, L)
        lower = dev.up(pair)
        for count in range(L, 1, -1):
            lower = dev.ours.mod_switch_down(lower, 2, count)
        assert np.array_equal(dev.down(lower)[0, 0], finals), (name, L)


def _lift_ciphertexts(level, degree, batch, seed):
    """[batch][2][L][N] ciphertexts whose every coefficient is a lift construction: two polynomials on the r thresholds,
    one of structured integers, rotated along the polynomial from item to item."""
    base = [rows(cases.lift_threshold_columns(level, seed), degree), rows(cases.lift_threshold_columns(level, seed + 1), degree),
            rows(cases.lift_integer_columns(level)[0], degree)]
    return np.stack([np.stack([np.roll(base[(item + c) % 3], item, axis=1) for c in range(2)]) for item in range(batch)])


@pytest.mark.parametrize("name", ["q40x3", "q62_62_61", "q60x8", "w32_27_28_28_n64"])
def test_mul_on_lift_thresholds(oracle, devices, name):
    """ct x ct is where the production lift runs (both operands in one launch, strided records, the Bsk rows handed on
    unfolded, the loads fused into the forward transform).  Expected words: the oracle's, which the CPU tests hold to the
    restatement on these same lift inputs."""
    dev = devices(name)
    for L in (dev.ours.L, 1):
        level = dev.levels[L]
        lhs, rhs = _lift_ciphertexts(level, dev.degree, 3, seed=600 + L), _lift_ciphertexts(level, dev.degree, 3, seed=610 + L)
        got = dev.down(dev.ours.mul(dev.up(lhs), dev.up(rhs), L))
        assert np.array_equal(got, dev.ref.mul(lhs, rhs, L)), (name, L)


@pytest.mark.parametrize("level", [None, 2])
def test_row_fused_mul_on_lift_thresholds(oracle, monkeypatch, level):
    """The same through the row-fused kernels of behz_kernels.hip (N = 4096, batches past HEAMD_BEHZ_FUSED_ABOVE rows)."""
    from conftest import host_threads

    monkeypatch.setenv("HEAMD_BEHZ_FUSED_ABOVE", "256")
    degree, t = 4096, 557057
    q = oracle.generate_primes([55] * 4, False, degree)
    ours, ref = heamd.BfvContext(degree, t, q), oracle.BfvContext(degree, t, q)
    L = ours.L if level is None else level
    tool = cases.Level(q[:L], ref.rns_tool(ref.L).bsk, t, cases.GAMMA[64], cases.MTILDE[64])
    batch = 256 // (2 * L + 1) + 2
    lhs, rhs = _lift_ciphertexts(tool, degree, batch, seed=620 + L), _lift_ciphertexts(tool, degree, batch, seed=630 + L)
    got = heamd.to_host(ours.mul(heamd.to_device(lhs), heamd.to_device(rhs), L))
    assert np.array_equal(got, ref.mul(lhs, rhs, L, threads=host_threads()))


@pytest.mark.parametrize("name", ["q55x4", "q61_33_62_45", "w32_27_28_28_n64"])
def test_key_switch_finish_at_the_q_ks_threshold(oracle, devices, name):
    """relinearize / applyGalois end in divideAndRoundQLast by the key-switching modulus.  With a key whose special-modulus
    row is the Eval form of the constant 1 in key[0] and zero in the others, the product's special-modulus word at
    coefficient k is c2_0[k] mod q_ks (the inner product of Bfv+Keys.swift:180-202 leaves row 0 of the target alone there),
    so row 0 of the target carries the six remainders straight into the finish kernel's comparison."""
    dev = devices(name)
    ours, ref, n, L = dev.ours, dev.ref, dev.degree, dev.ours.L
    q, q_ks = ref.coefficient_moduli[:L], ref.coefficient_moduli[L]
    # q55x4 (equal sizes, the primes come largest first): q_0 > q_ks and all six remainders are there.  The other two: q_0 < q_ks,
    # and a remainder of q_0 or more cannot be the word of a row mod q_0 -- q_ks - 1 always, floor(q_ks/2) + 1 too under the
    # 61-bit q_0; those are left out (0, 1, floor(q_ks/2) - 1 and floor(q_ks/2) stay)
    assert (q[0] > q_ks) == (name == "q55x4")
    remainders = [h for h in cases.q_last_remainders(q_ks) if h < q[0]]
    assert len(remainders) == 6 if q[0] > q_ks else 4 <= len(remainders) < 6
    rng = np.random.default_rng(700 + L)
    picks = cases.cycled(len(remainders), n)
    uniform = lambda prefix, moduli: np.stack([rng.integers(0, m, size=prefix + (n,), dtype=np.uint64) for m in moduli], axis=len(prefix))
    key = uniform((L, 2), q + [q_ks])
    key[:, :, L, :] = 0
    key[0, :, L, :] = 1
    ct = uniform((2, 3), q)
    for item in range(2):  # the remainders on the last polynomial of a three-polynomial ciphertext, and on the other lane in item 1
        ct[item, 2, 0] = np.roll(np.array([remainders[i] for i in picks], dtype=np.uint64), item)
    # the claim above, from the oracle's own single-modulus transform: (c2_0 mod q_ks) x 1 in Eval form, back in Coeff form
    special = oracle.PolyContext(n, [q_ks])
    word = special.inverse_ntt(special.mul(special.forward_ntt(ct[0, 2, :1] % np.uint64(q_ks)), key[0, 0, L:]))
    assert word[0].tolist() == [remainders[i] for i in picks]
    relin = dev.down(ours.relinearize(dev.up(ct), dev.up(key)))
    assert np.array_equal(relin, ref.relinearize(ct, key)), name
    # applyGalois switches c1 after the automorphism: put the remainders where element 3 takes them from
    pair = uniform((2, 2), q)
    for item in range(2):
        wanted = np.roll(np.array([remainders[i] for i in picks], dtype=np.uint64), item)
        source = np.zeros(n, dtype=np.uint64)
        for k in range(n):  # coefficient k goes to 3k mod 2N, negated past N (PolyRq/Galois.swift:115-143)
            j = 3 * k % (2 * n)
            source[k] = wanted[j] if j < n else (q[0] - wanted[j - n]) % q[0]
        pair[item, 1, 0] = source
    moved = ref.ciphertext_context().apply_galois(pair[:, 1], 3)
    assert moved[0, 0].tolist() == [remainders[i] for i in picks]
    expected = ref.apply_galois(pair, 3, key)
    assert np.array_equal(dev.down(ours.apply_galois(dev.up(pair), 3, dev.up(key))), expected), name
    in_place, device_key = dev.up(pair), dev.up(key)
    entry = heamd.load_library().he_bfv_apply_galois_device_u32 if SETS[name][1] == 32 else heamd.load_library().he_bfv_apply_galois_device
    ptr = ctypes.c_void_p(in_place.data_ptr())
    assert entry(ours.h, L, ptr, 3, ctypes.c_void_p(device_key.data_ptr()), ptr, 2, None, 0, None) == 0
    assert np.array_equal(dev.down(in_place), expected), name
