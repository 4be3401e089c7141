"""The pointer contract of include/he_amd.h on the device (tests/aliasing_cases.py is the table, tests/test_aliasing_contract.py
its host-only half).

Three things run here.  The aliasing forms the contract ALLOWS, word for word against the CPU oracle: an in-place entry with
its operand at the slab it updates (x + x, x - x, x * x, a ciphertext times its own first polynomial), read-only operands that
are one slab (ct x ct of a ciphertext with itself, small and row-fused, <v, v>, a left vector that is an item of the right
one, the secret key as its own current key) and the no-op exception of modSwitchDownToSingle.  The refusals no host-only
context reaches -- the `_u32` twins, whose polynomial layer looks at the device first, and the entries that take the word as
an argument, at 32 -- with every slab inside one allocation, so that a missing check would store inside it and fail the
comparison behind the calls instead of faulting.  And the accepted forms of the entries that have no context.

No test launches a form the contract refuses.
"""

import numpy as np
import pytest

import aliasing_cases as A
import heamd

pytestmark = pytest.mark.gpu

INVALID, OK = 16, 0
# (degree, bits of the ciphertext moduli + the key-switching modulus, batch): less than a wavefront; several workgroups and
# an odd row count for the kernels that take rows in pairs
SHAPES = {64: [(8, (40, 41, 41), 3), (4096, (55, 55, 55, 55), 5)],
          32: [(8, (27, 28, 28), 3), (4096, (27, 28, 28, 29), 5)]}
CASES = [(bits, shape) for bits in (64, 32) for shape in SHAPES[bits]]
IDS = ["u%d-N%d" % (bits, shape[0]) for bits, shape in CASES]


def _slab(rng, prefix, moduli, degree):
    """[*prefix][L][N] uniform below each row's modulus, the first item's rows all 0 and the last item's all q - 1"""
    rows = [rng.integers(0, q, size=tuple(prefix) + (degree,), dtype=np.uint64) for q in moduli]
    slab = np.ascontiguousarray(np.stack(rows, axis=len(prefix)))
    slab[0] = 0
    slab[-1] = np.array(moduli, dtype=np.uint64)[:, None] - np.uint64(1)
    return slab


def _io(bits):
    return (heamd.to_device32, heamd.to_host32) if bits == 32 else (heamd.to_device, heamd.to_host)


def _scheme(oracle, bits, degree, q_bits):
    q = oracle.generate_primes(list(q_bits), False, degree, word_bits=bits)
    t = oracle.generate_primes([17], True, degree, word_bits=bits)[0]
    ours = heamd.BfvContext32(degree, t, q) if bits == 32 else heamd.BfvContext(degree, t, q)
    return ours, oracle.BfvContext(degree, t, q, word_bits=bits), q[:-1]


# ---- rule 2: the operand of an in-place entry at the slab it updates ----------------------------------------------------------
@pytest.mark.parametrize("bits,shape", CASES, ids=IDS)
def test_elementwise_operand_is_the_updated_slab(oracle, bits, shape):
    degree, q_bits, batch = shape
    moduli = oracle.generate_primes(list(q_bits[:-1]), False, degree, word_bits=bits)
    ours, ref = heamd.PolyContext(degree, moduli), oracle.PolyContext(degree, moduli)
    dev, host = _io(bits)
    x = _slab(np.random.default_rng(degree + bits), (batch,), moduli, degree)
    run = (lambda op, slab: ours.elementwise_u32_(op, slab, slab)) if bits == 32 else (
        lambda op, slab: {"add": ours.add_, "sub": ours.sub_, "mul": ours.mul_}[op](slab, slab))
    assert np.array_equal(host(run("add", dev(x))), ref.add(x, x))
    assert not host(run("sub", dev(x))).any()
    assert np.array_equal(host(run("mul", dev(x))), ref.mul(x, x))


@pytest.mark.parametrize("bits,shape", CASES, ids=IDS)
def test_mul_plain_by_the_ciphertexts_own_polynomial(oracle, bits, shape):
    """pt == ct: one ciphertext times its own c0 (c0 <- c0 c0, c1 <- c1 c0 with the c0 that came in), and `batch` one-polynomial
    ciphertexts squared; more ciphertexts of more polynomials are refused (ciphertext b's plaintext is then a polynomial that
    another lane updates) and leave the slab as it was"""
    degree, q_bits, batch = shape
    ours, ref, moduli = _scheme(oracle, bits, degree, q_bits)
    dev, host = _io(bits)
    rng = np.random.default_rng(degree + bits + 1)
    one = _slab(rng, (1, 2), moduli, degree)
    one[0, 1] = _slab(rng, (3,), moduli, degree)[1]
    ct = dev(one)
    assert np.array_equal(host(ours.mul_plain_(ct, ct[0, 0], 2)), ref.mul_plain(one, one[0, 0], 2))
    squares = _slab(rng, (batch, 1), moduli, degree)
    ct = dev(squares)
    assert np.array_equal(host(ours.mul_plain_(ct, ct.view(batch, len(moduli), degree), 1)),
                          ref.mul_plain(squares, squares.reshape(batch, len(moduli), degree), 1))
    many = _slab(rng, (batch, 2), moduli, degree)
    ct = dev(many)
    with pytest.raises(heamd.HeError) as err:
        ours.mul_plain_(ct, ct.view(-1)[: batch * len(moduli) * degree], 2)
    assert err.value.name == "invalidArgument" and "ct overlaps pt" in str(err.value)
    assert np.array_equal(host(ct), many)


# ---- rule 1: read-only operands that are one slab ------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,shape", CASES, ids=IDS)
def test_products_of_a_slab_with_itself(oracle, bits, shape):
    """ct x ct of every ciphertext with itself, <v, v>, and inner products whose left vector is an item of the right one"""
    degree, q_bits, batch = shape
    ours, ref, moduli = _scheme(oracle, bits, degree, q_bits)
    dev, host = _io(bits)
    rng = np.random.default_rng(degree + bits + 2)
    x = _slab(rng, (batch, 2), moduli, degree)
    ct = dev(x)
    assert np.array_equal(host(ours.mul(ct, ct)), ref.mul(x, x))
    assert np.array_equal(host(ours.inner_product(ct, ct)), ref.inner_product(x, x))
    assert np.array_equal(host(ct), x)
    items = _slab(rng, (3, batch, 2), moduli, degree)
    rhs = dev(items)
    got = host(ours.inner_product_shared(rhs[1], rhs))  # lhs lies inside rhs
    assert np.array_equal(got, np.stack([ref.inner_product(items[1], item) for item in items]))


def test_row_fused_square_equals_the_product_with_a_copy(oracle):
    """the smallest batch whose ct x ct takes the row-fused kernels with the Q band on the context's side lane: both operands one
    slab -- every item equal to the same call on a separate copy of the operand, the first and the last (rows of 0, rows of
    q - 1) equal to the oracle's"""
    import torch

    degree, batch = 4096, 512
    ours, ref, moduli = _scheme(oracle, 64, degree, (55, 55, 55))
    assert batch * ours.L >= 1024 and (batch - 1) * ours.L < 1024
    x = _slab(np.random.default_rng(97), (batch, 2), moduli, degree)
    ct = heamd.to_device(x)
    squared = ours.mul(ct, ct)
    assert torch.equal(squared, ours.mul(ct, ct.clone()))
    ends = x[[0, batch - 1]]
    assert np.array_equal(heamd.to_host(squared[[0, batch - 1]]), ref.mul(ends, ends))
    assert np.array_equal(heamd.to_host(ct[[0, batch - 1]]), ends)


@pytest.mark.parametrize("bits", [64, 32])
def test_the_secret_key_as_its_own_current_key(oracle, bits):
    """he_bfv_generate_key_switch_keys_device reads both: one slab for the two gives the words two slabs give"""
    import torch

    degree = 64
    ours, _, _ = _scheme(oracle, bits, degree, (27, 28, 28))
    generator = torch.Generator().manual_seed(5)
    seeds = lambda count: torch.randint(0, 256, (count, 32), dtype=torch.uint8, generator=generator).cuda()  # noqa: E731
    secret = ours.generate_secret_key(seeds(1))[0]
    a_seeds, error_seeds = seeds(ours.L), seeds(ours.L)
    aliased = ours.generate_key_switch_keys(secret, secret, a_seeds, error_seeds)
    assert torch.equal(aliased, ours.generate_key_switch_keys(secret, secret.clone(), a_seeds, error_seeds))
    assert aliased.shape[:2] == (1, ours.L) and bool(aliased.any())


# ---- rule 3: the exception that is not tested elsewhere, and ct x ct's refusal -------------------------------------------------
def test_mod_switch_down_to_single_at_one_modulus_in_place(oracle):
    """already there: out == in is accepted and leaves the ciphertexts as they were (the reference's loop runs no step), another
    out gets a copy, and an out that overlaps in otherwise is refused"""
    degree, batch = 8, 3
    ours, _, moduli = _scheme(oracle, 64, degree, (40, 41, 41))
    lib = heamd.load_library()
    x = _slab(np.random.default_rng(8), (batch, 2), moduli[:1], degree)
    ct = heamd.to_device(x)
    single = lib.he_bfv_mod_switch_down_to_single_device
    assert single(ours.h, 1, 2, ct.data_ptr(), ct.data_ptr(), batch, None) == OK
    assert np.array_equal(heamd.to_host(ct), x)
    assert np.array_equal(heamd.to_host(ours.mod_switch_down_to_single(ct, 2, moduli_count=1)), x)
    assert single(ours.h, 1, 2, ct.data_ptr(), ct.data_ptr() + 8, batch - 1, None) == INVALID
    assert "out overlaps in" in lib.he_last_error_message().decode()
    assert np.array_equal(heamd.to_host(ct), x)


@pytest.mark.parametrize("bits", [64, 32])
def test_mul_refuses_an_output_over_an_operand(oracle, bits):
    """he_bfv_mul_device: out over lhs and out over rhs at the three overlap positions, whatever the other operand; nothing
    is launched; abutting slabs give the oracle's product"""
    import torch

    degree, batch = 8, 3
    ours, ref, moduli = _scheme(oracle, bits, degree, SHAPES[bits][0][1])
    dev, host = _io(bits)
    lib = heamd.load_library()
    mul = getattr(lib, "he_bfv_mul_device" + ("_u32" if bits == 32 else ""))
    w = bits // 8
    x = _slab(np.random.default_rng(bits), (batch, 2), moduli, degree)
    operand_bytes, out_bytes = x.size * w, x.size // 2 * 3 * w
    arena = torch.zeros((out_bytes + operand_bytes + out_bytes) // w, dtype=dev(x).dtype, device="cuda")
    middle = arena[out_bytes // w: (out_bytes + operand_bytes) // w]
    middle.copy_(dev(x).view(-1))
    other = dev(x)
    before = arena.clone()
    at = middle.data_ptr()
    for name, args in (("lhs", lambda out: (at, other.data_ptr(), out)), ("rhs", lambda out: (other.data_ptr(), at, out)),
                       ("lhs", lambda out: (at, at, out))):
        for out in (at, at + operand_bytes - 1, at - out_bytes + 1):
            assert mul(ours.h, ours.L, *args(out), batch, None, 0, None) == INVALID, (name, out - at)
            assert "ct x ct: out overlaps " + name in lib.he_last_error_message().decode()
    torch.cuda.synchronize()
    assert torch.equal(arena, before)
    for out in (at + operand_bytes, at - out_bytes):  # abutting behind and before the operand
        assert mul(ours.h, ours.L, at, at, out, batch, None, 0, None) == OK
        product = arena[(out - arena.data_ptr()) // w:][: out_bytes // w].reshape(batch, 3, len(moduli), degree)
        assert np.array_equal(host(product), ref.mul(x, x))
    assert np.array_equal(host(middle).reshape(x.shape), x)


# ---- the refusals no host-only context reaches ------------------------------------------------------------------------------------
GAP = 1 << 14  # slab i of a call lies GAP (i + 1) bytes into the arena; no slab of the small ring is half as long
FOUR_BYTE = [row for row in A.CASES if row.words in ("twin", "arg") and row.ring == "small"]


@pytest.fixture(scope="module")
def device_contexts(oracle):
    degree, bits = A.RINGS["small"]
    moduli = oracle.generate_primes(list(bits), False, degree, word_bits=32)
    t = oracle.generate_primes([A.PLAINTEXT_BITS], True, degree, word_bits=32)[0]
    return {("poly", 32): heamd.PolyContext(degree, moduli), ("poly", 64): heamd.PolyContext(degree, moduli),
            ("bfv", 32): heamd.BfvContext32(degree, t, moduli), ("bfv", 64): heamd.BfvContext(degree, t, moduli)}, moduli


@pytest.mark.parametrize("row", FOUR_BYTE, ids=lambda row: row.name)
def test_four_byte_forms_refuse_overlaps(device_contexts, row):
    """status and text for every (written slab, other slab) of the `_u32` twin, or of the entry at word_bits 32: the same
    first byte unless the table allows it, first byte on last, last byte on first -- and not one byte of the arena changes"""
    import torch

    contexts, moduli = device_contexts
    lib = heamd.load_library()
    name = row.name + "_u32" if row.words == "twin" else row.name
    handle = contexts[row.context, 32].h
    variants = [{}] + [need for _, _, need in row.same if need]
    arena = torch.full((GAP * (len(row.slabs) + 2),), 0x5A, dtype=torch.uint8, device="cuda")
    calls = 0
    for overrides in variants:
        env = A.environment(row, moduli, 4, overrides)
        sizes = A.slab_bytes(row, env)
        assert all(0 < size < GAP // 2 for size in sizes.values()), sizes
        apart = {slab: arena.data_ptr() + GAP * (i + 1) for i, slab in enumerate(sizes)}
        for written, other in A.pairs(row):
            refused, _ = A.overlap_positions(apart[other], sizes[other], sizes[written])
            for position, address in refused.items():
                if position == "same" and A.may_be_same(row, written, other, overrides):
                    continue  # (allowed: it would launch; the forms above run those that matter on real operands)
                status, text = A.invoke(lib, row, name, handle, env, dict(apart, **{written: address}))
                assert status == INVALID, (name, overrides, written, other, position, text)
                assert "overlaps" in text and all(row.says.get(n, n) in text for n in (written, other)), (name, text)
                calls += 1
    assert calls >= 2
    torch.cuda.synchronize()
    assert bool((arena == 0x5A).all())


@pytest.mark.parametrize("row", [row for row in A.CASES if row.zero is not None and row.ring == "small"], ids=lambda row: row.name)
def test_empty_calls_with_one_address_for_every_slab_are_no_ops(device_contexts, row):
    """a batch of 0 overlaps nothing, both words: HE_OK, and the memory behind the address is left alone"""
    import torch

    contexts, moduli = device_contexts
    lib = heamd.load_library()
    memory = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    for word_bytes in (8, 4) if row.words != 64 else (8,):
        name = row.name + "_u32" if (row.words == "twin" and word_bytes == 4) else row.name
        handle = contexts[row.context, 8 * word_bytes].h if row.context is not None else None
        env = A.environment(row, moduli, word_bytes, {row.zero: 0})
        env["workspace_bytes"] = memory.numel()
        status, text = A.invoke(lib, row, name, handle, env, {slab: memory.data_ptr() for slab in row.slabs})
        assert status == OK, (name, text)
    torch.cuda.synchronize()
    assert bool((memory == 0x5A).all())


# ---- the word-size bridge: no context, so its accepted forms run on memory -----------------------------------------------------
def test_word_bridge_takes_abutting_slabs():
    import torch

    lib = heamd.load_library()
    words = 24
    values = torch.arange(1, words + 1, dtype=torch.int32, device="cuda") * 0x01010101
    for out_first in (False, True):
        arena = torch.zeros(3 * words, dtype=torch.int32, device="cuda")  # 4 w bytes of input beside 8 w of output
        narrow, wide = (arena[2 * words:], arena[: 2 * words]) if out_first else (arena[:words], arena[words:])
        narrow.copy_(values)
        assert narrow.data_ptr() % 16 == 0 and wide.data_ptr() % 16 == 0
        assert lib.he_words_widen_u32_device(narrow.data_ptr(), wide.data_ptr(), words, None) == OK
        assert torch.equal(wide.view(torch.int64), values.to(torch.int64))
        narrow.zero_()
        assert lib.he_words_narrow_u64_device(wide.data_ptr(), narrow.data_ptr(), words, None) == OK
        assert torch.equal(narrow, values)
    pair = torch.zeros(2 * words, dtype=torch.int64, device="cuda")
    pair[:words] = values.to(torch.int64)
    for non_temporal in (0, 1):
        pair[words:].zero_()
        assert lib.he_words_copy_device(pair.data_ptr(), pair[words:].data_ptr(), words, non_temporal, None) == OK
        assert torch.equal(pair[words:], pair[:words])
    # one word in: the ranges share bytes
    assert lib.he_words_copy_device(pair.data_ptr(), pair[words - 1:].data_ptr(), words, 0, None) == INVALID
    assert "device_out overlaps device_in" in lib.he_last_error_message().decode()
