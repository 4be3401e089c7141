"""Every grid-stride loop takes several trips: each strided kernel of csrc/ runs with HEAMD_GRID_CAP = 1 and = 3 (csrc/launch_grid.hpp)
and its result is compared word for word with the CPU oracle -- the same oracle that decides the uncapped launches everywhere else in
this suite, so agreement with it is agreement with the uncapped run.

ROWS is the table: one row per wrapper call, naming the kernels it reaches (tests/test_launch_grid.py scans csrc/ and fails when a
kernel that strides by gridDim.x is missing here).  Shapes are the smallest at which a second trip can go wrong: with 256-lane
workgroups a kernel needs more than 2 x 3 x 256 items for every lane to make two trips at cap 3 (and then makes six at cap 1), a count
that is no multiple of 256 leaves the last trip ragged, degree 64 puts several rows and moduli into one trip, degree 1024 spreads a row
over several trips, three moduli keep the modulus index out of step with the trips, and every slab holds 0 and q - 1 in its first and
last words.  Kernels whose item count is fixed by the ring (one polynomial of L x N words) cannot be ragged at degree 1024; their
degree-64 case is, and a row says so where it matters.

The kernels of rns_kernels.hip that take exactly one item per lane (lift, floor, scaleAndRound, plaintext translate) have no loop; they
are in the table all the same, under SINGLE_TRIP: a cap that reached their grids would leave items uncovered, and these rows would fail.
"""
import ctypes

import numpy as np
import pytest

import heamd

pytestmark = pytest.mark.gpu

LANES = 256
BITS = [40, 45, 50]  # three moduli


def units(items_per_unit, lanes=LANES):
    """Smallest count of units (polynomials, ciphertexts, ...) whose items give every lane two trips at cap 3, hence six at cap 1,
    with a ragged last trip where the unit size allows one."""
    count = 2
    while True:
        total = count * items_per_unit
        ragged3 = items_per_unit % (3 * lanes) == 0 or total % (3 * lanes) != 0
        ragged1 = items_per_unit % lanes == 0 or total % lanes != 0
        if total > 2 * 3 * lanes and ragged3 and ragged1:
            return count
        count += 1


def uniform(rng, shape_prefix, moduli, degree):
    """uint64 [*shape_prefix][L][N], row i uniform below moduli[i]; 0 and q - 1 in the first and last words of the slab."""
    rows = [rng.integers(0, q, size=tuple(shape_prefix) + (degree,), dtype=np.uint64) for q in moduli]
    slab = np.ascontiguousarray(np.stack(rows, axis=len(shape_prefix)))
    flat = slab.reshape(-1, len(moduli), degree)
    flat[0, :, 0] = 0
    flat[0, :, -1] = [m - 1 for m in moduli]
    flat[-1, :, 0] = [m - 1 for m in moduli]
    flat[-1, :, -1] = 0
    return slab


def dev32(array):
    return heamd.to_device32(array)


def host32(tensor):
    return heamd.to_host32(tensor)


# ---- the table -----------------------------------------------------------------------------------------------------------------------
# name -> (kernels reached, build): build(oracle) returns (run, expected); run() launches on the device and returns a list of host
# arrays, expected is the oracle's list.  build runs once per row (the reference is shared by both caps and never modified).
ROWS = {}
SINGLE_TRIP = ("lift_kernel", "floor_kernel", "scale_and_round_kernel", "plaintext_translate_kernel")


def row(name, *kernels):
    def register(build):
        ROWS[name] = (kernels, build)
        return build

    return register


def _poly_contexts(oracle, degree, bits=BITS, word_bits=64):
    moduli = oracle.generate_primes(bits, False, degree, word_bits=word_bits) if word_bits == 32 else \
        oracle.generate_primes(bits, False, degree)
    return moduli, heamd.PolyContext(degree, moduli), oracle.PolyContext(degree, moduli)


# -- poly_kernels.hip --
def _elementwise(oracle, degree, seed):
    moduli, ours, ref = _poly_contexts(oracle, degree)
    rng = np.random.default_rng(seed)
    batch = units(len(moduli) * degree // 2 if degree >= 2 else len(moduli))
    x, y = uniform(rng, (batch,), moduli, degree), uniform(rng, (batch,), moduli, degree)
    scalars = [int(rng.integers(0, q)) for q in moduli]
    expected = [ref.add(x, y), ref.sub(x, y), ref.neg(x), ref.mul(x, y), ref.mul_scalar(x, scalars)]
    dev, host = heamd.to_device, heamd.to_host

    def run():
        return [host(ours.add_(dev(x), dev(y))), host(ours.sub_(dev(x), dev(y))), host(ours.neg_(dev(x))),
                host(ours.mul_(dev(x), dev(y))), host(ours.mul_scalar_(dev(x), scalars))]

    return run, expected


@row("elementwise-64", "elementwise_kernel")
def _(oracle):
    return _elementwise(oracle, 64, 1)


@row("elementwise-1024", "elementwise_kernel")
def _(oracle):
    return _elementwise(oracle, 1024, 2)


@row("elementwise-degree-1", "elementwise_scalar_kernel")
def _(oracle):
    return _elementwise(oracle, 1, 3)


def _bfv(oracle, degree, bits=(40, 45, 50, 51), t_bits=17, packed=False):
    if packed:
        t = oracle.generate_primes([10 if degree <= 64 else 14], True, degree, word_bits=32)[0]
        q = oracle.generate_primes([27, 28, 28, 29], False, degree, word_bits=32)
        return heamd.BfvContext32(degree, t, q), oracle.BfvContext(degree, t, q, word_bits=32)
    t = oracle.generate_primes([t_bits], True, degree)[0]
    q = oracle.generate_primes(list(bits), False, degree)
    return heamd.BfvContext(degree, t, q), oracle.BfvContext(degree, t, q)


def _mul_plain(oracle, degree, packed, seed):
    ours, ref = _bfv(oracle, degree, packed=packed)
    moduli = ref.ciphertext_context().moduli
    rng = np.random.default_rng(seed)
    batch = units(len(moduli) * degree // (1 if packed else 2))
    cts, pts = uniform(rng, (batch, 2), moduli, degree), uniform(rng, (batch,), moduli, degree)
    expected = [ref.mul_plain(cts, pts, 2)]
    dev, host = (dev32, host32) if packed else (heamd.to_device, heamd.to_host)
    return (lambda: [host(ours.mul_plain_(dev(cts), dev(pts), 2))]), expected


@row("mul-plain-64", "mul_plain_kernel")
def _(oracle):
    return _mul_plain(oracle, 64, False, 4)


@row("mul-plain-1024", "mul_plain_kernel")
def _(oracle):
    return _mul_plain(oracle, 1024, False, 5)


@row("mul-plain-u32-64", "mul_plain_kernel32")
def _(oracle):
    return _mul_plain(oracle, 64, True, 6)


@row("mul-plain-u32-1024", "mul_plain_kernel32")
def _(oracle):
    return _mul_plain(oracle, 1024, True, 7)


def _q_last(oracle, degree, bits, seed):
    moduli, ours, ref = _poly_contexts(oracle, degree, bits)
    rng = np.random.default_rng(seed)
    x = uniform(rng, (units(degree // 2),), moduli, degree)
    x[1, -1, :4] = [0, moduli[-1] - 1, moduli[-1] // 2, moduli[-1] // 2 + 1]
    return (lambda: [heamd.to_host(ours.divide_and_round_q_last(heamd.to_device(x)))]), [ref.divide_and_round_q_last(x)]


@row("q-last-rows-64", "divide_and_round_q_last_rows_kernel")
def _(oracle):
    return _q_last(oracle, 64, BITS, 8)


@row("q-last-rows-1024", "divide_and_round_q_last_rows_kernel")
def _(oracle):
    return _q_last(oracle, 1024, BITS, 9)


@row("q-last-nine-moduli-64", "divide_and_round_q_last_kernel")
def _(oracle):
    return _q_last(oracle, 64, [40, 45, 50, 41, 46, 51, 42, 47, 52], 10)


@row("q-last-nine-moduli-1024", "divide_and_round_q_last_kernel")
def _(oracle):
    return _q_last(oracle, 1024, [40, 45, 50, 41, 46, 51, 42, 47, 52], 11)


def _to_single(oracle, degree, seed):
    ours, ref = _bfv(oracle, degree)
    moduli = ref.ciphertext_context().moduli
    rng = np.random.default_rng(seed)
    ct = uniform(rng, ((units(degree // 2) + 1) // 2, 2), moduli, degree)
    expected = ct
    for step in range(len(moduli), 1, -1):
        expected = ref.mod_switch_down(expected, poly_count=2, moduli_count=step)

    def run():
        got = heamd.to_host(ours.mod_switch_down_to_single(heamd.to_device(ct), 2))
        return [got.reshape(expected.shape)]

    return run, [expected]


@row("to-single-64", "mod_switch_down_to_single_kernel")
def _(oracle):
    return _to_single(oracle, 64, 12)


@row("to-single-1024", "mod_switch_down_to_single_kernel")
def _(oracle):
    return _to_single(oracle, 1024, 13)


@row("lazy-accumulator", "adding_lazy_product_kernel", "reduce_accumulator_kernel")
def _(oracle):
    """One polynomial of L x N words is all these launches ever take, so a count above 2 x 3 x 256 needs N >= 512 and is then a
    multiple of 256 (no ragged workgroup): N = 1024 with five moduli is 5120 words (6 2/3 trips of 3 x 256), N = 512 with five
    is 2560 (3 1/3 trips, a trip of cap 3 spans a row and a half)."""
    import torch

    cases = []
    for degree, bits in ((1024, [59, 60, 58, 57, 61]), (512, [59, 60, 58, 57, 61])):
        moduli, ours, ref = _poly_contexts(oracle, degree, bits)
        rng = np.random.default_rng(14 + degree)
        pairs = [(uniform(rng, (1,), moduli, degree)[0], uniform(rng, (1,), moduli, degree)[0]) for _ in range(3)]
        acc_ref = np.zeros((len(moduli), degree, 2), dtype=np.uint64)
        for x, y in pairs:
            ref.adding_lazy_product(x, y, acc_ref)
        wild = rng.integers(0, 1 << 63, size=(len(moduli), degree, 2), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        cases.append((ours, pairs, wild, len(moduli), degree,
                      [acc_ref.copy(), ref.reduce_accumulator(acc_ref), ref.reduce_accumulator(wild)]))

    def run():
        got = []
        for ours, pairs, wild, count, degree, _ in cases:
            acc = torch.zeros((count, degree, 2), dtype=torch.int64, device="cuda")
            for x, y in pairs:
                ours.adding_lazy_product_(heamd.to_device(x), heamd.to_device(y), acc)
            got += [heamd.to_host(acc), heamd.to_host(ours.reduce_accumulator(acc)),
                    heamd.to_host(ours.reduce_accumulator(heamd.to_device(wild)))]
        return got

    return run, [e for case in cases for e in case[5]]


# -- galois_kernels.hip --
def _permutes(oracle, degree, seed):
    moduli, ours, ref = _poly_contexts(oracle, degree)
    rng = np.random.default_rng(seed)
    slab = uniform(rng, (units(len(moduli) * degree),), moduli, degree)
    elements, powers = (3, 2 * degree - 1, degree + 1), (1, -1, degree + 1, -2 * degree + 1)
    expected = [ref.apply_galois(slab, e, eval_format=f) for e in elements for f in (False, True)]
    expected += [ref.multiply_power_of_x(slab, p) for p in powers]

    def run():
        got = [heamd.to_host(ours.apply_galois(heamd.to_device(slab), e, eval_format=f)) for e in elements for f in (False, True)]
        return got + [heamd.to_host(ours.multiply_power_of_x(heamd.to_device(slab), p)) for p in powers]

    return run, expected


@row("permutes-64", "coeff_permute_kernel", "galois_eval_kernel")
def _(oracle):
    return _permutes(oracle, 64, 20)


@row("permutes-1024", "coeff_permute_kernel", "galois_eval_kernel")
def _(oracle):
    return _permutes(oracle, 1024, 21)


def _plaintexts(oracle, degree, packed, seed):
    ours, ref = _bfv(oracle, degree, packed=packed)
    rng = np.random.default_rng(seed)
    pt = rng.integers(0, ref.t, size=(units(degree), degree), dtype=np.uint64)
    pt[0, :4] = [0, ref.t - 1, (ref.t + 1) // 2, (ref.t + 1) // 2 - 1]
    pt[-1, -2:] = [ref.t - 1, 0]
    levels = (ref.L, ref.L - 1)
    evals = [ref.plaintext_to_eval(pt, moduli_count=level) for level in levels]
    dev, host = (dev32, host32) if packed else (heamd.to_device, heamd.to_host)

    def run():
        got = [host(ours.plaintext_to_eval(dev(pt), moduli_count=level)) for level in levels]
        return got + [host(ours.plaintext_to_coeff(dev(e), moduli_count=level)) for e, level in zip(evals, levels)]

    return run, evals + [pt for _ in levels]


PLAINTEXT_KERNELS = ("plaintext_lift_kernel", "plaintext_unlift_kernel", "first_row_kernel")


@row("plaintexts-64", *PLAINTEXT_KERNELS)
def _(oracle):
    return _plaintexts(oracle, 64, False, 22)


@row("plaintexts-1024", *PLAINTEXT_KERNELS)
def _(oracle):
    return _plaintexts(oracle, 1024, False, 23)


@row("plaintexts-u32-64", *PLAINTEXT_KERNELS)
def _(oracle):
    return _plaintexts(oracle, 64, True, 24)


@row("plaintexts-u32-1024", *PLAINTEXT_KERNELS)
def _(oracle):
    return _plaintexts(oracle, 1024, True, 25)


def _expand(oracle, degree, bits, total, seed):
    """PirUtil.expand of two queries under different keys; a total that is no power of two leaves leaves above the tree's height,
    which the move table emits doubled."""
    ours, ref = _bfv(oracle, degree, bits=bits)
    q = ref.coefficient_moduli
    rng = np.random.default_rng(seed)
    shifts = range((total - 1).bit_length())
    queries = uniform(rng, (2, 1, 2), q[:-1], degree)
    keys = [{(degree >> k) + 1: uniform(rng, (ours.L, 2), q, degree) for k in shifts} for _ in range(2)]
    expected = [oracle.pir.expand(ref, queries[i], total, keys[i]) for i in range(2)]

    def run():
        device_keys = [{e: heamd.to_device(k) for e, k in keys[i].items()} for i in range(2)]
        both = heamd.to_host(ours.pir_expand_batch(heamd.to_device(queries), total, device_keys))
        return [both[0], both[1]]

    return run, expected


@row("expand-64", "expand_step_kernel", "expand_move_kernel", "coeff_permute_kernel", "key_switch_spread_kernel",
     "key_switch_finish_kernel")
def _(oracle):
    return _expand(oracle, 64, (40, 45, 50, 51), 13, 26)


@row("expand-fused-4096", "key_switch_finish_kernel")
def _(oracle):
    """a ring with a tiled transform: the children of a level leave the key switch's last kernel (its expand and Galois ends)"""
    return _expand(oracle, 4096, (50, 45, 55), 6, 27)


def _serialize(oracle, degree, bits, skips, misalign, seed):
    """misalign: None (the wrappers' own buffers) or the byte offset of the records inside a device buffer (8: the 8-byte word
    kernels at a degree that would take the tiles, 1: the byte kernels)."""
    import torch

    moduli = oracle.generate_primes(bits, False, 1)
    ours, ref = heamd.PolyContext(degree, moduli), oracle.PolyContext(degree, moduli)
    rng = np.random.default_rng(seed)
    batch = max(units(len(moduli) * degree), units(sum(m.bit_length() for m in moduli) * degree // 64))
    slab = uniform(rng, (batch,), moduli, degree)
    packed = [ref.serialize(slab, skip) for skip in skips]
    expected = packed + [ref.deserialize(p, skip) for p, skip in zip(packed, skips)]
    lib = heamd.load_library()

    def run():
        if misalign is None:
            got = [ours.serialize(heamd.to_device(slab), skip).cpu().numpy() for skip in skips]
            return got + [heamd.to_host(ours.deserialize(torch.from_numpy(p).cuda(), skip)) for p, skip in zip(packed, skips)]
        got, back = [], []
        device_slab = heamd.to_device(slab)
        for p, skip in zip(packed, skips):
            per_poly = ours.serialization_byte_count(skip)
            buffer = torch.zeros(batch * per_poly + 64, dtype=torch.uint8, device="cuda")
            view = buffer[misalign: misalign + batch * per_poly]
            assert lib.he_poly_serialize_device(ours.h, ctypes.c_void_p(device_slab.data_ptr()), batch, skip,
                                                ctypes.c_void_p(view.data_ptr()), None) == 0
            torch.cuda.synchronize()
            got.append(view.cpu().numpy().reshape(batch, per_poly))
            view.copy_(torch.from_numpy(p).reshape(-1))
            out = torch.zeros_like(device_slab)
            assert lib.he_poly_deserialize_device(ours.h, ctypes.c_void_p(view.data_ptr()), per_poly, batch, skip,
                                                  ctypes.c_void_p(out.data_ptr()), None) == 0
            torch.cuda.synchronize()
            back.append(heamd.to_host(out))
        return got + back

    return run, expected


@row("serialize-words-64", "serialize_words_kernel", "deserialize_words_kernel")
def _(oracle):
    return _serialize(oracle, 64, [62, 33, 41], (0, 2), None, 28)


@row("serialize-words-1024", "serialize_words_kernel", "deserialize_words_kernel")
def _(oracle):
    return _serialize(oracle, 1024, [62, 33, 41], (0, 2), 8, 29)


@row("serialize-bytes-32", "serialize_kernel", "deserialize_kernel")
def _(oracle):
    return _serialize(oracle, 32, [61, 33, 21], (0, 2), None, 30)


@row("serialize-bytes-1024", "serialize_kernel", "deserialize_kernel")
def _(oracle):
    return _serialize(oracle, 1024, [61, 33, 21], (0, 2), 1, 31)


# -- rns_kernels.hip (and the rest of the scheme layer's unfused path: degrees without a tiled transform) --
def _scheme(oracle, degree, packed, level_down, seed):
    ours, ref = _bfv(oracle, degree, packed=packed)
    L = ref.L - (1 if level_down else 0)
    moduli = ref.ciphertext_context(L).moduli
    tool = ref.rns_tool(L)
    rng = np.random.default_rng(seed)
    batch = units(2 * degree)
    lhs, rhs = uniform(rng, (batch, 2), moduli, degree), uniform(rng, (batch, 2), moduli, degree)
    ct3 = uniform(rng, (batch, 3), moduli, degree)
    key = uniform(rng, (ref.L, 2), ref.key_switching_context().moduli, degree)
    element = degree // 2 + 1
    x = uniform(rng, (batch,), moduli, degree)
    y = uniform(rng, (batch,), ref.qbsk_context(L).moduli, degree)
    messages = rng.integers(0, ref.t, size=(batch, degree), dtype=np.uint64)
    messages[0, :2] = [ref.t - 1, 0]
    count = 3
    left, right = uniform(rng, (count, 2), moduli, degree), uniform(rng, (2, count, 2), moduli, degree)
    expected = [ref.mul(lhs, rhs, L), ref.relinearize(ct3, key, L), ref.apply_galois(lhs, element, key, moduli_count=L),
                np.stack([tool.lift_q_to_qbsk(p) for p in x]), np.stack([tool.floor_qbsk_to_q(p) for p in y]),
                np.stack([tool.scale_and_round(p, 1) for p in x]),
                ref.plaintext_translate(lhs, messages, 2, False, moduli_count=L), ref.inner_product(left, right[0], L)]
    expected += [ref.inner_product(left, right[i], L) for i in range(2)]
    dev, host = (dev32, host32) if packed else (heamd.to_device, heamd.to_host)

    def run():
        device_key = dev(key)
        got = [host(ours.mul(dev(lhs), dev(rhs), L)), host(ours.relinearize(dev(ct3), device_key, L)),
               host(ours.apply_galois(dev(lhs), element, device_key, moduli_count=L)), host(ours.lift_q_to_qbsk(dev(x), L)),
               host(ours.floor_qbsk_to_q(dev(y), L)), host(ours.scale_and_round(dev(x), 1, moduli_count=L)),
               host(ours.add_plain_(dev(lhs), dev(messages), 2, False, moduli_count=L)),
               host(ours.inner_product(dev(left), dev(right[0]), L))]
        shared = host(ours.inner_product_shared(dev(left), dev(right), L))
        return got + [shared[0], shared[1]]

    return run, expected


SCHEME_KERNELS = ("tensor_accumulate_kernel", "key_switch_spread_kernel", "key_switch_finish_kernel", "coeff_permute_kernel") + SINGLE_TRIP


@row("scheme-64", "tensor_accumulate_shared_kernel", *SCHEME_KERNELS)
def _(oracle):
    return _scheme(oracle, 64, False, False, 40)


@row("scheme-64-level-down", "tensor_accumulate_shared_kernel", *SCHEME_KERNELS)
def _(oracle):
    return _scheme(oracle, 64, False, True, 41)


@row("scheme-1024", "tensor_accumulate_shared_kernel", *SCHEME_KERNELS)
def _(oracle):
    return _scheme(oracle, 1024, False, False, 42)


@row("scheme-1024-level-down", "tensor_accumulate_shared_kernel", *SCHEME_KERNELS)
def _(oracle):
    return _scheme(oracle, 1024, False, True, 43)


@row("scheme-u32-64", "tensor_accumulate_shared_kernel", *SCHEME_KERNELS)
def _(oracle):
    return _scheme(oracle, 64, True, False, 44)


@row("scheme-u32-64-level-down", "tensor_accumulate_shared_kernel", *SCHEME_KERNELS)
def _(oracle):
    return _scheme(oracle, 64, True, True, 45)


@row("scheme-u32-1024", "tensor_accumulate_shared_kernel", *SCHEME_KERNELS)
def _(oracle):
    return _scheme(oracle, 1024, True, False, 46)


@row("scheme-u32-1024-level-down", "tensor_accumulate_shared_kernel", *SCHEME_KERNELS)
def _(oracle):
    return _scheme(oracle, 1024, True, True, 47)


@row("shared-tensor-128", "tensor_accumulate_kernel", "tensor_accumulate_shared_kernel")
def _(oracle):
    """8-byte words reach the strided shared-left-vector kernel below degree 256 only (from there on a kernel without a loop takes
    over), and one launch covers one polynomial of (2L + 1) N words: degree 128 with six ciphertext moduli is 13 x 128 = 1664 words,
    6 1/2 workgroups -- 7 trips at cap 1, 2 1/6 at cap 3.  (4-byte words take the strided kernel at every degree: the packed scheme
    rows at degree 1024 run it over 7168 words.)"""
    degree = 128
    ours, ref = _bfv(oracle, degree, bits=(40, 45, 50, 41, 46, 51, 52))
    moduli = ref.ciphertext_context().moduli
    assert (2 * len(moduli) + 1) * degree > 2 * 3 * LANES
    rng = np.random.default_rng(48)
    count, items = 5, 3
    left, right = uniform(rng, (count, 2), moduli, degree), uniform(rng, (items, count, 2), moduli, degree)
    expected = [ref.inner_product(left, right[i]) for i in range(items)]

    def run():
        shared = heamd.to_host(ours.inner_product_shared(heamd.to_device(left), heamd.to_device(right)))
        return [shared[i] for i in range(items)] + [heamd.to_host(ours.inner_product(heamd.to_device(left), heamd.to_device(right[0])))]

    return run, expected + [expected[0]]


@row("galois-fused-4096", "key_switch_finish_kernel")
def _(oracle):
    """Bfv.applyGalois on a ring with a tiled transform and a batch too small for the transform's own store to finish the key
    switch: the Galois end of key_switch_finish_kernel (the automorphism of c0 rides its loads).  Three ciphertexts, elements that
    flip signs (N + 1), reverse (2N - 1) and scatter (3).  "Too small" is ntt_key_mac_finish_supported (ntt_routing.hip): the
    transform finishes the key switch itself only above 2 x kOneGeneration (ntt_rows.hpp) rows, and this batch has 3 x 2 x (L + 1) =
    18; should that threshold ever drop below 18 rows, this row stops reaching the kernel and needs a smaller batch."""
    degree = 4096
    ours, ref = _bfv(oracle, degree, bits=(50, 45, 55))
    q = ref.coefficient_moduli
    rng = np.random.default_rng(49)
    cts = uniform(rng, (3, 2), q[:-1], degree)
    key = uniform(rng, (ours.L, 2), q, degree)
    elements = (degree + 1, 2 * degree - 1, 3)
    expected = [ref.apply_galois(cts, element, key) for element in elements]

    def run():
        device_key = heamd.to_device(key)
        return [heamd.to_host(ours.apply_galois(heamd.to_device(cts), element, device_key)) for element in elements]

    return run, expected


# -- the 4-byte kernels of poly_kernels.hip; copy_kernels.hip --
def _word32(oracle, degree, seed):
    moduli, ours, ref = _poly_contexts(oracle, degree, [27, 28, 28], word_bits=32)
    rng = np.random.default_rng(seed)
    batch = units(degree)  # divideAndRoundQLast takes one lane per coefficient of a polynomial
    x, y = uniform(rng, (batch,), moduli, degree), uniform(rng, (batch,), moduli, degree)
    scalars = [int(rng.integers(0, q)) for q in moduli]
    expected = [ref.add(x, y), ref.sub(x, y), ref.mul(x, y), ref.neg(x), ref.mul_scalar(x, scalars), ref.divide_and_round_q_last(x)]

    def run():
        got = [host32(ours.elementwise_u32_(op, dev32(x), dev32(y))) for op in ("add", "sub", "mul")]
        return got + [host32(ours.elementwise_u32_("neg", dev32(x))), host32(ours.mul_scalar_u32_(dev32(x), scalars)),
                      host32(ours.divide_and_round_q_last_u32(dev32(x)))]

    return run, expected


@row("word32-64", "elementwise32_kernel", "divide_and_round_q_last32_kernel")
def _(oracle):
    return _word32(oracle, 64, 50)


@row("word32-1024", "elementwise32_kernel", "divide_and_round_q_last32_kernel")
def _(oracle):
    return _word32(oracle, 1024, 51)


@row("word-bridge", "widen_kernel", "narrow_kernel", "stream_copy_kernel")
def _(oracle):
    """8003 words: 2000 quads (7.8 workgroups) and a tail of three; the copies move the same words at 8 bytes per lane."""
    import torch

    x = np.random.default_rng(52).integers(0, 1 << 30, size=8003, dtype=np.uint64)
    x[[0, -1]] = [(1 << 30) - 1, 0]

    def run():
        wide = heamd.widen_u32(dev32(x))
        got = [heamd.to_host(wide), host32(heamd.narrow_u64(wide))]
        for non_temporal in (False, True):
            out = torch.zeros_like(wide)
            heamd.stream_copy(wide, out, non_temporal)
            got.append(heamd.to_host(out))
        return got

    return run, [x, x, x, x]


# -- simple_pir_kernels.hip, pnns_kernels.hip, pir_database_kernels.hip, seeded_kernels.hip --
SIMPLE_PIR_KERNELS = ("simple_pir_database_kernel", "simple_pir_widen_kernel", "simple_pir_hint_mac_kernel", "simple_pir_pack_kernel",
                      "simple_pir_unpack_kernel")


# two of the shapes of tests/test_gpu_simple_pir.py (the reference's own small database, SimplePirTests.swift:23-46), the smallest there
# whose database, staging and hint all exceed 2 x 3 x 256 elements:
# (entry_count, entry_size_in_bytes, plaintext_bits, ciphertext_bits, lattice_dimension, word_bits)
SIMPLE_PIR_SHAPES = {32: (600, 20, 7, 28, 1024, 32), 64: (600, 20, 14, 42, 1024, 64)}


def _simple_pir(oracle, word_bits, seed):
    import torch

    import simple_pir_reference as R

    entry_count, entry_size, pbits, cbits, n, _ = SIMPLE_PIR_SHAPES[word_bits]
    rng = np.random.default_rng(seed)
    entries = rng.integers(0, 256, size=(entry_count, entry_size), dtype=np.uint8)
    key = bytes(rng.integers(0, 256, size=32, dtype=np.uint8))
    params = R.shape(oracle, pbits, cbits, n, entry_count, entry_size, word_bits)
    database = R.process_database(oracle, entries, params)
    assert database.size > 2 * 3 * LANES
    hint = R.hint(params, database, R.materialize_a(params, R.a_polynomials(oracle, params, key)))
    requests = rng.integers(0, 1 << cbits, size=(3, params["database_columns"]), dtype=np.uint64)
    requests[0, 0], requests[-1, -1] = (1 << cbits) - 1, 0
    replies = R.compute_response(params, database, requests, word_bits).astype(np.uint64)
    cls = heamd.SimplePirServer if word_bits == 64 else heamd.SimplePirServer32
    dev, host = (heamd.to_device, heamd.to_host) if word_bits == 64 else (dev32, host32)

    def run():
        server = cls.process(torch.from_numpy(entries).cuda(), pbits, cbits, n, key)
        wide = server.wide_database()
        again = cls.from_wide(wide, server.hint, params)
        return [host(wide), host(server.hint), host(again.wide_database()), host(server.compute_response(dev(requests)))]

    return run, [database, hint, database, replies]


@row("simple-pir-u32", *SIMPLE_PIR_KERNELS)
def _(oracle):
    return _simple_pir(oracle, 32, 58)


@row("simple-pir-u64", *SIMPLE_PIR_KERNELS)
def _(oracle):
    return _simple_pir(oracle, 64, 59)


@row("pnns-quantize", "pnns_quantize_rows_kernel")
def _(oracle):
    """4000 rows of three columns, 16 rows per workgroup: 250 workgroups' worth of rows, no multiple of three"""
    import torch

    import pnns_reference as pnns

    ours, _ = _bfv(oracle, 64)
    context = heamd.PnnsContext(ours)
    rng = np.random.default_rng(60)
    vectors = rng.standard_normal((4000, 3)).astype(np.float32)
    vectors[5] = 0
    vectors[7] = 1e-30
    vectors[11:400] *= np.float32(1e4)
    scales = (100.0, -77.5)
    expected = [pnns.normalized_scaled_and_rounded(vectors, scale) for scale in scales]
    return (lambda: [context.quantize_rows(torch.from_numpy(vectors).cuda(), scale).cpu().numpy() for scale in scales]), expected


@row("pir-database", "pir_database_unpack_kernel")
def _(oracle):
    """the smallest database of tests/test_gpu_pir_database.py (N = 64, dimensions [5, 1], entries split over three plaintexts, the
    last slot nil): 15 slots, one workgroup per slot -- 15 trips at cap 1, 5 at cap 3"""
    import torch

    import pir_database_reference as refdb

    ours, ref = _bfv(oracle, 64, bits=(40, 40, 40, 41))
    rng = np.random.default_rng(61)
    dims, entry_size = [5, 1], 300
    sizes = np.array([entry_size, 7, 0, entry_size - 1], dtype=np.uint64)
    entries = [rng.integers(0, 256, size=int(size), dtype=np.uint8).tobytes() for size in sizes]
    padded = rng.integers(0, 256, size=(len(entries), entry_size), dtype=np.uint8)  # garbage past each entry's own size
    for index, entry in enumerate(entries):
        padded[index, :len(entry)] = np.frombuffer(entry, dtype=np.uint8)
    want_db, want_present = refdb.process(oracle, ref, entries, dims, entry_size, False)

    def run():
        database, present = ours.pir_process_database(torch.from_numpy(padded).cuda(), dims, entry_size, False, entry_sizes=sizes)
        torch.cuda.synchronize()
        return [heamd.to_host(database).reshape(want_db.shape), present.cpu().numpy()]

    return run, [want_db, want_present]


@row("seeded", "seeded_stream_kernel")
def _(oracle):
    """70 seeds of one 256-block chunk each, four chunks per workgroup: 17 1/2 workgroups"""
    import torch

    degree = 64
    moduli = oracle.generate_primes([30, 31, 33], False, degree)
    ours, ref = heamd.PolyContext(degree, moduli), oracle.PolyContext(degree, moduli)
    seeds = np.random.default_rng(62).integers(0, 256, size=(70, 32), dtype=np.uint8)
    seeds[0], seeds[-1] = 0, 255
    return (lambda: [heamd.to_host(ours.random_from_seeds(torch.from_numpy(seeds).cuda()))]), [ref.random_from_seeds(seeds)]


COVERED_KERNELS = sorted({k for kernels, _ in ROWS.values() for k in kernels} - set(SINGLE_TRIP))

_built = {}


@pytest.mark.parametrize("cap", ["1", "3"])
@pytest.mark.parametrize("name", sorted(ROWS))
def test_capped_grid_matches_oracle(oracle, monkeypatch, name, cap):
    if name not in _built:
        _built[name] = ROWS[name][1](oracle)  # with the variable unset: nothing of the reference depends on it
    run, expected = _built[name]
    if cap == "3":
        del _built[name]  # the caps of a row follow one another: its contexts and slabs do not outlive it
    monkeypatch.setenv("HEAMD_GRID_CAP", cap)
    got = run()
    assert len(got) == len(expected)
    for index, (ours, want) in enumerate(zip(got, expected)):
        ours, want = np.asarray(ours), np.asarray(want)
        assert ours.shape == want.shape, (name, cap, index, ours.shape, want.shape)
        if not np.array_equal(ours, want):
            first = int(np.flatnonzero(ours.reshape(-1) != want.reshape(-1))[0])
            pytest.fail(f"{name} at HEAMD_GRID_CAP={cap}: result {index} differs from the oracle first at flat word {first} of "
                        f"{want.size} (shape {want.shape}): {ours.reshape(-1)[first]} != {want.reshape(-1)[first]}")
