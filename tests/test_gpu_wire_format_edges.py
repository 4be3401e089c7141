"""The wire-format path on inputs no random test reaches, word for word against the oracle and against
tests/wire_format_reference.py (Python integers; tests/test_wire_format_reference.py holds the oracle to it at these inputs):

  D1  seeds whose DRBG counter V_0 sits just below a 2^32, 2^64, 2^96 or 2^128 boundary, so that the counter additions of
      csrc/seeded_kernels.hip (stream V + 1 + 4 lane + j, chain V + 256, re-key V + 257 / V + 258) carry into every upper word;
  D2  SimplePIR's process, whose A is ONE stream over several polynomials, from two such seeds;
  D3  deserialize on bytes that no serializer wrote: all-0xFF and random records (fields at and above the modulus), pad bits set;
  D4  records longer than the polynomial needs: the stride bytes_per_poly, which also chooses the kernel form;
  D5  every field width 1..62 through the byte, the 8-byte word and the 128-coefficient tile kernels, both directions.
Every serialize / deserialize case asserts the kernel form it ran through form(), the restatement of csrc/serialize_form.hpp.

Out of scope: a carry in a LATER chunk's counter.  For c >= 1 the counter V_c is an AES output, so such a seed cannot be
constructed, and finding one by search costs about 2 * 10^7 chain steps.  The same counter_add and the same lane shuffles run
in chunk 0, where the table below places every carry."""
import ctypes

import numpy as np
import pytest

import simple_pir_reference as R
import wire_format_reference as W

pytestmark = pytest.mark.gpu


def _bits(modulus):
    return (modulus - 1).bit_length()  # ceilLog2 (ModularArithmetic/Scalar.swift:266-269)


def _moduli(oracle, bits, ntt_degree=1):
    """one modulus per entry of `bits` with that ceilLog2: primes, and 2 for the single width no odd prime has"""
    primes = iter(oracle.generate_primes([b for b in bits if b > 1], False, ntt_degree))
    moduli = [2 if b == 1 else next(primes) for b in bits]
    assert [_bits(q) for q in moduli] == list(bits) and len(set(moduli)) == len(moduli)
    return moduli


def _contexts(oracle, degree, bits):
    import heamd

    moduli = _moduli(oracle, bits)
    return heamd.PolyContext(degree, moduli), oracle.PolyContext(degree, moduli)


def _bytes_to_device(data):
    import torch

    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def _deserialize(ours, data, bytes_per_poly, batch, skip):
    """he_poly_deserialize_device on a uint8 device tensor -> (host slab [batch][L][N], the kernel form the call took)"""
    import heamd
    import torch

    out = torch.full((batch, len(ours.moduli), ours.degree), -1, dtype=torch.int64, device="cuda")
    status = heamd.load_library().he_poly_deserialize_device(ours.h, ctypes.c_void_p(data.data_ptr()), bytes_per_poly, batch, skip,
                                                             ctypes.c_void_p(out.data_ptr()), None)
    assert status == 0, heamd.load_library().he_last_error_message()
    torch.cuda.synchronize()
    widths = [_bits(q) - skip for q in ours.moduli]
    return heamd.to_host(out), W.form("deserialize", ours.degree, widths, data.data_ptr(), out.data_ptr(), bytes_per_poly)


def _serialize(ours, slab, skip):
    """he_poly_serialize_device -> (host bytes [batch][record], the kernel form the call took)"""
    import heamd
    import torch

    device_slab = heamd.to_device(slab)
    batch, record = slab.shape[0], ours.serialization_byte_count(skip)
    out = torch.full((batch, record), 0xA5, dtype=torch.uint8, device="cuda")
    status = heamd.load_library().he_poly_serialize_device(ours.h, ctypes.c_void_p(device_slab.data_ptr()), batch, skip,
                                                           ctypes.c_void_p(out.data_ptr()), None)
    assert status == 0, heamd.load_library().he_last_error_message()
    torch.cuda.synchronize()
    widths = [_bits(q) - skip for q in ours.moduli]
    return out.cpu().numpy(), W.form("serialize", ours.degree, widths, out.data_ptr(), device_slab.data_ptr())


def _unpack_batch(records, degree, widths, skip):
    return np.array([W.unpack_record(bytes(record), degree, widths, skip) for record in records], dtype=np.uint64)


# ---- D1: counter carries -------------------------------------------------------------------------------------------------------
CONTROL_SEEDS = (W.seed_for_counter(0), W.seed_for_counter(1 << 64, bytes(range(16))), bytes(range(32)))


def _carry_seeds():
    return [seed for *_, seed in W.carry_cases()] + list(CONTROL_SEEDS)


def test_carry_seeds_cover_what_they_claim():
    """Every counter addition of a seeded polynomial's first chunk, at every word boundary of the 128-bit counter -- judged by
    the Python DRBG's V_0, not by the table that made the seeds."""
    seeds = _carry_seeds()
    assert len(seeds) % 8 != 0  # the chain kernel's last wavefront has idle 8-lane groups
    counters = [W.CtrDrbg(seed).v for seed in seeds]
    for bits in (32, 64, 96, 128):
        after = [(v + 256) & W.MASK128 for v in counters]
        in_stream = [not W.carries(v, 1, bits) and W.carries(v, 256, bits) for v in counters]
        at_256 = [(v + 256) % (1 << bits) == 0 for v in counters]
        no_chunk_carry = [not W.carries(v, 256, bits) for v in counters]
        both = [quiet and W.carries(a, 1, bits) for quiet, a in zip(no_chunk_carry, after)]
        second_only = [quiet and W.carries(a, 2, bits) and not W.carries(a, 1, bits) for quiet, a in zip(no_chunk_carry, after)]
        nowhere = [not W.carries(v, 258, bits) for v in counters]
        for name, hits in (("stream", in_stream), ("V + 256", at_256), ("re-key + 1 and + 2", both), ("re-key + 2 only", second_only),
                           ("nowhere", nowhere)):
            assert any(hits), (bits, name)
        # the first stream block itself (V + 1) wraps, and a lane in the middle of the wavefront does
        assert any(W.carries(v, 1, bits) for v in counters) and any((v + 129) % (1 << bits) == 0 for v in counters)
    assert any(v + 256 > W.MASK128 for v in counters)  # the whole counter wraps to zero


# degree, modulus bits: two whole chunks (the re-key after a carrying chunk shows in the second); 192 words, a partial chunk
# (blocks past `words` are not stored); one modulus
CARRY_CONTEXTS = [(256, [40, 62]), (64, [30, 31, 33]), (512, [55])]


@pytest.mark.parametrize("degree,bits", CARRY_CONTEXTS, ids=lambda v: str(v).replace(" ", ""))
def test_seeded_polynomials_at_counter_carries(oracle, degree, bits):
    import heamd
    import torch

    moduli = oracle.generate_primes(bits, False, degree)
    ours, ref = heamd.PolyContext(degree, moduli), oracle.PolyContext(degree, moduli)
    seeds = np.frombuffer(b"".join(_carry_seeds()), dtype=np.uint8).reshape(-1, 32)
    got = heamd.to_host(ours.random_from_seeds(torch.from_numpy(seeds.copy()).cuda()))
    expected = ref.random_from_seeds(seeds)
    for index, (one, other) in enumerate(zip(got, expected)):
        assert np.array_equal(one, other), ("seed", index, W.carry_cases()[index][:2] if index < len(W.carry_cases()) else "control")
    # one carrying seed per boundary (the carry falls at lane 32 of the stream), restated without the oracle: the first
    # chunk's 256 counter blocks as little-endian 128-bit integers mod q
    words = min(256, len(moduli) * degree)
    for index, (level, k, _, seed) in enumerate(W.carry_cases()):
        if k != 129:
            continue
        stream = W.CtrDrbg(seed).generate(4096)
        restated = [int.from_bytes(stream[16 * i:16 * i + 16], "little") % moduli[i // degree] for i in range(words)]
        assert got[index].ravel()[:words].tolist() == restated, level


# ---- D2: SimplePIR's one stream over several polynomials ---------------------------------------------------------------------------
def _simple_pir_shapes(oracle):
    """the shapes of tests/test_gpu_simple_pir.py whose A (a_poly_count * N coefficients from one stream) is the smallest that
    spans at least two 256-coefficient chunks"""
    from test_gpu_simple_pir import SHAPES

    sizes = {}
    for name, (entry_count, entry_size, pbits, cbits, n, word_bits) in SHAPES.items():
        params = R.shape(oracle, pbits, cbits, n, entry_count, entry_size, word_bits)
        if params["a_poly_count"] * n > 256:
            sizes[name] = params["a_poly_count"] * n
    return sorted(name for name, size in sizes.items() if size == min(sizes.values()))


@pytest.mark.parametrize("v0", [(1 << 128) - 200, (1 << 64) - 257], ids=["wraps-in-stream", "wraps-in-rekey"])
def test_simple_pir_process_at_counter_carries(oracle, v0):
    import heamd
    import torch

    from test_gpu_simple_pir import SHAPES

    names = _simple_pir_shapes(oracle)
    assert names == ["three-polys-u32", "three-polys-u64"]
    seed = W.seed_for_counter(v0, bytes(range(100, 116)))
    assert oracle.CtrDrbg(seed).state()[1] == v0.to_bytes(16, "big")
    for name in names:
        entry_count, entry_size, pbits, cbits, n, word_bits = SHAPES[name]
        params = R.shape(oracle, pbits, cbits, n, entry_count, entry_size, word_bits)
        assert params["a_poly_count"] * n >= 512
        entries = np.random.default_rng(n + word_bits).integers(0, 256, size=(entry_count, entry_size), dtype=np.uint8)
        database = R.process_database(oracle, entries, params)
        hint = R.hint(params, database, R.materialize_a(params, R.a_polynomials(oracle, params, seed)))
        server_class = heamd.SimplePirServer if word_bits == 64 else heamd.SimplePirServer32
        to_host = heamd.to_host if word_bits == 64 else heamd.to_host32
        server = server_class.process(torch.from_numpy(entries).cuda(), pbits, cbits, n, seed)
        torch.cuda.synchronize()
        assert np.array_equal(to_host(server.wide_database()), database), name
        assert np.array_equal(to_host(server.hint), hint), name


# ---- D3: arbitrary bytes -----------------------------------------------------------------------------------------------------------
MIXED_BITS = [9, 17, 40, 62]
# degree -> the form aligned buffers give: degree 4 is the only one whose rows end in pad bits (N width is a multiple of 8 from
# N = 8 on); 8: rows that start in the middle of a word; 128, 512, 1024: one tile, four tiles (one per wave), two trips per wave
ARBITRARY = {4: "byte", 8: "byte", 64: "word", 128: "tile", 512: "tile", 1024: "tile"}


def test_arbitrary_cases_cover_what_they_claim():
    assert set(ARBITRARY.values()) == {"byte", "word", "tile"}
    for skip in (0, 1, 5):
        pads = [8 * W.row_byte_count(4, b - skip) - 4 * (b - skip) for b in MIXED_BITS]
        assert any(pads)
        for degree in ARBITRARY:
            if degree >= 8:
                assert all(degree * (b - skip) % 8 == 0 for b in MIXED_BITS)  # no pad bits to set
    assert any(o % 8 for o in W.row_offsets(8, MIXED_BITS))


@pytest.mark.parametrize("degree", sorted(ARBITRARY))
def test_deserialize_arbitrary_bytes(oracle, degree):
    ours, ref = _contexts(oracle, degree, MIXED_BITS)
    rng = np.random.default_rng(300 + degree)
    for skip in (0, 1, 5):
        widths = [b - skip for b in MIXED_BITS]
        record = ours.serialization_byte_count(skip)
        assert record == ref.serialization_byte_count(skip) == W.row_offsets(degree, widths)[-1]
        # fields below the modulus, every pad bit set
        rows = [[int(v) for v in rng.integers(0, q, size=degree, dtype=np.uint64)] for q in ours.moduli]
        dirty = bytearray()
        for row, width in zip(rows, widths):
            packed = bytearray(W.pack(row, width, skip))
            packed[-1] |= (1 << (8 * len(packed) - degree * width)) - 1
            dirty += packed
        records = [b"\xff" * record, bytes(rng.integers(0, 256, size=record, dtype=np.uint8)), bytes(dirty)]
        got, form = _deserialize(ours, _bytes_to_device(b"".join(records)), record, len(records), skip)
        assert form == ARBITRARY[degree], (degree, skip)
        assert np.array_equal(got, _unpack_batch(records, degree, widths, skip)), (degree, skip)
        assert np.array_equal(got, ref.deserialize(np.frombuffer(b"".join(records), dtype=np.uint8).reshape(3, record), skip))
        assert got[0].tolist() == [[((1 << w) - 1) << skip] * degree for w in widths]
        assert got[2].tolist() == [[(v >> skip) << skip for v in row] for row in rows]


# ---- D4: the record stride ---------------------------------------------------------------------------------------------------------
# context -> (degree, modulus bits, {extra bytes per record: the form the call takes}); tight records take the form of the name
STRIDES = {
    "tile": (128, [9, 17, 40, 62], {1: "byte", 8: "word", 16: "tile", 24: "word"}),
    "word": (64, [9, 17, 41], {1: "byte", 8: "word", 16: "word", 24: "word"}),  # a record of 8 * 67 bytes: never 16-aligned
    "byte": (8, [9, 17, 40, 62], {1: "byte", 8: "byte", 16: "byte", 24: "byte"}),
}
STRIDE_CASES = [(name, extra, form) for name, (_, _, forms) in STRIDES.items() for extra, form in forms.items()]


def test_stride_cases_cover_what_they_claim():
    assert {extra for _, extra, _ in STRIDE_CASES} == {1, 8, 16, 24}
    assert {form for _, _, form in STRIDE_CASES} == {"byte", "word", "tile"}
    moved = {(name, form) for name, _, form in STRIDE_CASES if name != form}
    assert moved == {("tile", "word"), ("tile", "byte"), ("word", "byte")}  # a byte-form context stays one at every stride
    for name, (degree, bits, forms) in STRIDES.items():
        record = W.row_offsets(degree, bits)[-1]
        assert W.form("deserialize", degree, bits, 0, 0) == name
        for extra, form in forms.items():
            assert W.form("deserialize", degree, bits, 0, 0, record + extra) == form


@pytest.mark.parametrize("name,extra,form", STRIDE_CASES, ids=[f"{n}-context-plus{e}-{f}-form" for n, e, f in STRIDE_CASES])
def test_deserialize_strided_records(oracle, name, extra, form):
    import torch

    degree, bits, _ = STRIDES[name]
    ours, ref = _contexts(oracle, degree, bits)
    batch = 3
    slab = np.stack([np.random.default_rng(400 + degree).integers(0, q, size=(batch, degree), dtype=np.uint64)
                     for q in ours.moduli], axis=1)
    for skip in (0, 1):
        widths = [b - skip for b in bits]
        record = ours.serialization_byte_count(skip)
        tight = ref.serialize(slab, skip)
        assert [bytes(r) for r in tight] == [W.pack_record(poly.tolist(), widths, skip) for poly in slab]
        spaced = np.full((batch, record + extra), 0xFF, dtype=np.uint8)
        spaced[:, :record] = tight
        got, took = _deserialize(ours, torch.from_numpy(spaced).cuda(), record + extra, batch, skip)
        assert took == form, (name, extra, skip)
        expected = (slab >> np.uint64(skip)) << np.uint64(skip)
        assert np.array_equal(got, expected), (name, extra, skip)
        got_tight, took_tight = _deserialize(ours, torch.from_numpy(tight).cuda(), record, batch, skip)
        assert took_tight == name and np.array_equal(got_tight, got)


def test_stride_shorter_than_the_record_is_refused(oracle):
    import heamd
    import torch

    for name, (degree, bits, _) in STRIDES.items():
        ours, _ = _contexts(oracle, degree, bits)
        record = ours.serialization_byte_count()
        for short in (record - 1, record - 8, record - 16):
            with pytest.raises(heamd.HeError) as err:
                ours.deserialize(torch.zeros((3, short), dtype=torch.uint8, device="cuda"))
            assert err.value.name == "serializedBufferSizeMismatch", (name, short)


# ---- D5: every width through every form --------------------------------------------------------------------------------------------
ALL_BITS = list(range(1, 63))  # tests/test_wire_format_reference.py: the smallest and the largest width a PolyContext admits
# (degree, the form, row order): 62 rows, one per width; descending order gives every width other row offsets
SWEEP = [(8, "byte", ALL_BITS), (8, "byte", ALL_BITS[::-1]), (64, "word", ALL_BITS), (64, "word", ALL_BITS[::-1]),
         (128, "tile", ALL_BITS), (128, "tile", ALL_BITS[::-1]), (1024, "tile", ALL_BITS)]


def test_width_sweep_covers_every_width_on_every_form():
    covered = {}
    for degree, form, bits in SWEEP:
        for direction in ("serialize", "deserialize"):
            assert W.form(direction, degree, bits, 0, 0) == form
            covered.setdefault((direction, form), set()).update(bits)
    assert covered == {(direction, form): set(range(1, 63)) for direction in ("serialize", "deserialize")
                       for form in ("byte", "word", "tile")}
    assert {degree for degree, form, _ in SWEEP if form == "tile"} == {128, 1024}  # one tile; two trips per wave
    # in byte form rows start off word boundaries, in word form off 16-byte boundaries
    assert any(o % 8 for o in W.row_offsets(8, ALL_BITS)) and any(o % 16 for o in W.row_offsets(64, ALL_BITS))


def _sweep_slab(degree, bits):
    """two polynomials: 0, alternating bits, the all-ones field, the other alternation -- in that order and one place on"""
    slab = np.zeros((2, len(bits), degree), dtype=np.uint64)
    for r, width in enumerate(bits):
        ones = (1 << width) - 1
        fields = [0, 0xAAAAAAAAAAAAAAAA & ones, ones, 0x5555555555555555 & ones]
        for b in range(2):
            slab[b, r] = [fields[(k + b) % 4] for k in range(degree)]
    return slab


@pytest.mark.parametrize("degree,form,bits", SWEEP, ids=[f"{d}-{f}-{'up' if b[0] == 1 else 'down'}" for d, f, b in SWEEP])
def test_every_width_through_every_form(oracle, degree, form, bits):
    import torch

    ours, ref = _contexts(oracle, degree, bits)
    slab = _sweep_slab(degree, bits)
    packed, took = _serialize(ours, slab, 0)
    assert took == form
    expected = [W.pack_record(poly.tolist(), bits) for poly in slab]
    assert [bytes(r) for r in packed] == expected
    assert np.array_equal(packed, ref.serialize(slab, 0))
    record = len(expected[0])
    ones = b"\xff" * record
    got, took = _deserialize(ours, torch.from_numpy(np.ascontiguousarray(packed)).cuda(), record, 2, 0)
    assert took == form and np.array_equal(got, slab)
    got, took = _deserialize(ours, _bytes_to_device(ones), record, 1, 0)
    assert took == form
    assert got[0].tolist() == [[(1 << width) - 1] * degree for width in bits]
    assert np.array_equal(got, ref.deserialize(np.frombuffer(ones, dtype=np.uint8)[None], 0))
