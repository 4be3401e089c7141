"""The ciphertext-level wire format on the device: he_ciphertexts_serialize_device(_u32),
he_ciphertexts_deserialize_device(_u32), he_ciphertexts_deserialize_seeded_device(_u32) and the polynomial-level _u32 entries.
Every byte and word is compared with tests/ciphertext_wire_reference.py over the case table of tests/ciphertext_wire_cases.py;
output buffers are pre-filled with a sentinel and compared WHOLE (guards and stride gaps included); every case asserts the
kernel form it ran from the library's plan at the buffers' real addresses against the restatement."""
import ctypes
import os

import numpy as np
import pytest

import ciphertext_wire_cases as C
import ciphertext_wire_reference as R
import wire_format_reference as W

pytestmark = pytest.mark.gpu

GUARD = 256  # bytes before and after every output: a multiple of the buffers' alignment, so the offsets stay what the case names
SENTINEL = 0xA5


def _dtype(word_bits):
    return np.uint32 if word_bits == 32 else np.uint64


def _aligned_bytes(size, fill):
    import torch

    buffer = torch.full((size,), fill, dtype=torch.uint8, device="cuda")
    assert buffer.data_ptr() % C.BASE_ALIGNMENT == 0
    return buffer


def _slab_to_device(words, word_bits, offset_words):
    """host words -> (the device buffer, a view of it that starts offset_words in): guards of sentinel words around it"""
    import torch

    size = 8 if word_bits == 64 else 4
    guard = GUARD // size
    flat = np.full(guard + offset_words + words.size + guard, 0xA5A5A5A5A5A5A5A5 & ((1 << word_bits) - 1), dtype=_dtype(word_bits))
    flat[guard + offset_words:guard + offset_words + words.size] = words.ravel()
    signed = flat.view(np.int64 if word_bits == 64 else np.int32)
    buffer = torch.from_numpy(signed.copy()).cuda()
    assert buffer.data_ptr() % C.BASE_ALIGNMENT == 0
    return buffer, buffer[guard + offset_words:guard + offset_words + words.size], flat


def _host_words(tensor, word_bits):
    return tensor.cpu().numpy().view(_dtype(word_bits))


def _random_ciphertexts(rng, case, moduli):
    shape = (case.count, case.poly_count, case.degree)
    return np.stack([rng.integers(0, q, size=shape, dtype=np.uint64) for q in moduli], axis=2)


def _contexts(case):
    import heamd

    return heamd.PolyContext(case.degree, C.moduli_of(case.bits, heamd.generate_primes))


def _expected_records(cts, case, moduli, skips):
    return [R.pack_ciphertext(ct.tolist(), case.degree, moduli, skips) for ct in cts]


def _serialize(ctx, case, cts, skips, stride, word_bits=None):
    """-> (the whole output buffer on the host, the offset of record 0 in it, the plan of the call, record 0's address)"""
    word_bits = word_bits or case.word_bits
    record = ctx.ciphertexts_serialization_byte_count(case.poly_count, skips)
    span = (case.count - 1) * stride + record
    out = _aligned_bytes(GUARD + case.record_offset + span + GUARD, SENTINEL)
    _, slab, _ = _slab_to_device(cts.astype(_dtype(word_bits)), word_bits, case.slab_offset)
    records = out[GUARD + case.record_offset:]
    plan = ctx.ciphertexts_wire_plan("serialize", case.poly_count, skips, stride, records.data_ptr(), slab.data_ptr(), word_bits)
    ctx.ciphertexts_serialize(slab.view(case.count, case.poly_count, len(case.bits), case.degree), skips, stride, out=records)
    return out.cpu().numpy(), GUARD + case.record_offset, plan, records.data_ptr()


def _check_serialized(image, start, expected_records, stride):
    want = np.full(image.size, SENTINEL, dtype=np.uint8)
    for i, record in enumerate(expected_records):
        want[start + i * stride:start + i * stride + len(record)] = np.frombuffer(record, dtype=np.uint8)
    mismatches = np.nonzero(image != want)[0]
    assert mismatches.size == 0, ("first differing byte", int(mismatches[0]) - start, "of", mismatches.size)


@pytest.mark.parametrize("case", C.ALL, ids=C.case_id)
def test_serialize(case):
    ctx = _contexts(case)
    moduli = [int(q) for q in ctx.moduli]
    skips = C.skips_of(case)
    plain = skips or [0] * case.poly_count
    rng = np.random.default_rng(C.ALL.index(case))
    cts = _random_ciphertexts(rng, case, moduli)
    cts[0, -1] = np.array(moduli, dtype=np.uint64)[:, None] - 1  # every field of one polynomial q_r - 1
    record = R.record_bytes(case.degree, moduli, plain)
    stride = C.stride_of(case, record)
    expected = _expected_records(cts, case, moduli, plain)
    image, start, plan, address = _serialize(ctx, case, cts, skips, stride)
    assert address % C.BASE_ALIGNMENT == case.record_offset
    assert plan == R.ciphertext_form("serialize", case.degree, len(moduli), case.poly_count, record, stride, address)
    assert plan["form"] == "chunk" and plan["edge_free"] == (case.record_offset % 8 == 0 and stride % 8 == 0)
    _check_serialized(image, start, expected, stride)
    if case.word_bits == 32:  # the 8-byte entry on the widened words gives the same bytes
        wide, wide_start, _, _ = _serialize(ctx, case, cts, skips, stride, word_bits=64)
        assert wide_start == start and np.array_equal(wide, image)


def _records_buffer(records, case, stride, record_bytes):
    """device bytes of exactly offset + (count - 1) stride + record bytes: records at their stride, the gaps 0xFF"""
    import torch

    span = (case.count - 1) * stride + record_bytes
    host = np.full(case.record_offset + span, 0xFF, dtype=np.uint8)
    for i, record in enumerate(records):
        host[case.record_offset + i * stride:case.record_offset + i * stride + record_bytes] = np.frombuffer(record, dtype=np.uint8)
    buffer = torch.from_numpy(host).cuda()
    assert buffer.data_ptr() % C.BASE_ALIGNMENT == 0 and buffer.numel() == case.record_offset + span
    return buffer, buffer[case.record_offset:]


def _deserialize(ctx, case, records, skips, stride, record_bytes, word_bits=None):
    """-> (host words [count][polys][L][N], the flag word, the plan); asserts the guards around the slab"""
    import torch

    word_bits = word_bits or case.word_bits
    keep, view = _records_buffer(records, case, stride, record_bytes)
    words = case.count * case.poly_count * len(case.bits) * case.degree
    buffer, slab, before = _slab_to_device(np.zeros(words, dtype=_dtype(word_bits)) + 7, word_bits, case.slab_offset)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    plan = ctx.ciphertexts_wire_plan("deserialize", case.poly_count, skips, stride, view.data_ptr(), slab.data_ptr(), word_bits)
    ctx.ciphertexts_deserialize(view, case.count, case.poly_count, skips, stride, word_bits, out=slab, mismatch=flag)
    after = _host_words(buffer, word_bits)
    lead = GUARD // (word_bits // 8) + case.slab_offset
    assert np.array_equal(after[:lead], before[:lead]) and np.array_equal(after[lead + words:], before[lead + words:])
    got = after[lead:lead + words].reshape(case.count, case.poly_count, len(case.bits), case.degree)
    return got, int(flag.cpu()[0]), plan


def _wire_records(rng, case, moduli, plain, kind):
    """records into deserialize: "packed" (random fields below q, pad bits zero), "random" (any bytes, pad bits set) or
    "ones" (all 0xFF) behind a correct header"""
    record = R.record_bytes(case.degree, moduli, plain)
    if kind == "packed":
        return _expected_records(_random_ciphertexts(rng, case, moduli), case, moduli, plain)
    header = case.poly_count.to_bytes(2, "little")
    if kind == "ones":
        return [header + b"\xff" * (record - 2)] * case.count
    return [header + rng.integers(0, 256, size=record - 2, dtype=np.uint8).tobytes() for _ in range(case.count)]


@pytest.mark.parametrize("case", C.ALL, ids=C.case_id)
def test_deserialize(case):
    ctx = _contexts(case)
    moduli = [int(q) for q in ctx.moduli]
    skips = C.skips_of(case)
    plain = skips or [0] * case.poly_count
    rng = np.random.default_rng(1000 + C.ALL.index(case))
    record = R.record_bytes(case.degree, moduli, plain)
    stride = C.stride_of(case, record)
    kind = C.RECORD_KINDS[C.ALL.index(case) % 3]
    records = _wire_records(rng, case, moduli, plain, kind)
    got, flag, plan = _deserialize(ctx, case, records, skips, stride, record)
    assert plan["form"] == "field" and plan["edge_free"] == (case.record_offset % 8 == 0 and stride % 8 == 0)
    assert plan["items_per_record"] == case.poly_count * len(moduli) * case.degree and plan["record_bytes"] == record
    assert flag == 0
    for i, bytes_ in enumerate(records):
        count, polys = R.unpack_ciphertext(bytes_, case.poly_count, case.degree, moduli, plain)
        assert count == case.poly_count
        assert np.array_equal(got[i], np.array(polys, dtype=np.uint64).astype(got.dtype)), ("record", i, kind)
    if case.word_bits == 32:  # the 8-byte entry's words, narrowed
        wide, _, _ = _deserialize(ctx, case, records, skips, stride, record, word_bits=64)
        assert np.array_equal(wide.astype(np.uint32), got) and int(wide.max()) < (1 << 32)


@pytest.mark.parametrize("word_bits", [64, 32])
def test_wrong_header_sets_the_flag_and_spoils_nothing(word_bits):
    case = next(c for c in C.cases(word_bits) if c.degree == 64 and c.count == 5 and c.poly_count == 2 and len(c.bits) == 3)
    ctx = _contexts(case)
    moduli = [int(q) for q in ctx.moduli]
    skips = C.skips_of(case)
    plain = skips or [0, 0]
    rng = np.random.default_rng(5)
    record = R.record_bytes(case.degree, moduli, plain)
    stride = C.stride_of(case, record)
    records = _wire_records(rng, case, moduli, plain, "packed")
    for header in (b"\x03\x00", b"\x02\x01"):  # another count; the right low byte under a wrong high byte
        spoiled = list(records)
        spoiled[3] = header + records[3][2:]
        got, flag, _ = _deserialize(ctx, case, spoiled, skips, stride, record)
        assert flag == 1
        for i, bytes_ in enumerate(spoiled):  # every record, the spoiled one included, is decoded as poly_count polynomials
            _, polys = R.unpack_ciphertext(bytes_, 2, case.degree, moduli, plain)
            assert np.array_equal(got[i], np.array(polys, dtype=np.uint64).astype(got.dtype))


# ---- seeded ciphertexts --------------------------------------------------------------------------------------------------------
# words per polynomial below one 256-coefficient chunk, exactly one, one and a half
SEEDED_SHAPES = [(8, 3), (128, 2), (128, 3)]
SEEDED_BITS = {64: [40, 62, 55], 32: [30, 27, 28]}


def _seeds(count):
    carry = next(seed for bits, k, _, seed in W.carry_cases() if bits == 64 and k == 129)  # the stream carries at lane 32
    return [carry] + [bytes((17 * i + j) & 0xFF for j in range(32)) for i in range(1, count)]


@pytest.mark.parametrize("word_bits", [64, 32])
@pytest.mark.parametrize("degree,rows", SEEDED_SHAPES)
def test_deserialize_seeded(oracle, degree, rows, word_bits):
    import heamd
    import torch

    count = 5
    moduli = [int(q) for q in oracle.generate_primes(SEEDED_BITS[word_bits][:rows], False, degree)]
    ctx, ref = heamd.PolyContext(degree, moduli), oracle.PolyContext(degree, moduli)
    rng = np.random.default_rng(degree + rows)
    widths = R.widths(moduli, 0)
    record = W.row_offsets(degree, widths)[-1]
    assert record == ctx.serialization_byte_count(0)
    stride = record + 3  # odd: no record but the first keeps the buffer's alignment
    poly0 = np.stack([rng.integers(0, q, size=(count, degree), dtype=np.uint64) for q in moduli], axis=1)
    host = np.full((count - 1) * stride + record, 0xFF, dtype=np.uint8)
    for i in range(count):
        host[i * stride:i * stride + record] = np.frombuffer(W.pack_record(poly0[i].tolist(), widths), dtype=np.uint8)
    records = torch.from_numpy(host).cuda()
    seeds = _seeds(count)
    device_seeds = torch.from_numpy(np.frombuffer(b"".join(seeds), dtype=np.uint8).copy()).cuda()
    eval_a = np.array([R.seeded_polynomial(seed, degree, moduli) for seed in seeds], dtype=np.uint64)
    assert np.array_equal(eval_a, ref.random_from_seeds(np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(-1, 32)))
    words = count * 2 * rows * degree
    dtype = _dtype(word_bits)
    sentinel = dtype(0xA5A5A5A5A5A5A5A5 & ((1 << word_bits) - 1))
    for coeff_format in (0, 1):
        a = ref.inverse_ntt(eval_a.copy()) if coeff_format else eval_a
        for use_poly0, use_seeds in ((True, True), (True, False), (False, True)):
            buffer, slab, before = _slab_to_device(np.zeros(words, dtype=dtype) + sentinel, word_bits, 1)
            ctx.ciphertexts_deserialize_seeded(records if use_poly0 else None, device_seeds if use_seeds else None, count,
                                               coeff_format, stride, word_bits, out=slab)
            after = _host_words(buffer, word_bits)
            lead = GUARD // (word_bits // 8) + 1
            assert np.array_equal(after[:lead], before[:lead]) and np.array_equal(after[lead + words:], before[lead + words:])
            got = after[lead:lead + words].reshape(count, 2, rows, degree)
            want0 = poly0.astype(dtype) if use_poly0 else np.full_like(got[:, 0], sentinel)
            want1 = a.astype(dtype) if use_seeds else np.full_like(got[:, 1], sentinel)
            assert np.array_equal(got[:, 0], want0), (coeff_format, use_poly0, use_seeds, "slot 0")
            assert np.array_equal(got[:, 1], want1), (coeff_format, use_poly0, use_seeds, "slot 1")
    # the polynomial-level sampler on 4-byte slabs is the 8-byte one narrowed
    if word_bits == 32:
        narrow = _host_words(ctx.random_from_seeds_u32(device_seeds), 32)
        assert np.array_equal(narrow, eval_a.astype(np.uint32))
        assert np.array_equal(heamd.to_host(ctx.random_from_seeds(device_seeds)), eval_a)


# ---- the polynomial-level entries on 4-byte slabs --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.NARROW, ids=lambda c: f"n{c.degree}-l{len(c.bits)}-skip{c.skip}-at{c.bytes_offset}-plus{c.extra}")
def test_poly_wire_entries_on_4_byte_slabs(case):
    import heamd
    import torch

    lib = heamd.load_library()
    batch = 3
    ctx = heamd.PolyContext(case.degree, C.moduli_of(case.bits, heamd.generate_primes))
    moduli = [int(q) for q in ctx.moduli]
    widths = R.widths(moduli, case.skip)
    record = W.row_offsets(case.degree, widths)[-1]
    rng = np.random.default_rng(case.degree + case.extra)
    slab = np.stack([rng.integers(0, q, size=(batch, case.degree), dtype=np.uint64) for q in moduli], axis=1)
    slab[1] = np.array(moduli, dtype=np.uint64)[:, None] - 1
    packed = [W.pack_record(poly.tolist(), widths, case.skip) for poly in slab]
    # serialize: tight records from the buffer's offset on, guards around them
    out = _aligned_bytes(GUARD + case.bytes_offset + batch * record + GUARD, SENTINEL)
    view = out[GUARD + case.bytes_offset:]
    device_slab = torch.from_numpy(slab.astype(np.uint32).view(np.int32)).cuda()
    plan = ctx.ciphertexts_wire_plan("serialize", 0, [case.skip], 0, view.data_ptr(), device_slab.data_ptr(), 32)
    assert plan["form"] == case.serialize_form and plan["record_bytes"] == record
    assert lib.he_poly_serialize_device_u32(ctx.h, ctypes.c_void_p(device_slab.data_ptr()), batch, case.skip,
                                            ctypes.c_void_p(view.data_ptr()), None) == 0
    _check_serialized(out.cpu().numpy(), GUARD + case.bytes_offset, [b"".join(packed)], 0)
    wide = ctx.serialize(heamd.to_device(slab), case.skip).cpu().numpy()
    assert [bytes(r) for r in wide] == packed
    # deserialize: records `extra` bytes longer than the polynomial, pad bits and gaps set
    stride = record + case.extra
    host = np.full(case.bytes_offset + batch * stride, 0xFF, dtype=np.uint8)
    raw = [rng.integers(0, 256, size=record, dtype=np.uint8).tobytes() for _ in range(batch)]
    for i, bytes_ in enumerate(raw):
        host[case.bytes_offset + i * stride:case.bytes_offset + i * stride + record] = np.frombuffer(bytes_, dtype=np.uint8)
    device_bytes = torch.from_numpy(host).cuda()
    records = device_bytes[case.bytes_offset:]
    words = batch * len(moduli) * case.degree
    buffer, target, before = _slab_to_device(np.zeros(words, dtype=np.uint32), 32, 0)
    plan = ctx.ciphertexts_wire_plan("deserialize", 0, [case.skip], stride, records.data_ptr(), target.data_ptr(), 32)
    assert plan["form"] == case.deserialize_form
    assert lib.he_poly_deserialize_device_u32(ctx.h, ctypes.c_void_p(records.data_ptr()), stride, batch, case.skip,
                                              ctypes.c_void_p(target.data_ptr()), None) == 0
    after = _host_words(buffer, 32)
    lead = GUARD // 4
    assert np.array_equal(after[:lead], before[:lead]) and np.array_equal(after[lead + words:], before[lead + words:])
    expected = np.array([W.unpack_record(r, case.degree, widths, case.skip) for r in raw], dtype=np.uint64)
    assert np.array_equal(after[lead:lead + words].reshape(expected.shape), expected.astype(np.uint32))
    strided = records[:batch * stride].view(batch, stride) if case.bytes_offset == 0 else None
    if strided is not None:
        assert np.array_equal(heamd.to_host(ctx.deserialize(strided, case.skip)), expected)


# ---- capped grids ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def grid_cap():
    saved = os.environ.get("HEAMD_GRID_CAP")

    def set_cap(value):
        os.environ["HEAMD_GRID_CAP"] = str(value)

    yield set_cap
    if saved is None:
        os.environ.pop("HEAMD_GRID_CAP", None)
    else:
        os.environ["HEAMD_GRID_CAP"] = saved


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("word_bits", [64, 32])
def test_strided_loops_under_a_capped_grid(oracle, grid_cap, cap, word_bits):
    """a lane that makes several trips through its loop gives the words of one that makes a single trip: the sampler at
    ciphertext stride (16 ciphertexts of two chunks are 32 chunks, 8 workgroups of kStreamWaves = 4 uncapped: 8 trips at cap 1,
    3 at cap 3) and (4-byte slabs) the byte and word kernels the polynomial-level entries now share.  The two ciphertext
    kernels have no loop (one item per lane on an exact grid); they run here too, and the cap must not touch them."""
    import heamd
    import torch

    case = next(c for c in C.cases(word_bits) if c.degree == 1024 and c.count == 5 and c.poly_count == 2 and len(c.bits) == 3)
    ctx = _contexts(case)
    moduli = [int(q) for q in ctx.moduli]
    skips = C.skips_of(case)
    plain = skips or [0, 0]
    rng = np.random.default_rng(cap)
    record = R.record_bytes(case.degree, moduli, plain)
    stride = C.stride_of(case, record)
    cts = _random_ciphertexts(rng, case, moduli)
    expected = _expected_records(cts, case, moduli, plain)
    grid_cap(cap)
    image, start, _, _ = _serialize(ctx, case, cts, skips, stride)
    _check_serialized(image, start, expected, stride)
    got, flag, _ = _deserialize(ctx, case, expected, skips, stride, record)
    kept = np.stack([(cts[:, p] >> np.uint64(plain[p])) << np.uint64(plain[p]) for p in range(case.poly_count)], axis=1)
    assert flag == 0 and np.array_equal(got, kept.astype(got.dtype))  # the skipped bits come back as zeros
    # seeded: 16 ciphertexts of 384 words (a chunk and a half per polynomial), poly0 records at an odd stride.  The oracle's
    # sampler stands in for the Python one here (16 seeds in Python integers take too long; test_deserialize_seeded holds the
    # oracle's to it), the first seed is also restated in Python.
    degree, rows, count = 128, 3, 16
    ntt_moduli = [int(q) for q in oracle.generate_primes(SEEDED_BITS[word_bits][:rows], False, degree)]
    seeded, ref = heamd.PolyContext(degree, ntt_moduli), oracle.PolyContext(degree, ntt_moduli)
    seeds = _seeds(count)
    host_seeds = np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(-1, 32)
    device_seeds = torch.from_numpy(host_seeds.copy()).cuda()
    eval_a = ref.random_from_seeds(host_seeds)
    assert np.array_equal(eval_a[0], np.array(R.seeded_polynomial(seeds[0], degree, ntt_moduli), dtype=np.uint64))
    widths = R.widths(ntt_moduli, 0)
    poly_bytes = W.row_offsets(degree, widths)[-1]
    poly_stride = poly_bytes + 3
    poly0 = np.stack([rng.integers(0, q, size=(count, degree), dtype=np.uint64) for q in ntt_moduli], axis=1)
    host = np.full((count - 1) * poly_stride + poly_bytes, 0xFF, dtype=np.uint8)
    for i in range(count):
        host[i * poly_stride:i * poly_stride + poly_bytes] = np.frombuffer(W.pack_record(poly0[i].tolist(), widths), dtype=np.uint8)
    device_poly0 = torch.from_numpy(host).cuda()
    dtype = _dtype(word_bits)
    for coeff_format in (0, 1):
        a = ref.inverse_ntt(eval_a.copy()) if coeff_format else eval_a
        out = _host_words(seeded.ciphertexts_deserialize_seeded(device_poly0, device_seeds, count, coeff_format, poly_stride,
                                                                word_bits), word_bits)
        assert np.array_equal(out[:, 0], poly0.astype(dtype)) and np.array_equal(out[:, 1], a.astype(dtype)), coeff_format
    # ... and with the deserializer skipped, slot 0 keeps what it held
    held = torch.full((count, 2, rows, degree), 7, dtype=torch.int32 if word_bits == 32 else torch.int64, device="cuda")
    out = _host_words(seeded.ciphertexts_deserialize_seeded(None, device_seeds, count, 0, None, word_bits, out=held), word_bits)
    assert np.array_equal(out[:, 1], eval_a.astype(dtype)) and bool((out[:, 0] == 7).all())
    if word_bits == 32:
        for narrow in (c for c in C.NARROW if c.degree == 1024):
            test_poly_wire_entries_on_4_byte_slabs(narrow)
