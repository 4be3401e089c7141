"""he_pir_process_database_device(_u32): MulPirServer.process (MulPir.swift:431-556) on the device, word for word against the
restatement in pir_database_reference (oracle.bytes_to_coefficients + oracle.BfvContext.plaintext_to_eval), and end to end:
a database built on the device answers queries that decrypt to the entries' bytes."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import heamd
import pir_database_reference as refdb
from bfv_helpers import BfvClient

pytestmark = pytest.mark.gpu


def _context(oracle, degree, q_bits, t_bits=17):
    t = oracle.generate_primes([t_bits], True, degree)[0]
    q = oracle.generate_primes(q_bits, False, degree)
    return heamd.BfvContext(degree, t, q), oracle.BfvContext(degree, t, q)


_entries = refdb.varying_entries  # (tests/test_gpu_pir_client.py imports it under this name)


def _device_database(ours, padded, sizes, dims, entry_size, encoding, word32=False, out=None):
    import torch

    database, present = ours.pir_process_database(torch.from_numpy(padded).cuda(), dims, entry_size, encoding,
                                                  entry_sizes=sizes, out=out)
    torch.cuda.synchronize()
    words = heamd.to_host32(database) if word32 else heamd.to_host(database)
    return words, present.cpu().numpy()


def _assert_matches(oracle, ours, ref, entries, padded, sizes, dims, entry_size, encoding, word32=False):
    want_db, want_present = refdb.process(oracle, ref, entries, dims, entry_size, encoding)
    got_db, got_present = _device_database(ours, padded, sizes, dims, entry_size, encoding, word32)
    assert np.array_equal(got_present, want_present)
    assert np.array_equal(got_db.reshape(want_db.shape), want_db)
    return want_db, want_present


# N = 64 (no tiled transform: lift + generic NTT): 128 bytes per plaintext at a 17-bit t
@pytest.mark.parametrize("dims", [[4, 3], [4], [2, 2, 2], [5, 1]])
@pytest.mark.parametrize("mode", ["pack", "split"])
@pytest.mark.parametrize("encoding", [False, True])
def test_database_matches_the_restatement(oracle, dims, mode, encoding):
    ours, ref = _context(oracle, 64, [40, 40, 40, 41])
    rng = np.random.default_rng(len(dims) * 10 + (mode == "split") * 2 + encoding)
    total = int(np.prod(dims))
    if mode == "pack":
        entry_size, count = 20, max(1, total * 6 - 4)  # six entries per plaintext with a prefix, all six without one
    else:
        entry_size, count = 300, max(1, total - 1)  # three chunks; the last row is nil
    entries, padded, sizes = _entries(rng, count, entry_size)
    _assert_matches(oracle, ours, ref, entries, padded, sizes, dims, entry_size, encoding)


@pytest.mark.parametrize("degree", [4096, 8192, 16384, 32768])
@pytest.mark.parametrize("mode", ["pack", "split"])
def test_database_matches_the_restatement_on_the_tiled_rings(oracle, degree, mode):
    """The degrees whose lift rides the forward transform's load (launch_ntt_lift)."""
    ours, ref = _context(oracle, degree, [50, 50, 50, 51])
    rng = np.random.default_rng(degree + (mode == "split"))
    bpp = degree * 16 // 8
    dims = [4, 3]
    if mode == "pack":
        entry_size, count = bpp // 7 - 2, 40  # seven entries per plaintext: six plaintexts
    else:
        entry_size, count = 2 * bpp + 100, 11  # three chunks
    entries, padded, sizes = _entries(rng, count, entry_size)
    _assert_matches(oracle, ours, ref, entries, padded, sizes, dims, entry_size, True)


@pytest.mark.parametrize("mode", ["pack", "split"])
def test_enqueue_only_form_with_full_entries(oracle, mode):
    """entry_sizes NULL: every entry is entry_size_in_bytes long."""
    ours, ref = _context(oracle, 4096, [50, 50, 51])
    rng = np.random.default_rng(5 + (mode == "split"))
    entry_size, count = (100, 300) if mode == "pack" else (9000, 10)
    entries, padded, _ = _entries(rng, count, entry_size, full=True)
    want_db, want_present = refdb.process(oracle, ref, entries, [4, 3], entry_size, True)
    got_db, got_present = _device_database(ours, padded, None, [4, 3], entry_size, True)
    assert np.array_equal(got_present, want_present)
    assert np.array_equal(got_db.reshape(want_db.shape), want_db)


def test_database_on_a_uint32_parameter_set(oracle):
    """The parameter set of test_pir_on_a_uint32_parameter_set (n_4096_logq_27_28_28, t = 2^16 + 1): packed 4-byte words
    equal the 32-bit oracle's, and the 8-byte database of the same context holds the same values."""
    degree = 4096
    q = [(1 << 27) - 40959, (1 << 28) - 65535, (1 << 28) - 73727]
    t = (1 << 16) + 1
    ours = heamd.BfvContext32(degree, t, q)
    wide = heamd.BfvContext(degree, t, q, word_bits=32)
    ref = oracle.BfvContext(degree, t, q, word_bits=32)
    rng = np.random.default_rng(32)
    for dims, entry_size, count in (([4, 3], 500, 100), ([3, 2], 20000, 6)):
        entries, padded, sizes = _entries(rng, count, entry_size)
        want_db, _ = _assert_matches(oracle, ours, ref, entries, padded, sizes, dims, entry_size, True, word32=True)
        got_wide, _ = _device_database(wide, padded, sizes, dims, entry_size, True)
        assert np.array_equal(got_wide.reshape(want_db.shape), want_db)


@pytest.mark.parametrize("group", ["1", "5", "7"])
def test_small_groups_give_the_words_of_one(oracle, monkeypatch, group):
    """HEAMD_PIR_PROCESS_GROUP forces many groups of slots (ragged last group, groups across chunk boundaries)."""
    ours, _ = _context(oracle, 4096, [50, 50, 51])
    rng = np.random.default_rng(int(group))
    for entry_size, count in ((300, 200), (9000, 11)):
        _, padded, sizes = _entries(rng, count, entry_size)
        whole = _device_database(ours, padded, sizes, [4, 3], entry_size, True)
        monkeypatch.setenv("HEAMD_PIR_PROCESS_GROUP", group)
        grouped = _device_database(ours, padded, sizes, [4, 3], entry_size, True)
        monkeypatch.delenv("HEAMD_PIR_PROCESS_GROUP")
        assert np.array_equal(whole[0], grouped[0]) and np.array_equal(whole[1], grouped[1])


def test_errors_leave_the_outputs_untouched(oracle):
    import torch

    ours, _ = _context(oracle, 64, [40, 40, 41])
    rng = np.random.default_rng(3)
    entries, padded, sizes = _entries(rng, 10, 20)
    shape = ours.pir_database_shape([4], 10, 20, True)
    database = torch.full((shape["chunk_count"], 4, ours.L, 64), 0x5A5A, dtype=torch.int64, device="cuda")
    present = torch.full((shape["chunk_count"], 4), 7, dtype=torch.uint8, device="cuda")
    too_long = sizes.copy()
    too_long[4] = 21
    with pytest.raises(heamd.HeError) as err:  # invalidDatabaseEntrySize, from the C entry point
        ours.pir_process_database(torch.from_numpy(padded).cuda(), [4], 20, True, entry_sizes=too_long,
                                  out=(database, present))
    assert err.value.code == 16 and "entry with size 21" in str(err.value)
    with pytest.raises(heamd.HeError):  # invalidDatabaseEntryCount, from the binding
        ours.pir_process_database(entries, [4], 20, True, entry_count=11, out=(database, present))
    lib = heamd.load_library()
    import ctypes

    dims = (ctypes.c_uint32 * 2)(2, 2)
    device_entries = torch.from_numpy(padded).cuda()
    status = lib.he_pir_process_database_device(ours.h, dims, 2, ctypes.c_void_p(device_entries.data_ptr()), None, 10, 300,
                                                1, ctypes.c_void_p(database.data_ptr()), ctypes.c_void_p(present.data_ptr()),
                                                None)  # split mode, 10 entries for 4 rows
    assert status == 16
    torch.cuda.synchronize()
    assert bool((database == 0x5A5A).all()) and bool((present == 7).all())


def _selection(slot, dims):
    out = []
    for d in dims:
        out.append(slot % d)
        slot //= d
    return out


@pytest.mark.parametrize("mode", ["pack", "split"])
def test_device_database_answers_queries(oracle, mode):
    """Processed on the device, answered with pir_compute_response (three chunks in split mode), decrypted by the client and
    turned back into bytes: the queried entries' bytes and size prefixes, nil plaintexts included.  The packed database
    (pack_plaintexts) gives the same responses."""
    import torch

    ours, ref = _context(oracle, 256, [40, 40, 40, 41])  # N = 256: the smallest ring with a packed layout
    client = BfvClient(oracle, ref, seed=90)
    rng = np.random.default_rng(91 + (mode == "split"))
    dims = [4, 3]
    # 512 bytes per plaintext -- pack: 24 entries per plaintext, plaintexts 3..11 nil; split: three chunks, rows 10, 11 nil
    entry_size, count = (20, 50) if mode == "pack" else (1100, 10)
    entries, padded, sizes = _entries(rng, count, entry_size)
    database, present = ours.pir_process_database(torch.from_numpy(padded).cuda(), dims, entry_size, True,
                                                  entry_sizes=sizes)
    shape = ours.pir_database_shape(dims, count, entry_size, True)
    chunks, width, bpp = shape["chunk_count"], shape["entry_size_encoding_width"], shape["bytes_per_plaintext"]
    bits = ref.t.bit_length() - 1
    packed = ours.pack_plaintexts(database)
    qctx = ref.ciphertext_context()
    key = heamd.to_device(client.relinearization_key())
    one, zero = [1] + [0] * (ref.degree - 1), [0] * ref.degree
    plaintexts = -(-count // shape["entries_per_plaintext"]) if mode == "pack" else count
    for j in sorted({0, 1, plaintexts - 1, plaintexts, 11}):
        selection = _selection(refdb.slot_of(j, dims), dims)
        dim0 = np.stack([qctx.forward_ntt(client.encrypt(one if k == selection[0] else zero)) for k in range(dims[0])])
        rest = np.stack([client.encrypt(one if k == selection[1] else zero) for k in range(dims[1])])
        response = ours.pir_compute_response(dims, heamd.to_device(dim0), heamd.to_device(rest), database, chunks,
                                             present_device=present, relinearization_key=key)
        from_packed = ours.pir_compute_response_packed(dims, heamd.to_device(dim0), heamd.to_device(rest), packed, chunks,
                                                       present_device=present, relinearization_key=key)
        assert bool((response == from_packed).all()), j
        got = heamd.to_host(response)
        data = b"".join(bytes(oracle.coefficients_to_bytes(client.decrypt(got[k], moduli_count=1), bits))[:bpp]
                        for k in range(chunks))
        if mode == "split":
            if j >= count:
                assert not any(data), j
                continue
            assert data[:width] == refdb.prefix(len(entries[j]), width)
            assert data[width:width + len(entries[j])] == entries[j]
            assert not any(data[width + len(entries[j]):])
        else:
            per = shape["entries_per_plaintext"]
            encoded = width + entry_size
            for e in range(j * per, (j + 1) * per):
                record = data[(e - j * per) * encoded:(e - j * per + 1) * encoded]
                if e >= count:
                    assert not any(record), (j, e)
                    continue
                assert record[:width] == refdb.prefix(len(entries[e]), width)
                assert record[width:width + len(entries[e])] == entries[e]
                assert not any(record[width + len(entries[e]):])


def test_database_at_the_benchmark_ring(oracle):
    """N = 8192, L = 4 x 55-bit moduli, a 17-bit t, 2048 plaintexts in pack mode: every slot word for word (on a host with
    fewer than 8 threads: 64 slots spread over the database)."""
    import torch
    from conftest import exhaustive_parity, host_threads

    degree = 8192
    ours, ref = _context(oracle, degree, [55] * 5)
    rng = np.random.default_rng(8192)
    dims, entry_size = [64, 32], 120  # E = 121: 135 entries per 16 KiB plaintext
    count = 135 * 2048 - 50
    entries, padded, sizes = _entries(rng, count, entry_size)
    got_db, got_present = _device_database(ours, padded, sizes, dims, entry_size, True)
    slices = refdb.plaintext_bytes(entries, dims, degree, ref.t, entry_size, True)
    bits = ref.t.bit_length() - 1
    slots = range(2048) if exhaustive_parity() else np.linspace(0, 2047, 64).astype(int)
    del padded
    torch.cuda.empty_cache()

    def check(batch):
        coefficients = np.stack([refdb.unpack(oracle, slices[0][s], bits, degree) for s in batch])
        want = ref.plaintext_to_eval(coefficients)
        for row, s in enumerate(batch):
            assert got_present[0, s] == 1, s
            assert np.array_equal(got_db[0, s], want[row]), s
        return len(batch)

    batches = [list(slots)[i:i + 32] for i in range(0, len(slots), 32)]
    with ThreadPoolExecutor(max_workers=max(1, min(32, host_threads()))) as pool:
        assert sum(pool.map(check, batches)) == len(slots)
