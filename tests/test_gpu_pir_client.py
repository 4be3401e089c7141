"""The MulPIR client on the device against tests/pir_client_reference.py: word for word on the query
ciphertexts, byte for byte on the entries -- no comparison here has a tolerance.

  query words   he_pir_generate_query_device against the Python-integer client (encrypt_reference.py on the same seeds) at N = 64,
                and against he_bfv_encrypt_device on the reference's plaintexts at N = 4096; an index outside the database
  reply bytes   he_pir_decrypt_response_device on replies made by encrypting chosen plaintexts at one modulus (and at two):
                pack and split mode, with and without a size prefix, bits = 16, 17 and 9, coefficients in [2^bits, t), prefixes
                above E and of 0, decryptFull
  end to end    process_database -> evaluation keys from he_pir_evaluation_key_elements -> generate_query ->
                compute_response_to_query -> decrypt_response, nothing on the host in between
  footprint     both entries on tests/footprint.py arenas under both poisons, with and without a caller's workspace

Shapes are the smallest at which each branch exists; the comment next to a shape names the branch."""
import collections
import ctypes

import numpy as np
import pytest

import encrypt_reference
import footprint
import heamd
import pir_client_reference as client
import pir_database_reference as refdb
from test_gpu_pir_database import _entries

pytestmark = pytest.mark.gpu

T17, T9 = 65537, 641  # bits = 16: every field begins a byte; t = 641: 9 bits at N = 64, fields begin anywhere
OK, INVALID = 0, 16
vp = ctypes.c_void_p

_rings = {}


class Ring:
    """One parameter set on one slab word: the device context, a secret key made from a seed on the device and the same key as
    the Python-integer reference makes it"""

    def __init__(self, oracle, degree, t, bits, word32):
        import torch

        self.oracle, self.degree, self.t, self.word32 = oracle, degree, t, word32
        self.q = heamd.generate_primes(list(bits), False, degree)
        self.ours = (heamd.BfvContext32 if word32 else heamd.BfvContext)(degree, t, self.q)
        self.L = self.ours.L
        self.stream = encrypt_reference.oracle_stream(oracle)
        seed = np.random.default_rng(degree + t).integers(0, 256, size=(1, 32), dtype=np.uint8)
        self.key = self.ours.generate_secret_key(torch.from_numpy(seed).cuda())[0].contiguous()
        self.s_eval = encrypt_reference.generate_secret_key(oracle.PolyContext(degree, self.q), bytes(seed[0]), self.stream)

    def to_device(self, array):
        array = np.ascontiguousarray(array, dtype=np.uint64)
        return heamd.to_device32(array) if self.word32 else heamd.to_device(array)

    def to_host(self, tensor):
        return heamd.to_host32(tensor) if self.word32 else heamd.to_host(tensor)

    def poly_ctx(self, moduli_count):
        return self.oracle.PolyContext(self.degree, self.q[:moduli_count])


def ring_for(oracle, degree, t, word32, bits=None):
    bits = bits or ((27, 28, 28) if word32 else (40, 40, 41))  # two ciphertext moduli and the key-switching one
    key = (degree, t, word32, tuple(bits))
    if key not in _rings:
        _rings[key] = Ring(oracle, degree, t, bits, word32)
    return _rings[key]


def t18(oracle):
    return oracle.generate_primes([18], True, 64)[0]  # 17 bits per coefficient: not a multiple of 8


def seeds(rng, *shape):
    import torch

    return torch.from_numpy(rng.integers(0, 256, size=shape + (32,), dtype=np.uint8)).cuda()


def device_indices(indices):
    import torch

    return torch.from_numpy(np.array(indices, dtype=np.uint64).view(np.int64)).cuda()


# ---- query words -------------------------------------------------------------------------------------------------------------------
def check_query(oracle, word32, dims, indices, entry_count=None, flagged=False):
    """N = 64 (no tiled transform), E = 20 with a prefix: six entries per plaintext"""
    ring = ring_for(oracle, 64, T17, word32)
    indices = np.array(indices, dtype=np.uint64)
    queries, count = indices.shape
    entry_count = entry_count or int(np.prod(dims)) * 6 - 2
    p = client.plan(64, T17, dims, entry_count, 20, True, count)
    assert p["entries_per_plaintext"] == 6
    C = p["query_ciphertext_count"]
    rng = np.random.default_rng(sum(dims) + count)
    a_seeds, error_seeds = seeds(rng, queries, C), seeds(rng, queries, C)
    out, flag = ring.ours.pir_generate_query(device_indices(indices), dims, entry_count, 20, True, ring.key, a_seeds, error_seeds)
    assert tuple(out.shape) == (queries, C, 2, ring.L, 64)
    a_host, e_host = a_seeds.cpu().numpy(), error_seeds.cpu().numpy()
    expected = np.stack([client.generate_query(ring.poly_ctx(ring.L), T17, p, [int(e) for e in indices[q]], ring.s_eval,
                                               [bytes(s) for s in a_host[q]], [bytes(s) for s in e_host[q]], ring.stream)
                         for q in range(queries)])
    assert np.array_equal(ring.to_host(out), expected), (dims, word32)
    assert int(flag.item()) == int(flagged)
    return p


# the pool of a query shape: 0, the last entry, 7 and 13 (position 1 of their plaintexts: e mod per != 0), the middle
@pytest.mark.parametrize("word32", [False, True])
@pytest.mark.parametrize("dims,count", [([4, 3], 1), ([4, 3], 3), ([5], 1), ([5], 3), ([2, 2, 2], 1), ([2, 2, 2], 3)])
def test_query_words_equal_the_python_integer_client(oracle, dims, count, word32):
    entries = int(np.prod(dims)) * 6 - 2
    pool = [0, entries - 1, 7, entries // 2, 13, 1] if count == 3 else [7, entries - 1]
    p = check_query(oracle, word32, dims, np.array(pool).reshape(2, count))
    assert p["query_ciphertext_count"] == 1


@pytest.mark.parametrize("word32", [False, True])
def test_query_of_two_ciphertexts_with_two_selection_values(oracle, word32):
    """dims [40, 30], two indices: S I = 140 > N, so three ciphertexts; the last compresses 12 inputs (2^-4) where the others
    compress 64 (2^-6), and the second index's inputs straddle ciphertexts"""
    entries = 1200 * 6 - 3
    p = check_query(oracle, word32, [40, 30], [[0, entries - 1], [7, entries // 2]], entry_count=entries)
    assert p["query_ciphertext_count"] == 3 and p["expanded_query_count"] - 2 * 64 == 12
    assert client.selection_value(12, T17) != client.selection_value(64, T17)


@pytest.mark.parametrize("word32", [False, True])
def test_index_outside_the_database_sets_the_flag_and_selects_nothing(oracle, word32):
    """entry_count itself and 2^64 - 1: the flag, zero selection words for that index, the other indices' words as they are
    without it (the reference's nonzero_positions leaves an invalid index out and nothing else)"""
    dims, entries = [4, 3], 70
    bad = [[entries, 7, entries - 1], [0, (1 << 64) - 1, 5]]
    p = check_query(oracle, word32, dims, bad, flagged=True)
    for row in bad:
        plaintext = client.query_plaintexts(p, T17, row)[0]
        good = client.query_plaintexts(p, T17, [e if e < entries else 0 for e in row])[0]
        at = [i for i, e in enumerate(row) if e >= entries][0]
        assert not plaintext[7 * at:7 * at + 7].any() and good[7 * at:7 * at + 7].any()
        keep = np.ones(64, dtype=bool)
        keep[7 * at:7 * at + 7] = False
        assert np.array_equal(plaintext[keep], good[keep])


@pytest.mark.parametrize("word32", [False, True])
def test_query_words_at_4096(oracle, word32):
    """N = 4096 (the tiled transforms), dims [40, 30] and 60 indices: S I = 4200, two ciphertexts, 104 inputs in the last.  The
    words are he_bfv_encrypt_device's on the reference's plaintexts and the same seeds."""
    import torch

    degree, dims, count, queries = 4096, [40, 30], 60, 2
    ring = ring_for(oracle, degree, T17, word32, bits=(27, 28, 28) if word32 else (50, 51, 52))
    per = degree * 16 // 8 // 21
    entries = 1200 * per - 5
    p = client.plan(degree, T17, dims, entries, 20, True, count)
    assert (p["query_ciphertext_count"], p["entries_per_plaintext"]) == (2, per)
    rng = np.random.default_rng(4096)
    indices = rng.integers(0, entries, size=(queries, count), dtype=np.uint64)
    indices[0, :3], indices[1, -2:] = [0, entries - 1, per + 1], [entries - 1, 0]
    a_seeds, error_seeds = seeds(rng, queries, 2), seeds(rng, queries, 2)
    out, flag = ring.ours.pir_generate_query(device_indices(indices), dims, entries, 20, True, ring.key, a_seeds, error_seeds)
    plaintexts = np.stack([client.query_plaintexts(p, T17, [int(e) for e in row]) for row in indices])
    assert np.count_nonzero(plaintexts) == queries * count * 2
    expected = ring.ours.encrypt(ring.to_device(plaintexts.reshape(-1, degree)), ring.key, a_seeds.view(-1, 32),
                                 error_seeds.view(-1, 32))
    assert torch.equal(out.view(expected.shape), expected) and int(flag.item()) == 0
    assert tuple(ring.ours.pir_generate_query(device_indices(indices[:0]), dims, entries, 20, True, ring.key, a_seeds[:0],
                                              error_seeds[:0])[0].shape) == (0, 2, 2, ring.L, degree)  # an empty batch


# ---- reply bytes -------------------------------------------------------------------------------------------------------------------
def reply_plaintexts(oracle, rng, p, t, index, size):
    """[R][N] coefficients of a reply whose byte string is random but for the size prefix of `index`'s record, with two
    coefficients of that record's body (and two of the last plaintext) moved into [2^bits, t): one whose field begins a byte,
    one whose field does not (where bits leaves such a field)"""
    bits, bpp, n = p["bits"], p["bytes_per_plaintext"], p["degree"]
    width, R = p["entry_size_encoding_width"], p["reply_ciphertext_count"]
    data = bytearray(rng.integers(0, 256, R * bpp, dtype=np.uint8).tobytes())
    start = (index % p["entries_per_plaintext"]) * p["encoded"]
    data[start:start + width] = refdb.prefix(size, width)
    coefficients = np.stack([refdb.unpack(oracle, bytes(data[k * bpp:(k + 1) * bpp]), bits, n) for k in range(R)])
    assert int(coefficients.max()) < 1 << bits
    room = t - (1 << bits)
    for plaintext, first_bit in [(0, (start + width) * 8 + bits)] + ([(R - 1, bits)] if R > 1 else []):
        fields = [k for k in range(n) if k * bits >= first_bit]
        aligned = [k for k in fields if k * bits % 8 == 0][:1]
        unaligned = [k for k in fields if k * bits % 8 != 0][:1]
        assert aligned and (unaligned or bits % 8 == 0)
        for k in aligned + unaligned:
            coefficients[plaintext, k] = (1 << bits) + int(coefficients[plaintext, k]) % room
    return coefficients


REPLY_RINGS = {  # name: (t or its name, 4-byte words, moduli_count of the replies)
    "bits16-u64": (T17, False, 1), "bits16-u64-two-moduli": (T17, False, 2), "bits9-u64": (T9, False, 1), "bits17-u64": ("t18", False, 1),
    "bits16-u32": (T17, True, 1), "bits9-u32": (T9, True, 1), "bits17-u32": ("t18", True, 1),
}
REPLY_MODES = {"pack-prefix": (20, True), "pack": (20, False), "split-prefix": (300, True), "split": (300, False)}


@pytest.mark.parametrize("mode", list(REPLY_MODES))
@pytest.mark.parametrize("name", list(REPLY_RINGS))
def test_reply_bytes_equal_the_reference(oracle, name, mode):
    import torch

    t, word32, moduli_count = REPLY_RINGS[name]
    t = t18(oracle) if t == "t18" else t
    ring = ring_for(oracle, 64, t, word32)
    entry_size, encoding = REPLY_MODES[mode]
    dims = [4, 3]
    probe = client.plan(64, t, dims, 0, entry_size, encoding, 3)
    per, R, width = probe["entries_per_plaintext"], probe["reply_ciphertext_count"], probe["entry_size_encoding_width"]
    assert (R > 1) == mode.startswith("split") and width == (0 if not encoding else 1 if entry_size == 20 else 2)
    entries = 12 * per
    p = client.plan(64, t, dims, entries, entry_size, encoding, 3)
    # positions 0, 1 and per - 1 of a plaintext in pack mode; sizes: full, above E, 0, half, the largest the prefix holds, 1
    indices = [[0, per + 1, entries - 1], [2 % entries, 3 * per - 1, 7]]
    sizes = [[entry_size, entry_size + 5, 0], [entry_size // 2, (1 << (8 * max(width, 1))) - 1, 1]]
    rng = np.random.default_rng(sum(map(ord, name + mode)))
    plaintexts = np.stack([[reply_plaintexts(oracle, rng, p, t, indices[q][i], sizes[q][i]) for i in range(3)] for q in range(2)])
    assert int(plaintexts.max()) >= 1 << p["bits"] and int(plaintexts.max()) < t
    flat = ring.to_device(plaintexts.reshape(-1, 64))
    cts = ring.ours.encrypt(flat, ring.key, seeds(rng, 6 * R), seeds(rng, 6 * R), moduli_count=moduli_count)
    assert torch.equal(ring.ours.decrypt(cts, ring.key), flat)  # the parameter set decrypts, coefficients above 2^bits included
    response = cts.view(2, 3, R, 2, moduli_count, 64)
    keep = response.clone()
    got_entries, got_sizes = ring.ours.pir_decrypt_response(response, device_indices(indices), dims, entries, entry_size, encoding,
                                                            ring.key)
    full, full_sizes = ring.ours.pir_decrypt_response(response, None, dims, entries, entry_size, encoding, ring.key)
    assert torch.equal(response, keep)  # never written
    assert tuple(got_entries.shape) == (2, 3, entry_size) and tuple(full.shape) == (2, 3, R * p["bytes_per_plaintext"])
    for q in range(2):
        for i in range(3):
            data = client.reply_bytes(oracle, plaintexts[q, i], p["bits"])
            assert bytes(full[q, i].cpu().numpy()) == data, (name, mode, q, i)  # decryptFull
            assert int(full_sizes[q, i]) == len(data)
            entry, size = client.entry_of_reply(p, data, indices[q][i])
            assert bytes(got_entries[q, i].cpu().numpy()) == entry, (name, mode, q, i)
            assert int(got_sizes[q, i]) == size, (name, mode, q, i)
            if encoding:
                assert size == min(sizes[q][i], entry_size)  # the clamp, and the excess coefficients left the prefix alone
            else:
                assert size == entry_size
    # an empty batch
    none = ring.ours.pir_decrypt_response(response[:0], device_indices(indices)[:0], dims, entries, entry_size, encoding, ring.key)
    assert tuple(none[0].shape) == (0, 3, entry_size)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pack", "split"])
@pytest.mark.parametrize("degree", [64, 256])  # the rings of test_gpu_pir.py's whole-query test and of test_gpu_pir_database.py
def test_indices_to_entries_on_the_device(oracle, degree, mode):
    import torch

    t = oracle.generate_primes([17], True, degree)[0]
    ours = heamd.BfvContext(degree, t, oracle.generate_primes([40, 40, 40, 41], False, degree))
    L, bpp, dims, count = ours.L, degree * 16 // 8, [4, 3], 3
    rng = np.random.default_rng(degree + (mode == "split"))
    if mode == "pack":
        entry_size = 20
        per = bpp // 21
        entry_count, nil = 12 * per - 3, list(range(per, 2 * per))  # plaintext 1 holds empty entries only: nil
    else:
        entry_size, per = 2 * bpp + 76, 1  # three chunks
        entry_count, nil = 11, [4]
    entries, padded, sizes = _entries(rng, entry_count, entry_size)
    for e in nil:
        entries[e], sizes[e] = b"", 0
    assert len({len(e) for e in entries}) > 3  # the sizes vary
    database, present = ours.pir_process_database(torch.from_numpy(padded).cuda(), dims, entry_size, True, entry_sizes=sizes)
    chunks = database.shape[0]
    assert int((present == 0).sum()) >= chunks  # the nil plaintext, in every chunk
    plan = ours.pir_client_plan(dims, entry_count, entry_size, True, count)
    assert (plan["reply_ciphertext_count"], plan["entries_per_plaintext"]) == (chunks, per)
    key = ours.generate_secret_key(seeds(rng, 1))[0].contiguous()
    elements = ours.pir_evaluation_key_elements(plan["expanded_query_count"], "none")
    galois = ours.generate_galois_keys(key, elements, seeds(rng, len(elements), L), seeds(rng, len(elements), L))
    relin = ours.generate_relinearization_key(key, seeds(rng, L), seeds(rng, L))
    # the first and the last entry, a nil plaintext's, an all-zero entry of nonzero size (3), positions inside a plaintext
    indices = [[0, nil[0], entry_count - 1], [(per + 1) % entry_count, 3, 5]]
    assert not any(entries[3]) and len(entries[3]) > 0
    C = plan["query_ciphertext_count"]
    query, flag = ours.pir_generate_query(device_indices(indices), dims, entry_count, entry_size, True, key, seeds(rng, 2, C),
                                          seeds(rng, 2, C))
    assert int(flag.item()) == 0
    response = torch.stack([ours.pir_compute_response_to_query(dims, query[q], count, {e: galois[k] for k, e in enumerate(elements)},
                                                               relin, database, chunks, present_devices=present)
                            for q in range(2)]).contiguous()
    got_entries, got_sizes = ours.pir_decrypt_response(response, device_indices(indices), dims, entry_count, entry_size, True, key)
    for q in range(2):
        for i in range(count):
            entry = entries[indices[q][i]]
            assert int(got_sizes[q, i]) == len(entry), (q, i)
            assert bytes(got_entries[q, i].cpu().numpy()) == entry + bytes(entry_size - len(entry)), (q, i)


# ---- footprint -----------------------------------------------------------------------------------------------------------------------
def check_footprint(what, inputs, outputs, zeroed, workspace_bytes, invoke):
    """One call on one arena (tests/footprint.py): `inputs` {slab: uint8 device tensor} are only read, `outputs` {slab: bytes}
    are poisoned and written, `zeroed` {slab: bytes} are written slabs the caller zeroes, then the workspace.
    invoke(addresses, workspace_bytes) -> status.  -> {slab: bytes of the result}"""
    import torch

    assert workspace_bytes >= 32 and workspace_bytes % 16 == 0
    sizes = collections.OrderedDict((name, tensor.numel()) for name, tensor in inputs.items())
    sizes.update(outputs)
    sizes.update(zeroed)
    sizes["workspace"] = workspace_bytes
    results = list(outputs) + list(zeroed)
    arena = footprint.layout(sizes, tuple(results) + ("workspace",))
    backing = torch.empty(arena.total + footprint.ALIGN, dtype=torch.uint8, device="cuda")
    skew = -backing.data_ptr() % footprint.ALIGN
    memory = backing[skew: skew + arena.total]
    spans = {name: footprint.span(arena, name) for name in sizes}
    where = {name: memory.data_ptr() + begin for name, (begin, _) in spans.items()}

    def fill(poison):
        memory.fill_(footprint.GUARD_BYTE)
        for name, tensor in inputs.items():
            memory[slice(*spans[name])] = tensor.reshape(-1)
        for name in list(outputs) + ["workspace"]:
            memory[slice(*spans[name])] = poison
        for name in zeroed:
            memory[slice(*spans[name])] = 0
        return memory.clone()

    def call(at, nbytes):
        status = invoke(at, nbytes)
        torch.cuda.synchronize()
        return status

    runs = []
    for poison in footprint.POISONS:
        image, masked = footprint.expected_image(arena, fill(poison))
        assert call(where, workspace_bytes) == OK, (what, hex(poison), heamd.load_library().he_last_error_message())
        footprint.verify(arena, memory, image, masked, "%s over 0x%02X" % (what, poison))
        assert int(memory[slice(*spans["workspace"])].count_nonzero()) == 0, what  # zeroized once the stream has drained
        runs.append({name: memory[slice(*spans[name])].clone() for name in results})
    for name in results:
        assert torch.equal(runs[0][name], runs[1][name]), "%s: %s depends on what its outputs and workspace held" % (what, name)
    # workspace = NULL: the library's own scratch; the workspace slab is then one more slab to leave alone
    filled = fill(footprint.POISONS[0])
    assert call(dict(where, workspace=None), 0) == OK, what
    footprint.verify(arena, memory, filled, [spans[name] for name in results], "%s with workspace = NULL" % what)
    for name in results:
        assert torch.equal(memory[slice(*spans[name])], runs[0][name]), (what, name, "workspace = NULL")
    # 16 bytes short: refused, nothing launched
    filled = fill(footprint.POISONS[0])
    assert call(where, workspace_bytes - 16) == INVALID, what
    footprint.verify(arena, memory, filled, [], "%s with the workspace 16 bytes short" % what)
    return {name: tensor.cpu().numpy() for name, tensor in runs[0].items()}


def as_bytes(tensor):
    import torch

    return tensor.contiguous().view(torch.uint8).reshape(-1)


@pytest.mark.parametrize("word32", [False, True])
def test_generate_query_footprint(oracle, word32):
    """dims [40, 30], two indices, two queries: three ciphertexts per query, both selection values"""
    ring = ring_for(oracle, 64, T17, word32)
    lib, bits, word_bytes = heamd.load_library(), 32 if word32 else 64, 4 if word32 else 8
    dims, entries, count, queries = (ctypes.c_uint32 * 2)(40, 30), 7197, 2, 2
    p = client.plan(64, T17, [40, 30], entries, 20, True, count)
    C = p["query_ciphertext_count"]
    rng = np.random.default_rng(11)
    indices = [[0, entries - 1], [7, 3600]]
    inputs = collections.OrderedDict([("indices", as_bytes(device_indices(indices))), ("secret_key", as_bytes(ring.key)),
                                      ("a_seeds", as_bytes(seeds(rng, queries, C))), ("error_seeds", as_bytes(seeds(rng, queries, C)))])
    parameter = (dims, 2, entries, 20, 1, count)
    needed = int(lib.he_pir_generate_query_workspace_bytes(ring.ours.h, bits, *parameter, queries))

    def invoke(at, nbytes):
        return lib.he_pir_generate_query_device(ring.ours.h, bits, *parameter, vp(at["indices"]), queries, vp(at["secret_key"]),
                                                vp(at["a_seeds"]), vp(at["error_seeds"]), vp(at["out"]), vp(at["out_of_range"]),
                                                vp(at["workspace"]), nbytes, None)

    got = check_footprint("he_pir_generate_query_device u%d" % bits, inputs,
                          {"out": queries * C * 2 * ring.L * 64 * word_bytes}, {"out_of_range": 4}, needed, invoke)
    assert not got["out_of_range"].any()
    a_host = inputs["a_seeds"].cpu().numpy().reshape(queries, C, 32)
    e_host = inputs["error_seeds"].cpu().numpy().reshape(queries, C, 32)
    expected = np.stack([client.generate_query(ring.poly_ctx(ring.L), T17, p, indices[q], ring.s_eval, [bytes(s) for s in a_host[q]],
                                               [bytes(s) for s in e_host[q]], ring.stream) for q in range(queries)])
    words = got["out"].view(np.uint32 if word32 else np.uint64).astype(np.uint64)
    assert np.array_equal(words, expected.reshape(-1))


@pytest.mark.parametrize("word32", [False, True])
@pytest.mark.parametrize("mode", ["pack-prefix", "split-prefix"])
def test_decrypt_response_footprint(oracle, mode, word32):
    ring = ring_for(oracle, 64, T9, word32)
    lib, bits = heamd.load_library(), 32 if word32 else 64
    entry_size, encoding = REPLY_MODES[mode]
    probe = client.plan(64, T9, [4, 3], 0, entry_size, encoding, 3)
    per, R = probe["entries_per_plaintext"], probe["reply_ciphertext_count"]
    entries, count, queries = 12 * per, 3, 2
    p = client.plan(64, T9, [4, 3], entries, entry_size, encoding, count)
    indices = [[0, per + 1, entries - 1], [2 % entries, 3 * per - 1, 7]]
    sizes = [[entry_size, entry_size + 5, 0], [entry_size // 2, 1, 3]]
    rng = np.random.default_rng(len(mode) + word32)
    plaintexts = np.stack([[reply_plaintexts(oracle, rng, p, T9, indices[q][i], sizes[q][i]) for i in range(3)] for q in range(2)])
    cts = ring.ours.encrypt(ring.to_device(plaintexts.reshape(-1, 64)), ring.key, seeds(rng, 6 * R), seeds(rng, 6 * R), moduli_count=1)
    inputs = collections.OrderedDict([("response", as_bytes(cts)), ("indices", as_bytes(device_indices(indices))),
                                      ("secret_key", as_bytes(ring.key[:1]))])
    parameter = ((ctypes.c_uint32 * 2)(4, 3), 2, entries, entry_size, int(encoding), count)
    needed = int(lib.he_pir_decrypt_response_workspace_bytes(ring.ours.h, bits, *parameter, 1, queries))

    def invoke(at, nbytes):
        return lib.he_pir_decrypt_response_device(ring.ours.h, bits, *parameter, 1, vp(at["response"]), vp(at["indices"]), queries,
                                                  vp(at["secret_key"]), vp(at["out_entries"]), vp(at["out_sizes"]),
                                                  vp(at["workspace"]), nbytes, None)

    got = check_footprint("he_pir_decrypt_response_device u%d %s" % (bits, mode), inputs,
                          {"out_entries": queries * count * entry_size, "out_sizes": queries * count * 8}, {}, needed, invoke)
    expected = [client.entry_of_reply(p, client.reply_bytes(oracle, plaintexts[q, i], p["bits"]), indices[q][i])
                for q in range(2) for i in range(3)]
    assert bytes(got["out_entries"]) == b"".join(entry for entry, _ in expected)
    assert list(got["out_sizes"].view(np.uint64)) == [size for _, size in expected]
