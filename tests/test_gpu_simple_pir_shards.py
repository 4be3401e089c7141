"""SimplePIR over sharded databases on the device against tests/simple_pir_shard_reference.py, byte for byte: the
map and the scatter over the grid of tests/simple_pir_shard_cases.py with the values at an odd address, invalid order rows, a
wrong chunk count, the index lists, the assembly on slabs whose every slot holds other bytes, and the whole loop split -> process
-> precompute -> add_indices -> compute_response -> decrypt -> assemble at both word sizes.  Every array of a call lies in one
poisoned arena with guard bands, and every byte outside the stated outputs is compared after the call."""
import ctypes

import numpy as np
import pytest

import simple_pir_shard_cases as cases
import simple_pir_shard_reference as R

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
GUARD, GUARD_BYTE, POISON = 256, 0xA5, 0x5C


class Arena:
    """Named byte ranges in one device buffer, each on a 256-byte boundary plus its residue, GUARD bytes of padding at least
    between two.  Read ranges hold their content, written ones POISON, everything else GUARD_BYTE."""

    def __init__(self, specs):
        """specs: [(name, content bytes | byte count of a written range, residue)]"""
        import torch

        sizes = [len(spec[1]) if isinstance(spec[1], (bytes, bytearray, np.ndarray)) else int(spec[1]) for spec in specs]
        self.buffer = torch.empty(sum(sizes) + (2 * GUARD + 16) * (len(specs) + 1), dtype=torch.uint8, device="cuda")
        base = self.buffer.data_ptr()
        self.image = np.full(self.buffer.numel(), GUARD_BYTE, dtype=np.uint8)
        self.spans, self.written = {}, []
        cursor = 0
        for (name, content, residue), size in zip(specs, sizes):
            at = -(-(base + cursor + GUARD) // 256) * 256 + residue - base
            self.spans[name] = (at, at + size)
            if isinstance(content, (bytes, bytearray, np.ndarray)):
                self.image[at:at + size] = np.frombuffer(bytes(content), dtype=np.uint8) if size else 0
            else:
                self.image[at:at + size] = POISON
                self.written.append(name)
            cursor = at + size
        assert cursor + GUARD <= self.buffer.numel()
        self.buffer.copy_(torch.from_numpy(self.image))

    def ptr(self, name):
        return vp(self.buffer.data_ptr() + self.spans[name][0])

    def address(self, name):
        return self.buffer.data_ptr() + self.spans[name][0]

    def zero(self, name):
        begin, end = self.spans[name]
        self.image[begin:end] = 0
        self.buffer[begin:end] = 0

    def after(self):
        import torch

        torch.cuda.synchronize()
        return self.buffer.cpu().numpy()

    def got(self, name, dtype=np.uint8):
        begin, end = self.spans[name]
        return self.after()[begin:end].copy().view(dtype)

    def verify(self, expected, what):
        """expected: name -> the bytes a written range must hold (a range left out may hold anything).  Every other byte of
        the arena must be what it was."""
        after = self.after()
        image = self.image.copy()
        for name in self.written:
            begin, end = self.spans[name]
            if name in expected:
                image[begin:end] = np.frombuffer(bytes(expected[name]), dtype=np.uint8) if end > begin else 0
            else:
                image[begin:end] = after[begin:end]
        if not np.array_equal(after, image):
            byte = int(np.flatnonzero(after != image)[0])
            inside = [name for name, (begin, end) in self.spans.items() if begin <= byte < end]
            where = "%s+%d" % (inside[0], byte - self.spans[inside[0]][0]) if inside else "outside every range"
            raise AssertionError("%s: arena byte %d (%s) is %d, expected %d" % (what, byte, where, after[byte], image[byte]))


def words(values, dtype):
    return np.asarray(values, dtype=dtype).tobytes()


def status_name(status):
    import heamd

    return heamd.binding.STATUS_NAMES[status]


def split_arena(values, orders, shard_count, chunk_size, total_chunks, slab_residue=0):
    blob, offsets = cases.flat(values)
    count = len(values)
    return Arena([("value_offsets", words(offsets, np.uint64), 0),
                  ("shard_orders", words([v for order in orders for v in order], np.uint8), 0),
                  ("values", blob, 1),  # an odd address
                  ("chunk_starts", 8 * (count + 1), 0), ("chunk_shard", 4 * total_chunks, 0), ("chunk_index", 4 * total_chunks, 0),
                  ("shard_row_starts", 8 * (shard_count + 1), 0), ("row_chunk", 4 * total_chunks, 0), ("mismatch", 4, 0),
                  ("shards", total_chunks * chunk_size, slab_residue)]), blob, offsets


def run_map(arena, count, shard_count, chunk_size, total_chunks):
    import heamd

    arena.zero("mismatch")
    p = arena.ptr
    return status_name(heamd.load_library().he_simple_pir_shard_map_device(
        p("value_offsets"), p("shard_orders"), count, shard_count, chunk_size, total_chunks, p("chunk_starts"), p("chunk_shard"),
        p("chunk_index"), p("shard_row_starts"), p("row_chunk"), p("mismatch"), None))


def run_scatter(arena, count, chunk_size, total_chunks, values_bytes):
    import heamd

    p = arena.ptr
    return status_name(heamd.load_library().he_simple_pir_shard_scatter_device(
        p("values"), values_bytes, p("value_offsets"), count, chunk_size, total_chunks, p("chunk_starts"), p("row_chunk"),
        p("shards"), None))


def expected_split(values, orders, shard_count, chunk_size):
    """the arrays of the map by the closed forms and the slab by the line-for-line split"""
    lengths = [len(value) for value in values]
    arrays = R.device_map(lengths, orders, shard_count, chunk_size)
    _, shards = R.shard_database(list(enumerate(values)), arrays["orders"], shard_count, chunk_size)
    return {"chunk_starts": words(arrays["chunk_starts"], np.uint64), "chunk_shard": words(arrays["chunk_shard"], np.uint32),
            "chunk_index": words(arrays["chunk_index"], np.uint32), "shard_row_starts": words(arrays["shard_row_starts"], np.uint64),
            "row_chunk": words(arrays["row_chunk"], np.uint32), "mismatch": words([arrays["mismatch"]], np.uint32),
            "shards": b"".join(row for shard in shards for row in shard)}, arrays


# ---- the map and the scatter over the grid ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.GRID, ids=lambda case: case.name)
def test_map_and_scatter(case):
    import heamd

    values, orders = cases.database(case)
    S, C, count = case.shard_count, case.chunk_size, case.count
    expected, arrays = expected_split(values, orders, S, C)
    total = arrays["chunk_starts"][-1]
    arena, blob, offsets = split_arena(values, orders, S, C, total, case.slab_residue)
    assert arena.address("values") % 2 == 1 and arena.address("shards") % 16 == case.slab_residue
    plan = heamd.simple_pir_shard_plan(offsets, S, C, arena.address("shards"))
    assert plan == R.plan([len(value) for value in values], S, C, arena.address("shards")), case.name
    wanted_form = "none" if total == 0 else "wide" if C % 16 == 0 and case.slab_residue == 0 else "word" if C % 8 == 0 else "byte"
    assert plan["scatter_form"] == wanted_form and plan["total_chunks"] == total
    assert run_map(arena, count, S, C, total) == "ok"
    assert run_scatter(arena, count, C, total, len(blob)) == "ok"
    arena.verify(expected, case.name)


def test_the_grid_covers_what_it_claims():
    seen_counts = {(case.shard_count, case.count) for case in cases.GRID} | {("C", case.chunk_size, case.count) for case in cases.GRID}
    for count in cases.COUNTS:
        assert all((S, count) in seen_counts for S in cases.SHARD_COUNTS) and all(("C", C, count) in seen_counts for C in cases.CHUNK_SIZES)
    assert {(case.chunk_size % 16 == 0, case.slab_residue) for case in cases.GRID} >= {(True, 0), (True, 8), (False, 0)}
    big = next(case for case in cases.GRID if case.count > 3 * cases.TILE and case.shard_count == 5)
    values, _ = cases.database(big)
    lengths = [len(value) for value in values]
    assert lengths[:5] == [0, 1, big.chunk_size, 5 * big.chunk_size, 5 * big.chunk_size + 1] and max(lengths) > 250


# ---- invalid orders, a wrong chunk count ----------------------------------------------------------------------------------------------
def test_invalid_order_rows_set_bit_0_and_split_under_the_identity():
    rng = np.random.default_rng(5)
    S, C = 3, 2
    values = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in (7, 9, 0, 13, 4, 11)]
    orders = [[2, 0, 1], [1, 1, 0], [0, 2, 1], [0, 3, 1], [2, 1, 0], [255, 255, 255]]  # a repeat; a value >= S; both
    expected, arrays = expected_split(values, orders, S, C)
    assert arrays["mismatch"] == 1 and arrays["orders"][1] == [0, 1, 2] and arrays["orders"][3] == [0, 1, 2] and arrays["orders"][0] == [2, 0, 1]
    total = arrays["chunk_starts"][-1]
    arena, blob, _ = split_arena(values, orders, S, C, total)
    assert run_map(arena, len(values), S, C, total) == "ok" and run_scatter(arena, len(values), C, total, len(blob)) == "ok"
    arena.verify(expected, "invalid orders")
    good = [order if R.valid_order(order, S) else [0, 1, 2] for order in orders]
    arena, blob, _ = split_arena(values, good, S, C, total)
    assert run_map(arena, len(values), S, C, total) == "ok"
    assert arena.got("mismatch", np.uint32)[0] == 0


@pytest.mark.parametrize("delta", (-3, 2))
def test_a_wrong_chunk_count_sets_bit_1_and_keeps_the_guards(delta):
    case = next(case for case in cases.GRID if case.count > 3 * cases.TILE and case.shard_count == 3)
    values, orders = cases.database(case)
    S, C = case.shard_count, case.chunk_size
    _, arrays = expected_split(values, orders, S, C)
    claim = arrays["chunk_starts"][-1] + delta
    arena, blob, _ = split_arena(values, orders, S, C, claim)
    assert run_map(arena, case.count, S, C, claim) == "ok"
    assert arena.got("mismatch", np.uint32)[0] == 2
    assert run_scatter(arena, case.count, C, claim, len(blob)) == "ok"
    arena.verify({"mismatch": words([2], np.uint32), "chunk_starts": words(arrays["chunk_starts"], np.uint64)}, "claim %+d" % delta)


# ---- the client half -------------------------------------------------------------------------------------------------------------------
class Client:
    """A database split on the host by the line-for-line restatement, its map on the device, and lookups: present entries (the
    first -- its chunk at index 0 stands behind fake slots --, one with more than S chunks, one of size 0), and absent ones."""

    def __init__(self, chunk_size, shard_count=3):
        import torch

        rng = np.random.default_rng(chunk_size)
        self.S, self.C = shard_count, chunk_size
        lengths = [1, 0, chunk_size * (2 * shard_count + 2) - 1, 3 * chunk_size, chunk_size * shard_count + 1, 2, 5 * chunk_size]
        self.values = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in lengths]
        self.orders = [[int(v) for v in rng.permutation(shard_count)] for _ in lengths]
        self.count = len(lengths)
        self.database_map, self.shards = R.shard_database(list(enumerate(self.values)), self.orders, shard_count, chunk_size)
        self.shard_map = R.ShardMap(self.database_map)
        assert self.shard_map.shard_count == shard_count and self.shard_map.maximum_chunk_count == 2 * shard_count + 2
        self.arrays = R.device_map(lengths, self.orders, shard_count, chunk_size)
        self.total = self.arrays["chunk_starts"][-1]
        self.lookups = [0, 2, 1, self.count, 4, 6, self.count + 9, 2**40, 3]
        self.M, self.cps = self.shard_map.maximum_chunk_count, self.shard_map.chunks_per_shard
        self.lists = [R.query_indices(self.shard_map, shard_count, index) for index in self.lookups]  # [B][S][cps]
        self.torch = torch

    def map_specs(self):
        _, offsets = cases.flat(self.values)
        return [("value_offsets", words(offsets, np.uint64), 0), ("chunk_starts", words(self.arrays["chunk_starts"], np.uint64), 0),
                ("chunk_shard", words(self.arrays["chunk_shard"], np.uint32), 0),
                ("chunk_index", words(self.arrays["chunk_index"], np.uint32), 0)]

    def plane_indices(self):
        """[S][B][cps]"""
        return [[self.lists[b][s] for b in range(len(self.lookups))] for s in range(self.S)]


@pytest.mark.parametrize("chunk_size", (4, 8, 16))
def test_query_indices(chunk_size):
    import heamd

    c = Client(chunk_size)
    B = len(c.lookups)
    arena = Arena(c.map_specs() + [("entry_positions", words(c.lookups, np.uint64), 0), ("out_indices", 8 * c.S * B * c.cps, 0),
                                   ("out_found", 4 * B, 0)])
    p = arena.ptr
    assert status_name(heamd.load_library().he_simple_pir_shard_query_indices_device(
        p("entry_positions"), B, c.count, c.S, c.total, c.M, c.cps, p("chunk_starts"), p("chunk_shard"), p("chunk_index"),
        p("out_indices"), p("out_found"), None)) == "ok"
    arena.verify({"out_indices": words(c.plane_indices(), np.uint64),
                  "out_found": words([1 if index < c.count else 0 for index in c.lookups], np.uint32)}, "query indices")
    many = c.shard_map.get(2).chunks  # more than S chunks: several real indices per shard, in chunk order
    assert len(many) > c.S and c.lists[c.lookups.index(2)][many[0].shard_index][:2] == [many[0].index, many[c.S].index]
    assert c.lists[c.lookups.index(c.count)] == [[0] * c.cps] * c.S


@pytest.mark.parametrize("chunk_size,residue", ((4, 0), (8, 0), (16, 0), (16, 8), (16, 3)))
def test_assemble_takes_the_last_matching_slot(chunk_size, residue):
    import heamd

    c = Client(chunk_size)
    B = len(c.lookups)
    rng = np.random.default_rng(77)
    chunks = rng.integers(0, 256, size=(c.S, B, c.cps, c.C), dtype=np.uint8)  # other bytes in every slot
    for b, index in enumerate(c.lookups):  # ...and the true chunk wherever a slot asks for a real index (fake slots keep garbage)
        entry = c.shard_map.get(index)
        for location in (entry.chunks if entry is not None else []):
            slot = max(j for j, v in enumerate(c.lists[b][location.shard_index]) if v == location.index)
            chunks[location.shard_index, b, slot] = np.frombuffer(c.shards[location.shard_index][location.index], dtype=np.uint8)
    entries, sizes, found = [], [], []
    for b, index in enumerate(c.lookups):
        decrypted = [[bytes(chunks[s, b, j]) for j in range(c.cps)] for s in range(c.S)]
        result = R.assemble(c.shard_map, decrypted, c.lists[b], index)
        if result is not None:
            assert result == c.values[index]
        entries.append((result or b"") + bytes(c.M * c.C - len(result or b"")))
        sizes.append(len(result) if result is not None else 0)
        found.append(0 if result is None else 1)
    first = c.lookups.index(0)  # a real chunk at index 0 behind fake slots: the last slot that asks for index 0 answers
    location = c.shard_map.get(0).chunks[0]
    assert location.index == 0 and c.lists[first][location.shard_index] == [0] * c.cps and c.cps >= 2
    assert bytes(chunks[location.shard_index, first, c.cps - 1, :1]) == c.values[0] != bytes(chunks[location.shard_index, first, 0, :1])
    arena = Arena(c.map_specs() + [("entry_positions", words(c.lookups, np.uint64), 0), ("chunks", chunks.tobytes(), residue),
                                   ("indices", words(c.plane_indices(), np.uint64), 0), ("out_entries", B * c.M * c.C, 0),
                                   ("out_sizes", 8 * B, 0), ("out_found", 4 * B, 0)])
    p = arena.ptr
    assert status_name(heamd.load_library().he_simple_pir_shard_assemble_device(
        p("chunks"), p("indices"), p("entry_positions"), B, p("value_offsets"), c.count, c.S, c.C, c.total, c.M, c.cps,
        p("chunk_starts"), p("chunk_shard"), p("chunk_index"), p("out_entries"), p("out_sizes"), p("out_found"), None)) == "ok"
    arena.verify({"out_entries": b"".join(entries), "out_sizes": words(sizes, np.uint64), "out_found": words(found, np.uint32)},
                 "assemble")
    assert sizes[c.lookups.index(1)] == 0 and found[c.lookups.index(1)] == 1 and found[c.lookups.index(c.count)] == 0


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plaintext_bits,ciphertext_bits,word_bits", ((14, 42, 64), (7, 28, 32)))
def test_end_to_end_on_the_device(plaintext_bits, ciphertext_bits, word_bits):
    """split -> SimplePirServer.process per shard -> precompute -> add_indices -> compute_response -> decrypt -> assemble"""
    import heamd
    import torch

    rng = np.random.default_rng(word_bits)
    S, C, N, count = 3, 9, 64, 40
    values = [rng.integers(0, 256, size=int(rng.integers(0, 61)), dtype=np.uint8).tobytes() for _ in range(count)]
    orders = [[int(v) for v in rng.permutation(S)] for _ in range(count)]
    blob, offsets = cases.flat(values)
    original = [3 * e + 1 for e in range(count)]  # original indices that are not positions
    mismatch = torch.zeros(1, dtype=torch.int32, device="cuda")
    shard_map, shards = heamd.SimplePirDatabaseMap.shard_database(
        torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda(), offsets, orders, S, C, original, mismatch=mismatch)
    reference_map, reference_shards = R.shard_database(list(zip(original, values)), orders, S, C)
    reference = R.ShardMap(reference_map)
    assert int(mismatch.item()) == 0 and shard_map.scatter_form == "byte"
    assert (shard_map.shard_count, shard_map.maximum_chunk_count, shard_map.chunks_per_shard) == \
        (reference.shard_count, reference.maximum_chunk_count, reference.chunks_per_shard)
    for s in range(S):
        assert bytes(shards[s].cpu().numpy().tobytes()) == b"".join(reference_shards[s])
    seed = bytes(range(32))
    server_class = heamd.SimplePirServer if word_bits == 64 else heamd.SimplePirServer32
    servers = [server_class.process(shards[s], plaintext_bits, ciphertext_bits, N, seed) for s in range(S)]
    clients = [heamd.SimplePirClient(server.params, server.hint, seed, word_bits) for server in servers]
    with pytest.raises(ValueError):
        heamd.SimplePirClientForAllShards(shard_map, clients[:2])
    everything = heamd.SimplePirClientForAllShards(shard_map, clients)
    lookups = [original[0], original[-1], original[count // 2], 2]  # the first, the last, a middle entry, and no entry at all
    indices, found = everything.query_indices(lookups)
    assert found.cpu().tolist() == [1, 1, 1, 0]
    queries_per_shard = len(lookups) * shard_map.chunks_per_shard
    decrypted = []
    for s in range(S):
        per_entry = servers[s].params["chunks_per_entry"]
        secret_seeds = torch.from_numpy(rng.integers(0, 256, size=(queries_per_shard, per_entry, 32), dtype=np.uint8)).cuda()
        error_seeds = torch.from_numpy(rng.integers(0, 256, size=(queries_per_shard, 32), dtype=np.uint8)).cuda()
        queries, results = clients[s].precompute(secret_seeds, error_seeds)
        where = indices[s].reshape(-1).contiguous()
        assert not clients[s].add_indices(queries, where).any()
        responses = servers[s].compute_response(queries.reshape(-1, servers[s].params["database_columns"])).reshape(results.shape)
        got, flags = clients[s].decrypt(responses, results, where)
        assert not flags.any()
        decrypted.append(got.reshape(len(lookups), shard_map.chunks_per_shard, C))
    entries, sizes, found = everything.assemble(torch.stack(decrypted).contiguous(), indices, lookups)
    entries, sizes = entries.cpu().numpy(), sizes.cpu().tolist()
    assert found.cpu().tolist() == [1, 1, 1, 0] and sizes[3] == 0 and not entries[3].any()
    for b, index in enumerate(lookups[:3]):
        value = values[original.index(index)]
        assert sizes[b] == len(value) and bytes(entries[b, :sizes[b]]) == value and not entries[b, sizes[b]:].any()
