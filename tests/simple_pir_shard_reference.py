"""SimplePIR over sharded databases, restated from the reference line for line over Python lists: DatabaseMap.shardDatabase
(Sources/PrivateInformationRetrieval/SimplePir/DatabaseMap.swift:82-110) with the per-entry orders as an argument (the reference
shuffles with the system generator), ShardMap (SimplePir+Shards.swift:18-45), the index lists of SimplePirClientForAllShards.
query(for:) (:71-87) and the assembly of decrypt (:139-171) with its last-match search.  Beside them the closed forms the device
kernels use, the flat arrays of he_simple_pir_shard_map_device, and the form choice of csrc/simple_pir_shard_plan.hpp."""
import collections

ChunkLocation = collections.namedtuple("ChunkLocation", "shard_index index")
Entry = collections.namedtuple("Entry", "original_index size chunks")
DatabaseMap = collections.namedtuple("DatabaseMap", "entries chunk_size")

MAP_TILE, THREADS, SCAN_TILE = 128, 256, 1024  # csrc/simple_pir_shard_plan.hpp
FORMS = {"none": 0, "byte": 1, "word": 2, "wide": 3}


def shard_database(raw_entries, orders, shard_count, chunk_size):
    """DatabaseMap.shardDatabase: raw_entries [(original_index, bytes)], orders[e] the randomShards of entry e ->
    (DatabaseMap, shards: per shard a list of chunk_size-byte rows)."""
    entries = []
    shards = [[] for _ in range(shard_count)]
    for (original_index, value), random_shards in zip(raw_entries, orders):
        chunks = []
        pieces = [value[at:at + chunk_size] for at in range(0, len(value), chunk_size)]  # value.chunks(ofCount:)
        for chunk_index, chunk in enumerate(pieces):
            padded_chunk = bytes(chunk)
            if len(chunk) < chunk_size:
                padded_chunk += bytes(chunk_size - len(chunk))
            shard_index = random_shards[chunk_index % shard_count]
            chunks.append(ChunkLocation(shard_index, len(shards[shard_index])))
            shards[shard_index].append(padded_chunk)
        entries.append(Entry(original_index, len(value), chunks))
    return DatabaseMap(entries, chunk_size), shards


class ShardMap:
    """ShardMap.init(databaseMap:)"""

    def __init__(self, database_map):
        self.mapping = {}
        for entry in database_map.entries:
            self.mapping[entry.original_index] = entry  # of duplicate indices the last stays
        shards = set()
        for value in self.mapping.values():
            shards |= {chunk.shard_index for chunk in value.chunks}
        self.shard_count = len(shards)
        self.maximum_chunk_count = max((len(value.chunks) for value in self.mapping.values()), default=0)
        self.chunk_size = database_map.chunk_size
        # (dividingCeil by zero traps in the reference: a map without a chunk has no chunksPerShard)
        self.chunks_per_shard = -(-self.maximum_chunk_count // self.shard_count) if self.shard_count else 0

    def get(self, original_index):
        return self.mapping.get(original_index)


def query_indices(shard_map, client_count, index):
    """SimplePirClientForAllShards.query(for:) up to clients[s].query(at:): the index lists of all shards"""
    lists = [[] for _ in range(client_count)]
    entry = shard_map.get(index)
    if entry is not None:
        for chunk in entry.chunks:
            lists[chunk.shard_index].append(chunk.index)
    for shard_index in range(client_count):
        while len(lists[shard_index]) < shard_map.chunks_per_shard:
            lists[shard_index].append(0)
    return lists


def assemble(shard_map, decrypted, lists, index):
    """SimplePirClientForAllShards.decrypt behind the per-shard decryptions: decrypted[s][j] the bytes of query slot j of shard
    s, lists[s][j] that slot's index -> the entry's bytes, or None."""
    entry = shard_map.get(index)
    chunks = entry.chunks if entry is not None else []
    result = b""
    for chunk_index in range(shard_map.maximum_chunk_count):
        is_real_chunk = chunk_index < len(chunks)
        real_chunk = chunks[chunk_index] if is_real_chunk else ChunkLocation(0, 0)
        shard_index = real_chunk.shard_index if is_real_chunk else 0
        target_index = real_chunk.index if is_real_chunk else 0
        search_index = 0
        for idx, query_index in enumerate(lists[shard_index]):
            search_index = idx if query_index == target_index else search_index
        result += bytes(decrypted[shard_index][search_index][:shard_map.chunk_size])
    if entry is None:
        return None
    return result[:entry.size]


# ---- the closed forms of the device kernels ---------------------------------------------------------------------------------
def chunk_count(length, chunk_size):
    return -(-length // chunk_size)


def rows_given(chunks, order, shard, shard_count):
    """rows entry (chunks, order) gives `shard`: floor(c / S) + [order^-1(shard) < c mod S]"""
    return chunks // shard_count + (1 if order.index(shard) < chunks % shard_count else 0)


def closed_form_locations(lengths, orders, shard_count, chunk_size):
    """per entry the (shard, index) of every chunk: chunk k -> (order[k mod S], base[order[k mod S]] + floor(k / S))"""
    base = [0] * shard_count
    out = []
    for length, order in zip(lengths, orders):
        chunks = chunk_count(length, chunk_size)
        out.append([ChunkLocation(order[k % shard_count], base[order[k % shard_count]] + k // shard_count)
                    for k in range(chunks)])
        for position, shard in enumerate(order):  # rows_given(chunks, order, shard, S) with order^-1(shard) = position
            base[shard] += chunks // shard_count + (1 if position < chunks % shard_count else 0)
    return out


def valid_order(order, shard_count):
    return sorted(order) == list(range(shard_count))


def device_map(lengths, orders, shard_count, chunk_size):
    """The arrays of he_simple_pir_shard_map_device: a row that is no permutation is replaced by the identity (bit 0).
    -> dict(chunk_starts, chunk_shard, chunk_index, shard_row_starts, row_chunk, mismatch)"""
    mismatch = 0
    used = []
    for order in orders:
        order = [int(v) for v in order]
        if not valid_order(order, shard_count):
            mismatch |= 1
            order = list(range(shard_count))
        used.append(order)
    locations = closed_form_locations(lengths, used, shard_count, chunk_size)
    chunk_starts = [0]
    for per_entry in locations:
        chunk_starts.append(chunk_starts[-1] + len(per_entry))
    flat = [location for per_entry in locations for location in per_entry]
    per_shard = collections.Counter(location.shard_index for location in flat)
    rows = [per_shard[shard] for shard in range(shard_count)]
    shard_row_starts = [0]
    for count in rows:
        shard_row_starts.append(shard_row_starts[-1] + count)
    row_chunk = [0] * len(flat)
    for chunk, location in enumerate(flat):
        row_chunk[shard_row_starts[location.shard_index] + location.index] = chunk
    return {"chunk_starts": chunk_starts, "chunk_shard": [location.shard_index for location in flat],
            "chunk_index": [location.index for location in flat], "shard_row_starts": shard_row_starts, "row_chunk": row_chunk,
            "mismatch": mismatch, "orders": used}


# ---- csrc/simple_pir_shard_plan.hpp -------------------------------------------------------------------------------------------
def form(written, other, chunk_size, nbytes):
    if nbytes == 0 or chunk_size == 0:
        return "none"
    if (written | other) % 16 == 0 and chunk_size % 16 == 0:
        return "wide"
    if (written | other) % 8 == 0 and chunk_size % 8 == 0:
        return "word"
    return "byte"


def scan_scratch_elements(n):
    elements, blocks = 0, max(-(-n // SCAN_TILE), 1)
    while blocks > 1:
        elements += blocks
        blocks = -(-blocks // SCAN_TILE)
    return elements


def plan(lengths, shard_count, chunk_size, shards_address=0):
    """he_simple_pir_shard_plan, or the text of its refusal"""
    if not 1 <= shard_count <= 256:
        return "shard count"
    if chunk_size == 0:
        return "chunk size"
    count = len(lengths)
    if count > 2**32 - 2:
        return "count"
    chunks = [chunk_count(length, chunk_size) for length in lengths]
    total = sum(chunks)
    if total > 2**32 - 1:
        return "chunks"
    largest = max(chunks, default=0)
    tiles = -(-count // MAP_TILE)
    sums = shard_count * tiles
    return {"total_chunks": total, "maximum_chunk_count": largest, "chunks_per_shard": -(-largest // shard_count),
            "scatter_form": form(shards_address, 0, chunk_size, total * chunk_size), "map_tile_entries": MAP_TILE,
            "map_tiles": tiles, "count_workgroups": -(-(count + 1) // THREADS),
            "scratch_bytes": 8 * scan_scratch_elements(count + 1) + 4 * (sums + scan_scratch_elements(sums))}
