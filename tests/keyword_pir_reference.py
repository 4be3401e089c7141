"""Restatement of the reference's keyword-PIR database layers in Python over hashlib, independent of the library:
HashKeyword (Sources/PrivateInformationRetrieval/KeywordPir/HashBucket.swift:208-270), ShardingFunction
(KeywordDatabase.swift:56-62,103-111), HashBucket.serialize / deserialize / find (HashBucket.swift:44-206), CuckooTableConfig
(CuckooTable.swift:18-157) and the placement of CuckooTable.insert / insertLoop (:386-458) as csrc/keyword_pir.cpp states it:
duplicates by keyword hash, splitmix64 over a seed for the evicted slot, and an expansion that starts over with every entry."""
import hashlib
import math
import struct

MAX_RETRIES = 10
MAX_VALUE_SIZE = 0xFFFF
MAX_SLOT_COUNT = 0xFF
MASK64 = (1 << 64) - 1


class PirError(Exception):
    def __init__(self, name, detail=""):
        self.name = name
        super().__init__(f"{name} {detail}".strip())


def keyword_hash(keyword):
    """HashKeyword.hash: SHA-256 truncated to 8 bytes, read little-endian"""
    return int.from_bytes(hashlib.sha256(bytes(keyword)).digest()[:8], "little")


def index_from_hash(hash_, bucket_count, counter):
    digest = hashlib.sha256(hash_.to_bytes(8, "big") + bytes([counter])).digest()
    return int.from_bytes(digest[:8], "little") % bucket_count


def hash_indices_of_hash(hash_, bucket_count, hash_function_count):
    candidates = []
    for _ in range(hash_function_count):
        counter = 0
        index = index_from_hash(hash_, bucket_count, counter)
        while index in candidates and counter < MAX_RETRIES:
            counter += 1
            index = index_from_hash(hash_, bucket_count, counter)
        candidates.append(index)
    return candidates


def hash_indices(keyword, bucket_count, hash_function_count):
    """HashKeyword.hashIndices"""
    return hash_indices_of_hash(keyword_hash(keyword), bucket_count, hash_function_count)


def shard_index(keyword, shard_count, other_shard_count=0):
    """ShardingFunction.shardIndex: sha256, or doubleMod with other_shard_count"""
    hash_ = keyword_hash(keyword)
    if other_shard_count:
        hash_ %= other_shard_count
    return hash_ % shard_count


def serialized_size(value_sizes):
    """HashBucket.serializedSize(values:)"""
    return 1 + sum(10 + size for size in value_sizes)


def serialize_bucket(slots):
    """HashBucket.serialize: slots = [(keyword hash, value bytes)]"""
    if len(slots) > MAX_SLOT_COUNT:
        raise PirError("invalidHashBucketSlotCount")
    data = bytes([len(slots)])
    for hash_, value in slots:
        if len(value) > MAX_VALUE_SIZE:
            raise PirError("invalidHashBucketEntryValueSize")
        data += struct.pack("<QH", hash_, len(value)) + bytes(value)
    return data


def deserialize_bucket(raw):
    """HashBucket(deserialize:): bytes behind the last slot are ignored -> [(hash, value)]"""
    raw = bytes(raw)
    if not raw:
        raise PirError("corruptedData")
    slots, offset = [], 1
    for _ in range(raw[0]):
        if len(raw) < offset + 10:
            raise PirError("corruptedData")
        hash_, size = struct.unpack_from("<QH", raw, offset)
        offset += 10
        if offset + size > len(raw):
            raise PirError("corruptedData")
        slots.append((hash_, raw[offset:offset + size]))
        offset += size
    return slots


def find(raw, keyword=None, hash_=None):
    """HashBucket.find: the first slot with the keyword's hash, or None"""
    wanted = keyword_hash(keyword) if hash_ is None else hash_
    for slot_hash, value in deserialize_bucket(raw):
        if slot_hash == wanted:
            return value
    return None


class Config:
    """CuckooTableConfig; bucket_count given: .fixedSize, None: .allowExpansion"""

    def __init__(self, hash_function_count, max_eviction_count, max_serialized_bucket_size, bucket_count=None,
                 expansion_factor=1.1, target_load_factor=0.9, multiple_tables=True, slot_count=MAX_SLOT_COUNT):
        self.hash_function_count = hash_function_count
        self.max_eviction_count = max_eviction_count
        self.max_serialized_bucket_size = max_serialized_bucket_size
        self.bucket_count = bucket_count
        self.expansion_factor = expansion_factor
        self.target_load_factor = target_load_factor
        self.multiple_tables = multiple_tables
        self.slot_count = slot_count

    @property
    def fixed_size(self):
        return self.bucket_count is not None

    @property
    def table_count(self):
        return self.hash_function_count if self.multiple_tables else 1

    def validate(self):
        valid = (self.hash_function_count > 0 and self.max_serialized_bucket_size >= serialized_size([0])
                 and 0 < self.slot_count <= MAX_SLOT_COUNT)
        if self.fixed_size:
            valid = valid and self.bucket_count > 0
        else:  # (a load factor that is not above 0: the reference would divide by it)
            valid = valid and self.expansion_factor > 1.0 and 0.0 < self.target_load_factor < 1.0
        if not valid:
            raise PirError("invalidCuckooConfig")


def next_multiple(value, of):
    return -(-value // of) * of


def initial_bucket_count(config, value_sizes):
    """CuckooTable.init (:339-349)"""
    config.validate()
    if config.fixed_size:
        return next_multiple(config.bucket_count, config.table_count)
    least = -(-serialized_size(value_sizes) // config.max_serialized_bucket_size)
    return next_multiple(int(math.ceil(float(least) / config.target_load_factor)), config.table_count)


def expanded_bucket_count(config, bucket_count):
    """CuckooTable.expand (:466-474)"""
    return next_multiple(int(math.ceil(float(bucket_count) * config.expansion_factor)), config.table_count)


class SplitMix64:
    def __init__(self, seed):
        self.state = seed & MASK64

    def next(self):
        self.state = (self.state + 0x9E3779B97F4A7C15) & MASK64
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
        return z ^ (z >> 31)


class NeedsExpansion(Exception):
    def __init__(self, next_bucket_count):
        self.next_bucket_count = next_bucket_count
        super().__init__(f"needs {next_bucket_count} buckets")


def place(config, hashes, indices, value_sizes, bucket_count, seed):
    """One pass of csrc/keyword_pir.cpp's he_keyword_pir_cuckoo_place -> (buckets: a list of entry indices per bucket,
    duplicates dropped).  Raises PirError or NeedsExpansion."""
    config.validate()
    h, tables, limit = config.hash_function_count, config.table_count, config.max_serialized_bucket_size
    assert bucket_count > 0 and bucket_count % tables == 0
    per_table = bucket_count // tables
    if any(size > MAX_VALUE_SIZE for size in value_sizes):
        raise PirError("invalidHashBucketEntryValueSize")
    assert all(index < per_table for row in indices for index in row)

    def bucket_of(entry, t):
        return indices[entry][t] if tables == 1 else t * per_table + indices[entry][t]

    def expansion():
        if config.fixed_size:
            return PirError("failedToConstructCuckooTable")
        return NeedsExpansion(expanded_bucket_count(config, bucket_count))

    buckets = [[] for _ in range(bucket_count)]
    sizes = [1] * bucket_count
    rng = SplitMix64(seed)
    duplicates = 0
    for i in range(len(hashes)):
        if serialized_size([value_sizes[i]]) > limit:
            raise PirError("failedToConstructCuckooTable", "single-entry bucket too large")
        held, remaining = i, config.max_eviction_count
        while True:
            if remaining == 0:
                raise expansion()
            if any(hashes[resident] == hashes[held] for t in range(h) for resident in buckets[bucket_of(held, t)]):
                duplicates += 1
                break
            record = 10 + value_sizes[held]
            for t in range(h):
                b = bucket_of(held, t)
                if len(buckets[b]) < config.slot_count and sizes[b] + record <= limit:
                    buckets[b].append(held)
                    sizes[b] += record
                    break
            else:
                swaps = [(bucket_of(held, t), slot) for t in range(h)
                         for slot, resident in enumerate(buckets[bucket_of(held, t)])
                         if sizes[bucket_of(held, t)] - (10 + value_sizes[resident]) + record <= limit]
                if not swaps:
                    raise expansion()
                b, slot = swaps[rng.next() % len(swaps)]
                evicted = buckets[b][slot]
                sizes[b] += record - (10 + value_sizes[evicted])
                buckets[b][slot] = held
                held = evicted
                remaining -= 1
                continue
            break
    return buckets, duplicates


class Table:
    """CuckooTable.init over (keyword, value) pairs, as the table object of the library builds it"""

    def __init__(self, config, keywords, values, seed=0):
        self.config = config
        self.hashes = [keyword_hash(k) for k in keywords]
        self.values = [bytes(v) for v in values]
        sizes = [len(v) for v in self.values]
        if any(size > MAX_VALUE_SIZE for size in sizes):
            raise PirError("invalidHashBucketEntryValueSize")
        self.bucket_count = initial_bucket_count(config, sizes)
        self.expansions = 0
        while True:
            per_table = self.bucket_count // config.table_count
            self.indices = [hash_indices_of_hash(hash_, per_table, config.hash_function_count) for hash_ in self.hashes]
            try:
                self.buckets, self.duplicates = place(config, self.hashes, self.indices, sizes, self.bucket_count, seed)
                break
            except NeedsExpansion as grow:
                assert grow.next_bucket_count > self.bucket_count
                self.bucket_count = grow.next_bucket_count
                self.expansions += 1
        self.buckets_per_table = self.bucket_count // config.table_count
        self.placed = sum(len(b) for b in self.buckets)

    def serialize_buckets(self):
        """CuckooTable.serializeBuckets()"""
        return [serialize_bucket([(self.hashes[e], self.values[e]) for e in bucket]) for bucket in self.buckets]

    def largest_bucket_size(self):
        return max(len(raw) for raw in self.serialize_buckets())

    def load_factor(self):
        """summarize() (:366-367), in Float"""
        import numpy as np

        total = sum(len(raw) for raw in self.serialize_buckets())
        return np.float32(total) / np.float32(self.bucket_count * self.config.max_serialized_bucket_size)

    def padded(self, entry_size):
        return [raw + bytes(entry_size - len(raw)) for raw in self.serialize_buckets()]
