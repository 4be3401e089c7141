"""Restatement of the reference's database sharding in Python integers, independent of the library: Sharding (Sources/
PrivateInformationRetrieval/KeywordPir/KeywordDatabase.swift:152-268), the split of KeywordDatabase.init(rows:sharding:
shardingFunction:) (:406-437) as the library states it -- a stable partition of the rows by shard index, shards in input order
-- and the plan of the device partition (which digit passes and gather forms a shape runs)."""
import numpy as np

from keyword_pir_reference import PirError, shard_index  # noqa: F401  (shard_index is part of this module's surface)

ROWS_PER_WORKGROUP = 2048  # csrc/keyword_shard.hpp: kShardSortTile


class Sharding:
    """Sharding.init: exactly one of shard_count / entry_count_per_shard; max_shard_count None is nil"""

    def __init__(self, shard_count=None, entry_count_per_shard=None, max_shard_count=None, require_power_of_two=False):
        assert (shard_count is None) != (entry_count_per_shard is None)
        self.shard_count_value = shard_count
        self.entry_count_per_shard = entry_count_per_shard
        self.max_shard_count = max_shard_count
        self.require_power_of_two = bool(require_power_of_two)
        if shard_count is not None:
            if shard_count < 1:
                raise PirError("invalidSharding", "shardCount must be at least 1")
            if max_shard_count is not None and shard_count > max_shard_count:
                raise PirError("invalidSharding", "shardCount exceeds maxShardCount")
            if self.require_power_of_two and shard_count & (shard_count - 1):
                raise PirError("invalidSharding", "shardCount is not a power of two")
        else:
            if entry_count_per_shard < 1:
                raise PirError("invalidSharding", "entryCountPerShard must be at least 1")
            if max_shard_count == 0:  # the library's declared difference: the reference would resolve to no shard
                raise PirError("invalidSharding", "maxShardCount 0 leaves no shard")

    def shard_count(self, row_count):
        """shardCount(for:)"""
        if self.shard_count_value is not None:
            return self.shard_count_value
        count = max(row_count // self.entry_count_per_shard, 1)
        if self.max_shard_count is not None:
            count = min(count, self.max_shard_count)
        if self.require_power_of_two:
            count = 1 << (count.bit_length() - 1)  # previousPowerOfTwo
        return count


def partition(rows, indices, shard_count):
    """rows: [(keyword bytes, value bytes)], indices: one shard index per row (at or above shard_count: the last shard)
    -> (order, shard_starts, (keyword blob, value blob), (keyword offsets, value offsets)); shard_starts is a list, or
    above 65 536 shards an int64 array"""
    assert len(rows) == len(indices) and shard_count >= 1
    keys = [min(index, shard_count - 1) for index in indices]
    order = sorted(range(len(rows)), key=lambda row: keys[row])  # sorted() is stable: input order within a shard
    # (numpy only for speed at millions of shards: a count per shard and its running sum)
    per_shard = np.bincount(np.asarray(keys, dtype=np.int64), minlength=shard_count)
    shard_starts = [0] + np.cumsum(per_shard).tolist() if shard_count <= 1 << 16 else \
        np.concatenate(([0], np.cumsum(per_shard))).astype(np.int64)
    blobs, offsets = [], []
    for part in (0, 1):
        running = [0]
        for row in order:
            running.append(running[-1] + len(rows[row][part]))
        blobs.append(b"".join(bytes(rows[row][part]) for row in order))
        offsets.append(running)
    return order, shard_starts, tuple(blobs), tuple(offsets)


def plan(count, shard_count, keyword_bytes, value_bytes):
    """what he_keyword_database_partition_device runs"""
    workgroups = -(-count // ROWS_PER_WORKGROUP)
    return {
        "digit_passes": 0 if count == 0 else -(-(shard_count - 1).bit_length() // 8),
        "workgroups_per_pass": workgroups,
        "rows_per_workgroup": ROWS_PER_WORKGROUP,
        "last_workgroup_rows": count - (workgroups - 1) * ROWS_PER_WORKGROUP if count else 0,
        "keyword_gather_form": "chunk" if count and keyword_bytes else "none",
        "value_gather_form": "chunk" if count and value_bytes else "none",
    }
