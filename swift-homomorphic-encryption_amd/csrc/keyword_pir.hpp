// keyword_pir.hpp -- the device side of KeywordPirServer.process (reference Sources/PrivateInformationRetrieval/KeywordPir/
// KeywordPirProtocol.swift:191-247): HashKeyword, ShardingFunction and HashBucket.serialize (keyword_pir_kernels.hip).  The
// cuckoo placement between them is host code (keyword_pir.cpp); the entries and the table object are keyword_pir_api.cpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace heamd {

constexpr uint32_t kKeywordPirMaxHashFunctions = 8;

// HashKeyword.hash (HashBucket.swift:264-269): keyword i is blob[offsets[i], offsets[i + 1]); count <= 2^32 - 1
hipError_t launch_keyword_hash(const uint8_t* blob, const uint64_t* offsets, size_t count, uint64_t* hashes, hipStream_t stream);
// HashKeyword.hashIndices (HashBucket.swift:221-257): indices [count][h], h in 1 .. kKeywordPirMaxHashFunctions
hipError_t launch_keyword_hash_indices(const uint64_t* hashes, size_t count, uint64_t bucket_count, uint32_t h,
                                       uint32_t* indices, hipStream_t stream);
// ShardingFunction.shardIndex (KeywordDatabase.swift:56-62,103-111); other_shard_count 0: sha256, else doubleMod
hipError_t launch_keyword_shard_indices(const uint64_t* hashes, size_t count, uint64_t shard_count, uint64_t other_shard_count,
                                        uint32_t* out, hipStream_t stream);

// The buckets of a table as a CSR pair over the entry arrays.
struct HashBucketTable {
    const uint64_t* hashes = nullptr;          // [entries] keyword hashes
    const uint8_t* values = nullptr;           // the value blob
    const uint64_t* value_offsets = nullptr;   // [entries + 1] into the blob
    const uint32_t* bucket_offsets = nullptr;  // [bucket_count + 1] into slot_entries
    const uint32_t* slot_entries = nullptr;    // [placed] entry indices, bucket after bucket in slot order
    uint64_t bucket_count = 0, entry_size = 0;
};
// Where each slot's record starts in its bucket's row (1 + the records before it): slot_starts [placed].  mismatch
// (optional, a zeroed device word): bit 0 when a bucket's serialization is longer than entry_size, bit 1 when a bucket has
// more than 255 slots.
hipError_t launch_hash_bucket_slot_starts(const HashBucketTable& table, uint32_t* slot_starts, uint32_t* mismatch,
                                          hipStream_t stream);
// HashBucket.serialize (HashBucket.swift:90-103,177-187) of bucket b at out + b * entry_size, zero padded to entry_size
hipError_t launch_hash_bucket_serialize(const HashBucketTable& table, const uint32_t* slot_starts, uint8_t* out,
                                        hipStream_t stream);

}  // namespace heamd
