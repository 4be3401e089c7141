// simple_pir_shard_plan.hpp -- what the SimplePIR sharding entries run for a shape: DatabaseMap.shardDatabase (reference
// Sources/PrivateInformationRetrieval/SimplePir/DatabaseMap.swift:82-110) and SimplePirClientForAllShards
// (SimplePir+Shards.swift:47-173).  Plain C++ (no HIP include): a host compiler builds it, and tests/c/simple_pir_shard_form.cpp
// holds the form choice to its restatement in tests/simple_pir_shard_reference.py without a device, so a device test can say
// which form its case ran.
//
// The byte movers (the scatter of the values into the shard slab, the assembly of decrypted chunks into entries) own aligned
// pieces of what they write:
//   wide  16 bytes per lane: both addresses on 16-byte boundaries and chunk_size a multiple of 16;
//   word  8 bytes per lane: both on 8-byte boundaries and chunk_size a multiple of 8;
//   byte  everything else;
//   none  nothing to write.
// A piece never crosses a row of chunk_size bytes, so a lane reads one chunk.  The scatter's source (`values`) may lie at any
// byte address in every form: only the slab it writes counts (pass 0 for `other`).
#pragma once

#include <cstddef>
#include <cstdint>

namespace heamd {
namespace simple_pir_shard {

enum class Form : uint32_t { kNone = 0, kByte = 1, kWord = 2, kWide = 3 };

constexpr uint32_t piece_bytes(Form form) { return form == Form::kWide ? 16 : form == Form::kWord ? 8 : form == Form::kByte ? 1 : 0; }

// the form of a mover that writes `bytes` bytes in rows of chunk_size at `written` (and reads aligned rows at `other`)
constexpr Form form(uintptr_t written, uintptr_t other, uint64_t chunk_size, uint64_t bytes) {
    if (bytes == 0 || chunk_size == 0) return Form::kNone;
    if (((written | other) & 15) == 0 && (chunk_size & 15) == 0) return Form::kWide;
    if (((written | other) & 7) == 0 && (chunk_size & 7) == 0) return Form::kWord;
    return Form::kByte;
}

constexpr size_t kMaxShardCount = 256;           // an order is a row of bytes
constexpr uint64_t kMaxCount = 0xfffffffeull;    // entries: 2^32 - 2
constexpr uint64_t kMaxChunks = 0xffffffffull;   // chunks of all entries: 2^32 - 1
constexpr uint32_t kMapTile = 128;               // entries of one workgroup in the two map passes: one per lane
constexpr uint32_t kThreads = 256;               // lanes of every other workgroup
constexpr uint32_t kScanTile = 1024;             // keyword_shard.hpp's: elements of one workgroup in a scan

constexpr uint64_t ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b != 0 ? 1 : 0); }

// elements of the scratch an exclusive scan over n elements needs (keyword_shard.hpp: scan_scratch_elements)
constexpr size_t scan_scratch_elements(size_t n) {
    size_t elements = 0;
    for (size_t blocks = n == 0 ? 1 : ceil_div(n, kScanTile); blocks > 1; blocks = ceil_div(blocks, kScanTile)) elements += blocks;
    return elements;
}

struct Plan {
    uint64_t total_chunks = 0;         // sum of ceil(len_e / chunk_size)
    uint64_t maximum_chunk_count = 0;  // ShardMap.maximumChunkCount
    uint64_t chunks_per_shard = 0;     // ceil(maximum_chunk_count / shard_count): ShardMap.chunksPerShard when every shard is used
    size_t map_tiles = 0;              // workgroups of the reduce and of the apply pass: ceil(count / kMapTile)
    size_t count_workgroups = 0;       // workgroups of the chunk-count pass: ceil((count + 1) / kThreads)
    size_t sum_elements = 0;           // 4-byte words: shard_count x map_tiles tile sums and the sums of their scan
    size_t scan_elements = 0;          // 8-byte words: the sums of the scan of the chunk counts
    size_t scratch_bytes() const { return scan_elements * 8 + sum_elements * 4; }
};

enum class PlanError { kNone = 0, kShardCount, kChunkSize, kCount, kOffsets, kChunks };

// the launch shape and scratch of the map: a function of the two counts alone (the device entry has no offsets on the host)
inline void map_shape(uint64_t count, uint64_t shard_count, Plan& p) {
    p.map_tiles = static_cast<size_t>(ceil_div(count, kMapTile));
    p.count_workgroups = static_cast<size_t>(ceil_div(count + 1, kThreads));
    const size_t sums = static_cast<size_t>(shard_count) * p.map_tiles;
    p.sum_elements = sums + scan_scratch_elements(sums);
    p.scan_elements = scan_scratch_elements(static_cast<size_t>(count) + 1);
}

// value_offsets: HOST [count + 1] (may be null when count is 0)
inline PlanError plan(const uint64_t* value_offsets, uint64_t count, uint64_t shard_count, uint64_t chunk_size, Plan& out) {
    if (shard_count == 0 || shard_count > kMaxShardCount) return PlanError::kShardCount;
    if (chunk_size == 0) return PlanError::kChunkSize;
    if (count > kMaxCount) return PlanError::kCount;
    Plan p;
    for (uint64_t e = 0; e < count; ++e) {
        if (value_offsets[e + 1] < value_offsets[e]) return PlanError::kOffsets;
        const uint64_t chunks = ceil_div(value_offsets[e + 1] - value_offsets[e], chunk_size);
        if (chunks > kMaxChunks - p.total_chunks) return PlanError::kChunks;
        p.total_chunks += chunks;
        if (chunks > p.maximum_chunk_count) p.maximum_chunk_count = chunks;
    }
    p.chunks_per_shard = ceil_div(p.maximum_chunk_count, shard_count);
    map_shape(count, shard_count, p);
    out = p;
    return PlanError::kNone;
}

}  // namespace simple_pir_shard
}  // namespace heamd
