// simple_pir_shard.hpp -- the launchers of simple_pir_shard_kernels.hip: DatabaseMap.shardDatabase (reference Sources/
// PrivateInformationRetrieval/SimplePir/DatabaseMap.swift:82-110) as a map of chunks to shard rows and a scatter of the value
// bytes, and the index lists and the assembly of SimplePirClientForAllShards (SimplePir+Shards.swift:71-99, :139-171).  The
// entries: simple_pir_shard_api.cpp; the form choice and the tile arithmetic: simple_pir_shard_plan.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "simple_pir_shard_plan.hpp"

namespace heamd {

// The arrays he_simple_pir_shard_map_device writes (include/he_amd.h), as the other kernels read them.
struct SimplePirShardMapView {
    const uint64_t* chunk_starts;      // [count + 1]
    const uint32_t* chunk_shard;       // [total_chunks]
    const uint32_t* chunk_index;       // [total_chunks]
    const uint64_t* shard_row_starts;  // [shard_count + 1]
    const uint32_t* row_chunk;         // [total_chunks]
    uint64_t count, shard_count, chunk_size, total_chunks;
};

// sums: plan.sum_elements 4-byte words, scan: plan.scan_elements 8-byte words (scratch).  mismatch: optional.
hipError_t launch_simple_pir_shard_map(const uint64_t* value_offsets, const uint8_t* shard_orders, uint64_t count,
                                       uint64_t shard_count, uint64_t chunk_size, uint64_t total_chunks,
                                       const simple_pir_shard::Plan& plan, uint64_t* chunk_starts, uint32_t* chunk_shard,
                                       uint32_t* chunk_index, uint64_t* shard_row_starts, uint32_t* row_chunk, uint32_t* mismatch,
                                       uint32_t* sums, uint64_t* scan, hipStream_t stream);
// shards [total_chunks][chunk_size], every byte; values is read below values_bytes only
hipError_t launch_simple_pir_shard_scatter(const uint8_t* values, uint64_t values_bytes, const uint64_t* value_offsets,
                                           const SimplePirShardMapView& map, simple_pir_shard::Form form, uint8_t* shards,
                                           hipStream_t stream);
// out_indices [shard_count][batch][chunks_per_shard], out_found [batch]
hipError_t launch_simple_pir_shard_query_indices(const uint64_t* entry_positions, uint64_t batch, const SimplePirShardMapView& map,
                                                 uint64_t maximum_chunk_count, uint64_t chunks_per_shard, uint64_t* out_indices,
                                                 uint32_t* out_found, hipStream_t stream);
// out_entries [batch][maximum_chunk_count * chunk_size], out_sizes [batch], out_found [batch]
hipError_t launch_simple_pir_shard_assemble(const uint8_t* chunks, const uint64_t* indices, const uint64_t* entry_positions,
                                            uint64_t batch, const uint64_t* value_offsets, const SimplePirShardMapView& map,
                                            uint64_t maximum_chunk_count, uint64_t chunks_per_shard, simple_pir_shard::Form form,
                                            uint8_t* out_entries, uint64_t* out_sizes, uint32_t* out_found, hipStream_t stream);

}  // namespace heamd
