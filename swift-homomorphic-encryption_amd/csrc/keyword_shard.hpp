// keyword_shard.hpp -- KeywordDatabase.init(rows:sharding:shardingFunction:) on the device (reference Sources/
// PrivateInformationRetrieval/KeywordPir/KeywordDatabase.swift:406-437): a stable counting sort of the rows by shard index
// and the gather of the two byte blobs into the new order (keyword_shard_kernels.hip).  The entries and the sharded-database
// object are keyword_shard_api.cpp; the shard count (Sharding, :152-268) is host code there too.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/he_amd.h"

namespace heamd {

constexpr uint32_t kShardSortTile = 2048;  // rows of one workgroup in an order pass: 256 lanes, 8 rounds
constexpr uint32_t kScanTile = 1024;       // elements of one workgroup in a scan: 256 lanes, 4 each

// What a partition call runs for a shape, on the host.
struct PartitionPlan {
    uint32_t digit_passes = 0;  // ceil(bits(shard_count - 1) / 8); none for one shard or no row
    size_t workgroups = 0;      // per order pass: ceil(count / kShardSortTile)
    size_t last_rows = 0;       // rows of the last workgroup
};
PartitionPlan partition_plan(size_t count, size_t shard_count);
// elements of the scratch an in-place exclusive scan over n elements needs (the workgroup sums of every level)
size_t scan_scratch_elements(size_t n);

// data[i] = data[0] + .. + data[i - 1], in place: reduce / scan of the sums / apply, separate launches, no kernel waits for
// another workgroup.  scratch: scan_scratch_elements(n) elements.
hipError_t launch_exclusive_scan(uint32_t* data, size_t n, uint32_t* scratch, hipStream_t stream);
hipError_t launch_exclusive_scan(uint64_t* data, size_t n, uint64_t* scratch, hipStream_t stream);

// The stable order of rows by min(shard_indices[row], shard_count - 1): order [count] (row j of the output is input row
// order[j]).  alternate [count] (read and written when plan.digit_passes >= 2) and counts [256 * plan.workgroups +
// scan_scratch_elements(that)] are scratch.  count >= 1.
hipError_t launch_shard_order(const uint32_t* shard_indices, size_t count, size_t shard_count, const PartitionPlan& plan,
                              uint32_t* order, uint32_t* alternate, uint32_t* counts, hipStream_t stream);
// shard_starts [shard_count + 1]: the first output row of every shard, by lower-bound search over the sorted indices
hipError_t launch_shard_starts(const uint32_t* shard_indices, const uint32_t* order, size_t count, size_t shard_count,
                               uint32_t* shard_starts, hipStream_t stream);
// out_offsets [count + 1] = the lengths of the rows in the new order (and 0 behind them): the input of the scan.  mismatch
// (optional): bit 0 for an index >= shard_count, bit 1 when offsets[count] - offsets[0] is not `bytes`.
hipError_t launch_row_lengths(const uint64_t* offsets, const uint32_t* order, size_t count, uint64_t bytes,
                              const uint32_t* shard_indices, size_t shard_count, uint64_t* out_offsets, uint32_t* mismatch,
                              hipStream_t stream);
// out [0, min(bytes, out_offsets[count])) = the rows of blob in the new order, back to back (chunk form).  tile_rows: scratch
// of gather_scratch_elements(bytes) words -- the row every 512 output bytes start in, found first so that a lane's own search
// spans a few rows.
size_t gather_scratch_elements(uint64_t bytes);
hipError_t launch_blob_gather(const uint8_t* blob, const uint64_t* offsets, const uint32_t* order, const uint64_t* out_offsets,
                              size_t count, uint64_t bytes, uint8_t* out, uint32_t* tile_rows, hipStream_t stream);
// out[j] = in[order[j]]
hipError_t launch_gather_words(const uint64_t* in, const uint32_t* order, size_t count, uint64_t* out, hipStream_t stream);

// keyword_pir_api.cpp: he_keyword_pir_table_create_device behind its hashing -- the table of `count` entries whose keyword
// hashes are hashes_device (DEVICE) and whose value offsets are value_offsets (HOST [count + 1]).  Synchronises the stream.
int keyword_pir_table_from_hashes(const he_cuckoo_table_config* config, const uint64_t* hashes_device,
                                  const uint64_t* value_offsets, size_t count, uint64_t seed, he_keyword_pir_table** out_table,
                                  hipStream_t stream);

}  // namespace heamd
