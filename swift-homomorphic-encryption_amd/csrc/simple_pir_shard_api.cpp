// simple_pir_shard_api.cpp -- SimplePIR over sharded databases behind the C ABI: DatabaseMap.shardDatabase (reference Sources/
// PrivateInformationRetrieval/SimplePir/DatabaseMap.swift:82-110) as a plan on the host, a map and a scatter on the device, and
// SimplePirClientForAllShards' index lists and assembly (SimplePir+Shards.swift:71-99, :139-171).  Kernels:
// simple_pir_shard_kernels.hip; the form choice and the tile arithmetic: simple_pir_shard_plan.hpp.  The per-shard orders are an
// input (the reference shuffles with the system generator; this library generates no randomness).  The map's scratch comes from
// the stream-ordered cache and depends on the database alone; the two client entries take no scratch at all.
#include <string>

#include "api_internal.hpp"
#include "simple_pir_shard.hpp"
#include "word_layer.hpp"

using heamd::as_stream;
using heamd::invalid_argument;
using heamd::Scratch;
using heamd::SimplePirShardMapView;
namespace shard = heamd::simple_pir_shard;

static_assert(HE_SIMPLE_PIR_SHARD_FORM_NONE == uint32_t(shard::Form::kNone) && HE_SIMPLE_PIR_SHARD_FORM_BYTE == uint32_t(shard::Form::kByte) &&
                  HE_SIMPLE_PIR_SHARD_FORM_WORD == uint32_t(shard::Form::kWord) && HE_SIMPLE_PIR_SHARD_FORM_WIDE == uint32_t(shard::Form::kWide),
              "include/he_amd.h names the forms of simple_pir_shard_plan.hpp");

extern "C++" {
namespace {

int check_shape(size_t count, size_t shard_count, size_t chunk_size, uint64_t total_chunks) {
    if (shard_count == 0 || shard_count > shard::kMaxShardCount) return invalid_argument("shard count outside 1 .. 256");
    if (chunk_size == 0) return invalid_argument("chunk size 0");
    if (count > shard::kMaxCount) return invalid_argument("more than 2^32 - 2 entries");
    if (total_chunks > shard::kMaxChunks) return invalid_argument("more than 2^32 - 1 chunks");
    return HE_OK;
}

bool aligned(const void* pointer, size_t to) { return (reinterpret_cast<uintptr_t>(pointer) & (to - 1)) == 0; }

}  // namespace
}  // extern "C++"

int he_simple_pir_shard_plan(const uint64_t* value_offsets, size_t count, size_t shard_count, size_t chunk_size,
                             uint64_t shards_address, uint64_t* out_total_chunks, uint64_t* out_maximum_chunk_count,
                             uint64_t* out_chunks_per_shard, uint32_t* out_scatter_form, uint32_t* out_map_tile_entries,
                             size_t* out_map_tiles, size_t* out_count_workgroups, size_t* out_scratch_bytes) {
    if (count != 0 && count <= shard::kMaxCount && value_offsets == nullptr) return invalid_argument("null offsets");
    shard::Plan plan;
    switch (shard::plan(value_offsets, count, shard_count, chunk_size, plan)) {
        case shard::PlanError::kNone:
            break;
        case shard::PlanError::kShardCount:
            return invalid_argument("shard count outside 1 .. 256");
        case shard::PlanError::kChunkSize:
            return invalid_argument("chunk size 0");
        case shard::PlanError::kCount:
            return invalid_argument("more than 2^32 - 2 entries");
        case shard::PlanError::kOffsets:
            return invalid_argument("offsets decrease");
        case shard::PlanError::kChunks:
            return invalid_argument("more than 2^32 - 1 chunks");
    }
    if (out_total_chunks != nullptr) *out_total_chunks = plan.total_chunks;
    if (out_maximum_chunk_count != nullptr) *out_maximum_chunk_count = plan.maximum_chunk_count;
    if (out_chunks_per_shard != nullptr) *out_chunks_per_shard = plan.chunks_per_shard;
    if (out_scatter_form != nullptr)
        *out_scatter_form = uint32_t(shard::form(static_cast<uintptr_t>(shards_address), 0, chunk_size, plan.total_chunks * chunk_size));
    if (out_map_tile_entries != nullptr) *out_map_tile_entries = shard::kMapTile;
    if (out_map_tiles != nullptr) *out_map_tiles = plan.map_tiles;
    if (out_count_workgroups != nullptr) *out_count_workgroups = plan.count_workgroups;
    if (out_scratch_bytes != nullptr) *out_scratch_bytes = plan.scratch_bytes();
    return HE_OK;
}

int he_simple_pir_shard_map_device(const uint64_t* value_offsets, const uint8_t* shard_orders, size_t count, size_t shard_count,
                                   size_t chunk_size, uint64_t total_chunks, uint64_t* out_chunk_starts, uint32_t* out_chunk_shard,
                                   uint32_t* out_chunk_index, uint64_t* out_shard_row_starts, uint32_t* out_row_chunk,
                                   uint32_t* device_mismatch, he_stream s) {
    HEAMD_TRY_STATUS(check_shape(count, shard_count, chunk_size, total_chunks));
    if (value_offsets == nullptr || out_chunk_starts == nullptr || out_shard_row_starts == nullptr)
        return invalid_argument("null offsets, chunk starts or shard row starts");
    if (count != 0 && shard_orders == nullptr) return invalid_argument("null shard orders");
    if (total_chunks != 0 && (out_chunk_shard == nullptr || out_chunk_index == nullptr || out_row_chunk == nullptr))
        return invalid_argument("null chunk arrays");
    if (!aligned(value_offsets, 8) || !aligned(out_chunk_starts, 8) || !aligned(out_shard_row_starts, 8) ||
        !aligned(out_chunk_shard, 4) || !aligned(out_chunk_index, 4) || !aligned(out_row_chunk, 4) || !aligned(device_mismatch, 4))
        return invalid_argument("misaligned array");
    const size_t chunk_bytes = static_cast<size_t>(total_chunks) * sizeof(uint32_t);
    HEAMD_TRY_STATUS(heamd::check_slabs("shardDatabase", {{"out_chunk_starts", out_chunk_starts, (count + 1) * sizeof(uint64_t), true},
                                                          {"out_chunk_shard", out_chunk_shard, chunk_bytes, true},
                                                          {"out_chunk_index", out_chunk_index, chunk_bytes, true},
                                                          {"out_shard_row_starts", out_shard_row_starts,
                                                           (shard_count + 1) * sizeof(uint64_t), true},
                                                          {"out_row_chunk", out_row_chunk, chunk_bytes, true},
                                                          {"device_mismatch", device_mismatch, sizeof(uint32_t), true},
                                                          {"value_offsets", value_offsets, (count + 1) * sizeof(uint64_t), false},
                                                          {"shard_orders", shard_orders, count * shard_count, false}}));
    hipStream_t stream = as_stream(s);
    shard::Plan plan;
    shard::map_shape(count, shard_count, plan);
    Scratch sums(stream), scan(stream);
    HEAMD_HIP_TRY(sums.allocate(plan.sum_elements * sizeof(uint32_t)));
    HEAMD_HIP_TRY(scan.allocate(plan.scan_elements * sizeof(uint64_t)));
    HEAMD_HIP_TRY(heamd::launch_simple_pir_shard_map(value_offsets, shard_orders, count, shard_count, chunk_size, total_chunks, plan,
                                                     out_chunk_starts, out_chunk_shard, out_chunk_index, out_shard_row_starts,
                                                     out_row_chunk, device_mismatch, static_cast<uint32_t*>(sums.get()),
                                                     static_cast<uint64_t*>(scan.get()), stream));
    return HE_OK;
}

int he_simple_pir_shard_scatter_device(const uint8_t* values, uint64_t values_bytes, const uint64_t* value_offsets, size_t count,
                                       size_t chunk_size, uint64_t total_chunks, const uint64_t* chunk_starts,
                                       const uint32_t* row_chunk, uint8_t* shards, he_stream s) {
    HEAMD_TRY_STATUS(check_shape(count, 1, chunk_size, total_chunks));
    if (total_chunks == 0) return HE_OK;
    if (value_offsets == nullptr || chunk_starts == nullptr || row_chunk == nullptr || shards == nullptr)
        return invalid_argument("null offsets, map or shards");
    if (values_bytes != 0 && values == nullptr) return invalid_argument("null values");
    if (!aligned(value_offsets, 8) || !aligned(chunk_starts, 8) || !aligned(row_chunk, 4)) return invalid_argument("misaligned array");
    if (total_chunks > SIZE_MAX / chunk_size) return invalid_argument("the shards exceed the address space");
    const size_t slab_bytes = static_cast<size_t>(total_chunks) * chunk_size;
    HEAMD_TRY_STATUS(heamd::check_slabs("shardDatabase", {{"shards", shards, slab_bytes, true},
                                                          {"values", values, static_cast<size_t>(values_bytes), false},
                                                          {"value_offsets", value_offsets, (count + 1) * sizeof(uint64_t), false},
                                                          {"chunk_starts", chunk_starts, (count + 1) * sizeof(uint64_t), false},
                                                          {"row_chunk", row_chunk, total_chunks * sizeof(uint32_t), false}}));
    const SimplePirShardMapView map{chunk_starts, nullptr, nullptr, nullptr, row_chunk, count, 1, chunk_size, total_chunks};
    const shard::Form form = shard::form(reinterpret_cast<uintptr_t>(shards), 0, chunk_size, slab_bytes);
    HEAMD_HIP_TRY(heamd::launch_simple_pir_shard_scatter(values, values_bytes, value_offsets, map, form, shards, as_stream(s)));
    return HE_OK;
}

int he_simple_pir_shard_query_indices_device(const uint64_t* entry_positions, size_t batch, size_t count, size_t shard_count,
                                             uint64_t total_chunks, uint64_t maximum_chunk_count, uint64_t chunks_per_shard,
                                             const uint64_t* chunk_starts, const uint32_t* chunk_shard, const uint32_t* chunk_index,
                                             uint64_t* out_indices, uint32_t* out_found, he_stream s) {
    HEAMD_TRY_STATUS(check_shape(count, shard_count, 1, total_chunks));
    if (maximum_chunk_count > total_chunks) return invalid_argument("maximum chunk count above the chunk count");
    if (maximum_chunk_count != 0 && chunks_per_shard == 0) return invalid_argument("no query slot for an entry with chunks");
    if (chunks_per_shard > shard::kMaxChunks || batch > shard::kMaxChunks) return invalid_argument("too many queries for one call");
    if (batch == 0) return HE_OK;
    if (entry_positions == nullptr || out_found == nullptr || chunk_starts == nullptr) return invalid_argument("null positions, map or flags");
    if (chunks_per_shard != 0 && out_indices == nullptr) return invalid_argument("null indices");
    if (total_chunks != 0 && (chunk_shard == nullptr || chunk_index == nullptr)) return invalid_argument("null chunk arrays");
    if (!aligned(entry_positions, 8) || !aligned(chunk_starts, 8) || !aligned(out_indices, 8) || !aligned(chunk_shard, 4) ||
        !aligned(chunk_index, 4) || !aligned(out_found, 4))
        return invalid_argument("misaligned array");
    const size_t index_bytes = shard_count * batch * static_cast<size_t>(chunks_per_shard) * sizeof(uint64_t);
    HEAMD_TRY_STATUS(heamd::check_slabs("query(for:)", {{"out_indices", out_indices, index_bytes, true},
                                                        {"out_found", out_found, batch * sizeof(uint32_t), true},
                                                        {"entry_positions", entry_positions, batch * sizeof(uint64_t), false},
                                                        {"chunk_starts", chunk_starts, (count + 1) * sizeof(uint64_t), false},
                                                        {"chunk_shard", chunk_shard, total_chunks * sizeof(uint32_t), false},
                                                        {"chunk_index", chunk_index, total_chunks * sizeof(uint32_t), false}}));
    const SimplePirShardMapView map{chunk_starts, chunk_shard, chunk_index, nullptr, nullptr, count, shard_count, 1, total_chunks};
    HEAMD_HIP_TRY(heamd::launch_simple_pir_shard_query_indices(entry_positions, batch, map, maximum_chunk_count, chunks_per_shard,
                                                               out_indices, out_found, as_stream(s)));
    return HE_OK;
}

int he_simple_pir_shard_assemble_device(const uint8_t* chunks, const uint64_t* indices, const uint64_t* entry_positions, size_t batch,
                                        const uint64_t* value_offsets, size_t count, size_t shard_count, size_t chunk_size,
                                        uint64_t total_chunks, uint64_t maximum_chunk_count, uint64_t chunks_per_shard,
                                        const uint64_t* chunk_starts, const uint32_t* chunk_shard, const uint32_t* chunk_index,
                                        uint8_t* out_entries, uint64_t* out_sizes, uint32_t* out_found, he_stream s) {
    HEAMD_TRY_STATUS(check_shape(count, shard_count, chunk_size, total_chunks));
    if (maximum_chunk_count > total_chunks) return invalid_argument("maximum chunk count above the chunk count");
    if (maximum_chunk_count != 0 && chunks_per_shard == 0) return invalid_argument("no query slot for an entry with chunks");
    if (chunks_per_shard > shard::kMaxChunks || batch > shard::kMaxChunks) return invalid_argument("too many queries for one call");
    if (batch == 0) return HE_OK;
    if (entry_positions == nullptr || value_offsets == nullptr || chunk_starts == nullptr || out_sizes == nullptr || out_found == nullptr)
        return invalid_argument("null positions, offsets, map, sizes or flags");
    if (maximum_chunk_count != 0 && (chunks == nullptr || indices == nullptr || out_entries == nullptr))
        return invalid_argument("null chunks, indices or entries");
    if (total_chunks != 0 && (chunk_shard == nullptr || chunk_index == nullptr)) return invalid_argument("null chunk arrays");
    if (!aligned(indices, 8) || !aligned(entry_positions, 8) || !aligned(value_offsets, 8) || !aligned(chunk_starts, 8) ||
        !aligned(out_sizes, 8) || !aligned(chunk_shard, 4) || !aligned(chunk_index, 4) || !aligned(out_found, 4))
        return invalid_argument("misaligned array");
    if (maximum_chunk_count > SIZE_MAX / chunk_size / batch) return invalid_argument("the entries exceed the address space");
    const size_t slots = shard_count * batch * static_cast<size_t>(chunks_per_shard);
    const size_t entry_bytes = batch * static_cast<size_t>(maximum_chunk_count) * chunk_size;
    HEAMD_TRY_STATUS(heamd::check_slabs("decrypt(responses:for:with:)",
                                        {{"out_entries", out_entries, entry_bytes, true},
                                         {"out_sizes", out_sizes, batch * sizeof(uint64_t), true},
                                         {"out_found", out_found, batch * sizeof(uint32_t), true},
                                         {"chunks", chunks, slots * chunk_size, false},
                                         {"indices", indices, slots * sizeof(uint64_t), false},
                                         {"entry_positions", entry_positions, batch * sizeof(uint64_t), false},
                                         {"value_offsets", value_offsets, (count + 1) * sizeof(uint64_t), false},
                                         {"chunk_starts", chunk_starts, (count + 1) * sizeof(uint64_t), false},
                                         {"chunk_shard", chunk_shard, total_chunks * sizeof(uint32_t), false},
                                         {"chunk_index", chunk_index, total_chunks * sizeof(uint32_t), false}}));
    const SimplePirShardMapView map{chunk_starts, chunk_shard, chunk_index, nullptr, nullptr, count, shard_count, chunk_size, total_chunks};
    const shard::Form form = shard::form(reinterpret_cast<uintptr_t>(out_entries), reinterpret_cast<uintptr_t>(chunks), chunk_size, entry_bytes);
    HEAMD_HIP_TRY(heamd::launch_simple_pir_shard_assemble(chunks, indices, entry_positions, batch, value_offsets, map,
                                                          maximum_chunk_count, chunks_per_shard, form, out_entries, out_sizes,
                                                          out_found, as_stream(s)));
    return HE_OK;
}
