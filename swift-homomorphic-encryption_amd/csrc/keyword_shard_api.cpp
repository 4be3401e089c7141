// keyword_shard_api.cpp -- KeywordDatabase.init(rows:sharding:shardingFunction:) (reference Sources/PrivateInformationRetrieval/
// KeywordPir/KeywordDatabase.swift:406-437): the shard count of a Sharding (:152-268) on the host, the partition of a database
// by shard index on the device, and the object that strings hashing, sharding, the partition and one cuckoo table per shard
// together.  Kernels: keyword_shard_kernels.hip; the table of a shard: keyword_pir_api.cpp.
#include <memory>
#include <string>
#include <vector>

#include "api_internal.hpp"
#include "keyword_pir.hpp"
#include "keyword_shard.hpp"

using heamd::as_stream;
using heamd::invalid_argument;
using heamd::Scratch;

struct he_keyword_database {
    size_t count = 0, shard_count = 0;
    int device = 0;
    // one device block: the partitioned value blob | the partitioned keyword blob
    void* block = nullptr;
    const uint8_t* values = nullptr;
    std::vector<uint32_t> order;                // [count]
    std::vector<uint32_t> shard_starts;         // [shard_count + 1]
    std::vector<uint64_t> shard_value_offsets;  // [shard_count]: where a shard's values start in the partitioned blob
    std::vector<he_keyword_pir_table*> tables;  // [shard_count], NULL for a shard without a row
    ~he_keyword_database() {
        for (he_keyword_pir_table* table : tables) he_keyword_pir_table_destroy(table);
        if (block != nullptr) (void)hipFree(block);
    }
};

namespace {

constexpr size_t kMaxCount = 0xffffffffull;

int invalid_sharding(const std::string& what) {
    heamd::set_last_error("invalid sharding: " + what);
    return HE_ERR_INVALID_SHARDING;
}

}  // namespace

extern "C" int he_keyword_sharding_shard_count(const he_keyword_sharding* sharding, size_t row_count, size_t* out) {
    if (sharding == nullptr || out == nullptr) return invalid_argument("null pointer");
    const uint64_t value = sharding->value;
    if (!sharding->by_entry_count) {  // Sharding.init (:187-198)
        if (value < 1) return invalid_sharding("shardCount " + std::to_string(value) + " must be at least 1");
        if (sharding->has_max_shard_count && value > sharding->max_shard_count)
            return invalid_sharding("shardCount " + std::to_string(value) + " exceeds maxShardCount " +
                                    std::to_string(sharding->max_shard_count));
        if (sharding->require_power_of_two && (value & (value - 1)) != 0)
            return invalid_sharding("shardCount " + std::to_string(value) + " is not a power of two");
        *out = static_cast<size_t>(value);
        return HE_OK;
    }
    if (value < 1) return invalid_sharding("entryCountPerShard " + std::to_string(value) + " must be at least 1");  // (:199-203)
    // the reference resolves this to no shard and would divide by zero in shardIndex
    if (sharding->has_max_shard_count && sharding->max_shard_count == 0) return invalid_sharding("maxShardCount 0 leaves no shard");
    uint64_t count = uint64_t(row_count) / value;  // shardCount(for:) (:256-265): the flooring divide keeps entryCountPerShard
    if (count < 1) count = 1;
    if (sharding->has_max_shard_count && count > sharding->max_shard_count) count = sharding->max_shard_count;
    if (sharding->require_power_of_two)
        while ((count & (count - 1)) != 0) count &= count - 1;  // previousPowerOfTwo
    *out = static_cast<size_t>(count);
    return HE_OK;
}

extern "C" int he_keyword_database_partition_plan(size_t count, size_t shard_count, size_t keyword_bytes, size_t value_bytes,
                                                  uint32_t* out_digit_passes, size_t* out_workgroups_per_pass,
                                                  uint32_t* out_rows_per_workgroup, size_t* out_last_workgroup_rows,
                                                  uint32_t* out_keyword_gather_form, uint32_t* out_value_gather_form) {
    if (shard_count == 0 || shard_count > kMaxCount) return invalid_argument("shard count outside 1 .. 2^32 - 1");
    if (count > kMaxCount - 1) return invalid_argument("more than 2^32 - 2 rows");
    const heamd::PartitionPlan plan = heamd::partition_plan(count, shard_count);
    if (out_digit_passes != nullptr) *out_digit_passes = plan.digit_passes;
    if (out_workgroups_per_pass != nullptr) *out_workgroups_per_pass = plan.workgroups;
    if (out_rows_per_workgroup != nullptr) *out_rows_per_workgroup = heamd::kShardSortTile;
    if (out_last_workgroup_rows != nullptr) *out_last_workgroup_rows = plan.last_rows;
    if (out_keyword_gather_form != nullptr)
        *out_keyword_gather_form = count != 0 && keyword_bytes != 0 ? HE_KEYWORD_GATHER_CHUNK : HE_KEYWORD_GATHER_NONE;
    if (out_value_gather_form != nullptr)
        *out_value_gather_form = count != 0 && value_bytes != 0 ? HE_KEYWORD_GATHER_CHUNK : HE_KEYWORD_GATHER_NONE;
    return HE_OK;
}

extern "C" int he_keyword_database_partition_device(const uint8_t* keywords, const uint64_t* keyword_offsets,
                                                    size_t keyword_bytes, const uint8_t* values,
                                                    const uint64_t* value_offsets, size_t value_bytes, size_t count,
                                                    const uint32_t* shard_indices, size_t shard_count, uint8_t* out_keywords,
                                                    uint64_t* out_keyword_offsets, uint8_t* out_values,
                                                    uint64_t* out_value_offsets, uint32_t* out_order,
                                                    uint32_t* out_shard_starts, uint32_t* device_mismatch, he_stream s) {
    if (shard_count == 0 || shard_count > kMaxCount) return invalid_argument("shard count outside 1 .. 2^32 - 1");
    if (count > kMaxCount - 1) return invalid_argument("more than 2^32 - 2 rows");
    if (out_keyword_offsets == nullptr || out_value_offsets == nullptr || out_shard_starts == nullptr)
        return invalid_argument("null output");
    hipStream_t stream = as_stream(s);
    if (count == 0) {  // no row: every shard is empty
        HEAMD_HIP_TRY(hipMemsetAsync(out_keyword_offsets, 0, sizeof(uint64_t), stream));
        HEAMD_HIP_TRY(hipMemsetAsync(out_value_offsets, 0, sizeof(uint64_t), stream));
        HEAMD_HIP_TRY(hipMemsetAsync(out_shard_starts, 0, (shard_count + 1) * sizeof(uint32_t), stream));
        return HE_OK;
    }
    if (keyword_offsets == nullptr || value_offsets == nullptr || shard_indices == nullptr || out_order == nullptr)
        return invalid_argument("null pointer");
    if ((keyword_bytes != 0 && (keywords == nullptr || out_keywords == nullptr)) ||
        (value_bytes != 0 && (values == nullptr || out_values == nullptr)))
        return invalid_argument("null blob");

    const heamd::PartitionPlan plan = heamd::partition_plan(count, shard_count);
    const size_t bins = 256 * plan.workgroups;
    Scratch alternate(stream), counts(stream), sums(stream), tile_rows(stream);
    if (plan.digit_passes >= 2) HEAMD_HIP_TRY(alternate.allocate(count * sizeof(uint32_t)));
    if (plan.digit_passes >= 1)
        HEAMD_HIP_TRY(counts.allocate((bins + heamd::scan_scratch_elements(bins)) * sizeof(uint32_t)));
    HEAMD_HIP_TRY(sums.allocate(heamd::scan_scratch_elements(count + 1) * sizeof(uint64_t)));
    HEAMD_HIP_TRY(tile_rows.allocate(heamd::gather_scratch_elements(keyword_bytes > value_bytes ? keyword_bytes : value_bytes) *
                                     sizeof(uint32_t)));
    HEAMD_HIP_TRY(heamd::launch_shard_order(shard_indices, count, shard_count, plan, out_order,
                                            static_cast<uint32_t*>(alternate.get()), static_cast<uint32_t*>(counts.get()), stream));
    HEAMD_HIP_TRY(heamd::launch_shard_starts(shard_indices, out_order, count, shard_count, out_shard_starts, stream));
    struct Blob {
        const uint8_t* in;
        const uint64_t* offsets;
        size_t bytes;
        uint8_t* out;
        uint64_t* out_offsets;
    };
    const Blob blobs[2] = {{keywords, keyword_offsets, keyword_bytes, out_keywords, out_keyword_offsets},
                           {values, value_offsets, value_bytes, out_values, out_value_offsets}};
    for (const Blob& blob : blobs) {
        HEAMD_HIP_TRY(heamd::launch_row_lengths(blob.offsets, out_order, count, blob.bytes, shard_indices, shard_count,
                                                blob.out_offsets, device_mismatch, stream));
        HEAMD_HIP_TRY(heamd::launch_exclusive_scan(blob.out_offsets, count + 1, static_cast<uint64_t*>(sums.get()), stream));
        HEAMD_HIP_TRY(heamd::launch_blob_gather(blob.in, blob.offsets, out_order, blob.out_offsets, count, blob.bytes, blob.out,
                                                static_cast<uint32_t*>(tile_rows.get()), stream));
    }
    return HE_OK;
}

extern "C" int he_keyword_database_create_device(const he_cuckoo_table_config* config, const uint8_t* keywords,
                                                 const uint64_t* keyword_offsets, const uint8_t* values,
                                                 const uint64_t* value_offsets, size_t count, size_t shard_count,
                                                 uint64_t other_shard_count, uint64_t seed,
                                                 he_keyword_database** out, he_stream s) {
    const int valid = he_keyword_pir_config_validate(config);
    if (valid != HE_OK) return valid;
    if (out == nullptr) return invalid_argument("null database");
    *out = nullptr;
    if (shard_count == 0 || shard_count > kMaxCount) return invalid_argument("shard count outside 1 .. 2^32 - 1");
    if (keyword_offsets == nullptr || value_offsets == nullptr) return invalid_argument("null offsets");
    if (count > kMaxCount - 1) return invalid_argument("more than 2^32 - 2 entries");
    if (config->hash_function_count > heamd::kKeywordPirMaxHashFunctions) {
        heamd::set_last_error("more than 8 hash functions are not supported");
        return HE_ERR_UNSUPPORTED;
    }
    for (size_t i = 0; i < count; ++i) {
        if (keyword_offsets[i + 1] < keyword_offsets[i] || value_offsets[i + 1] < value_offsets[i])
            return invalid_argument("offsets decrease");
        if (value_offsets[i + 1] - value_offsets[i] > 0xffff) {
            heamd::set_last_error("Invalid hash bucket entry value size: maximum 65535");
            return HE_ERR_INVALID_HASH_BUCKET_ENTRY_VALUE_SIZE;
        }
    }
    const size_t keyword_bytes = keyword_offsets[count] - keyword_offsets[0], value_bytes = value_offsets[count] - value_offsets[0];
    if ((keyword_bytes != 0 && keywords == nullptr) || (value_bytes != 0 && values == nullptr)) return invalid_argument("null blob");

    hipStream_t stream = as_stream(s);
    std::unique_ptr<he_keyword_database> database(new he_keyword_database);
    database->count = count;
    database->shard_count = shard_count;
    database->order.resize(count);
    database->shard_starts.assign(shard_count + 1, 0);
    database->shard_value_offsets.assign(shard_count, 0);
    database->tables.assign(shard_count, nullptr);
    HEAMD_HIP_TRY(hipGetDevice(&database->device));
    if (count == 0) {
        *out = database.release();
        return HE_OK;
    }
    const size_t value_room = (value_bytes + 7) / 8 * 8;  // the keyword blob behind it starts at a multiple of 8
    HEAMD_HIP_TRY(hipMalloc(&database->block, value_room + keyword_bytes + 8));
    uint8_t* out_values = static_cast<uint8_t*>(database->block);
    uint8_t* out_keywords = out_values + value_room;
    database->values = out_values;

    const size_t offset_bytes = (count + 1) * sizeof(uint64_t);
    Scratch offsets_mem(stream), out_offsets_mem(stream), hashes_mem(stream), sorted_mem(stream), indices_mem(stream),
        order_mem(stream), starts_mem(stream);
    HEAMD_HIP_TRY(offsets_mem.allocate(2 * offset_bytes));
    HEAMD_HIP_TRY(out_offsets_mem.allocate(2 * offset_bytes));
    HEAMD_HIP_TRY(hashes_mem.allocate(count * sizeof(uint64_t)));
    HEAMD_HIP_TRY(sorted_mem.allocate(count * sizeof(uint64_t)));
    HEAMD_HIP_TRY(indices_mem.allocate(count * sizeof(uint32_t)));
    HEAMD_HIP_TRY(order_mem.allocate(count * sizeof(uint32_t)));
    HEAMD_HIP_TRY(starts_mem.allocate((shard_count + 1) * sizeof(uint32_t)));
    uint64_t* keyword_offsets_device = static_cast<uint64_t*>(offsets_mem.get());
    uint64_t* value_offsets_device = keyword_offsets_device + count + 1;
    uint64_t* out_keyword_offsets = static_cast<uint64_t*>(out_offsets_mem.get());
    uint64_t* out_value_offsets = out_keyword_offsets + count + 1;
    uint64_t* hashes = static_cast<uint64_t*>(hashes_mem.get());
    uint64_t* sorted_hashes = static_cast<uint64_t*>(sorted_mem.get());
    uint32_t* indices = static_cast<uint32_t*>(indices_mem.get());
    uint32_t* order = static_cast<uint32_t*>(order_mem.get());
    uint32_t* starts = static_cast<uint32_t*>(starts_mem.get());
    HEAMD_HIP_TRY(hipMemcpyAsync(keyword_offsets_device, keyword_offsets, offset_bytes, hipMemcpyHostToDevice, stream));
    HEAMD_HIP_TRY(hipMemcpyAsync(value_offsets_device, value_offsets, offset_bytes, hipMemcpyHostToDevice, stream));
    HEAMD_HIP_TRY(heamd::launch_keyword_hash(keywords, keyword_offsets_device, count, hashes, stream));
    HEAMD_HIP_TRY(heamd::launch_keyword_shard_indices(hashes, count, shard_count, other_shard_count, indices, stream));
    const int partitioned = he_keyword_database_partition_device(
        keywords, keyword_offsets_device, keyword_bytes, values, value_offsets_device, value_bytes, count, indices, shard_count,
        out_keywords, out_keyword_offsets, out_values, out_value_offsets, order, starts, nullptr, s);
    if (partitioned != HE_OK) return partitioned;
    HEAMD_HIP_TRY(heamd::launch_gather_words(hashes, order, count, sorted_hashes, stream));  // hashed once, not again
    HEAMD_HIP_TRY(hipMemcpyAsync(database->order.data(), order, count * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HEAMD_HIP_TRY(hipMemcpyAsync(database->shard_starts.data(), starts, (shard_count + 1) * sizeof(uint32_t),
                                 hipMemcpyDeviceToHost, stream));
    HEAMD_HIP_TRY(hipStreamSynchronize(stream));  // also: the offsets are borrowed pageable host buffers

    // the value offsets of the partitioned blob, restated on the host from the order (4 bytes per row came back)
    std::vector<uint64_t> sorted_offsets(count + 1, 0), shard_offsets;
    for (size_t j = 0; j < count; ++j) {
        const size_t row = database->order[j];
        if (row >= count) return invalid_argument("the partition returned a row that does not exist");
        sorted_offsets[j + 1] = sorted_offsets[j] + (value_offsets[row + 1] - value_offsets[row]);
    }
    for (size_t shard = 0; shard < shard_count; ++shard) {
        const size_t first = database->shard_starts[shard], end = database->shard_starts[shard + 1];
        if (first > end || end > count) return invalid_argument("the partition returned shard starts out of order");
        database->shard_value_offsets[shard] = sorted_offsets[first];
        if (first == end) continue;  // no KeywordDatabaseShard for a shard without a row (:423)
        shard_offsets.resize(end - first + 1);
        for (size_t j = first; j <= end; ++j) shard_offsets[j - first] = sorted_offsets[j] - sorted_offsets[first];
        const int built = heamd::keyword_pir_table_from_hashes(config, sorted_hashes + first, shard_offsets.data(), end - first,
                                                               seed + shard, &database->tables[shard], stream);
        if (built != HE_OK) return built;
    }
    *out = database.release();
    return HE_OK;
}

extern "C" void he_keyword_database_destroy(he_keyword_database* database) {
    if (database == nullptr) return;
    heamd::RelaxedCapture relaxed;
    delete database;
}

extern "C" size_t he_keyword_database_shard_count(const he_keyword_database* database) {
    return database ? database->shard_count : 0;
}
extern "C" size_t he_keyword_database_shard_row_count(const he_keyword_database* database, size_t shard) {
    if (database == nullptr || shard >= database->shard_count) return 0;
    return database->shard_starts[shard + 1] - database->shard_starts[shard];
}
extern "C" const he_keyword_pir_table* he_keyword_database_shard_table(
    const he_keyword_database* database, size_t shard) {
    return database != nullptr && shard < database->shard_count ? database->tables[shard] : nullptr;
}
extern "C" const uint8_t* he_keyword_database_shard_values(const he_keyword_database* database,
                                                                        size_t shard) {
    if (database == nullptr || shard >= database->shard_count || database->values == nullptr) return nullptr;
    return database->values + database->shard_value_offsets[shard];
}
extern "C" int he_keyword_database_order(const he_keyword_database* database, uint32_t* out_host) {
    if (database == nullptr) return invalid_argument("null sharded database");
    if (database->count != 0 && out_host == nullptr) return invalid_argument("null output");
    for (size_t j = 0; j < database->count; ++j) out_host[j] = database->order[j];
    return HE_OK;
}
