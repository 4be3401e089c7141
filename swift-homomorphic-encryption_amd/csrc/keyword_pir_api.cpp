// keyword_pir_api.cpp -- the device entries of the keyword-PIR database build and the table object that strings them
// together: CuckooTable.init (reference Sources/PrivateInformationRetrieval/KeywordPir/CuckooTable.swift:328-357) and the body
// of KeywordPirServer.process (KeywordPirProtocol.swift:191-247).  Kernels: keyword_pir_kernels.hip; placement: keyword_pir.cpp.
#include <string>
#include <vector>

#include "api_internal.hpp"
#include "bfv_context.hpp"
#include "keyword_pir.hpp"
#include "keyword_shard.hpp"

using heamd::as_stream;
using heamd::invalid_argument;
using heamd::Scratch;

struct he_keyword_pir_table {
    he_cuckoo_table_config config{};
    size_t count = 0, bucket_count = 0, table_count = 1, largest = 0, placed = 0, duplicates = 0, expansions = 0;
    float load_factor = 0;
    int device = 0;
    // one device block: hashes [count] | value_offsets [count + 1] | bucket_offsets [bucket_count + 1] | slot_entries [placed]
    void* block = nullptr;
    const uint64_t* hashes = nullptr;
    const uint64_t* value_offsets = nullptr;
    const uint32_t* bucket_offsets = nullptr;
    const uint32_t* slot_entries = nullptr;
    ~he_keyword_pir_table() {
        if (block != nullptr) (void)hipFree(block);
    }
};

namespace {

constexpr size_t kMaxCount = 0xffffffffull;

int serialize_buckets(const heamd::HashBucketTable& table, size_t slot_count, uint8_t* out, uint32_t* mismatch,
                      hipStream_t stream) {
    if (table.bucket_count == 0 || table.entry_size == 0) return HE_OK;
    Scratch starts(stream);
    HEAMD_HIP_TRY(starts.allocate(slot_count * sizeof(uint32_t)));
    uint32_t* slot_starts = static_cast<uint32_t*>(starts.get());
    HEAMD_HIP_TRY(heamd::launch_hash_bucket_slot_starts(table, slot_starts, mismatch, stream));
    HEAMD_HIP_TRY(heamd::launch_hash_bucket_serialize(table, slot_starts, out, stream));
    return HE_OK;
}

int table_on_device(const he_keyword_pir_table* table) {
    if (table == nullptr) return invalid_argument("null keyword PIR table");
    int device = 0;
    HEAMD_HIP_TRY(hipGetDevice(&device));
    if (device != table->device) {
        heamd::set_last_error("the keyword PIR table lives on HIP device " + std::to_string(table->device) + " but device " +
                              std::to_string(device) + " is current");
        return HE_ERR_DEVICE;
    }
    return HE_OK;
}

heamd::HashBucketTable bucket_table(const he_keyword_pir_table* table, const uint8_t* values, size_t entry_size) {
    heamd::HashBucketTable t;
    t.hashes = table->hashes;
    t.values = values;
    t.value_offsets = table->value_offsets;
    t.bucket_offsets = table->bucket_offsets;
    t.slot_entries = table->slot_entries;
    t.bucket_count = table->bucket_count;
    t.entry_size = entry_size;
    return t;
}

int check_entry_size(const he_keyword_pir_table* table, size_t entry_size_in_bytes) {
    if (entry_size_in_bytes < table->largest) {
        heamd::set_last_error("invalid argument: entry size " + std::to_string(entry_size_in_bytes) +
                              " is below the largest serialized bucket, " + std::to_string(table->largest) + " bytes");
        return HE_ERR_INVALID_ARGUMENT;
    }
    if (entry_size_in_bytes > (uint64_t(1) << 48)) return invalid_argument("entry size too large");
    return HE_OK;
}

int process_sub_table(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count, const uint8_t* entries,
                      size_t entry_count, size_t entry_size, uint64_t* database, uint8_t* present, he_stream s) {
    return he_pir_process_database_device(ctx, dimensions, dimension_count, entries, nullptr, entry_count, entry_size, 0,
                                          database, present, s);
}
int process_sub_table(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count, const uint8_t* entries,
                      size_t entry_count, size_t entry_size, uint32_t* database, uint8_t* present, he_stream s) {
    return he_pir_process_database_device_u32(ctx, dimensions, dimension_count, entries, nullptr, entry_count, entry_size, 0,
                                              database, present, s);
}

template <typename W>
int process_database(const he_bfv_context* ctx, const he_keyword_pir_table* table, const uint8_t* values,
                     const uint32_t* dimensions, uint32_t dimension_count, size_t entry_size, size_t chunk_count,
                     size_t per_chunk, W* database, uint8_t* present, he_stream s) {
    hipStream_t stream = as_stream(s);
    const size_t per_table = table->bucket_count / table->table_count;
    Scratch entries_mem(stream);
    HEAMD_HIP_TRY(entries_mem.allocate(table->bucket_count * entry_size));
    uint8_t* entries = static_cast<uint8_t*>(entries_mem.get());
    const int serialized = serialize_buckets(bucket_table(table, values, entry_size), table->placed, entries, nullptr, stream);
    if (serialized != HE_OK) return serialized;
    const size_t slots = chunk_count * per_chunk;
    const size_t words = slots * he_bfv_ciphertext_moduli_count(ctx) * heamd::bfv_impl(ctx).degree();
    for (size_t t = 0; t < table->table_count; ++t) {
        const int status = process_sub_table(ctx, dimensions, dimension_count, entries + t * per_table * entry_size, per_table,
                                             entry_size, database + t * words, present + t * slots, s);
        if (status != HE_OK) return status;
    }
    return HE_OK;
}

}  // namespace

extern "C" int he_keyword_pir_hash_keywords_device(const uint8_t* keywords, const uint64_t* keyword_offsets, size_t count,
                                                   uint64_t* out_hashes, he_stream s) {
    if (count == 0) return HE_OK;
    if (keyword_offsets == nullptr || out_hashes == nullptr) return invalid_argument("null pointer");
    if (count > kMaxCount) return invalid_argument("more than 2^32 - 1 keywords");
    HEAMD_HIP_TRY(heamd::launch_keyword_hash(keywords, keyword_offsets, count, out_hashes, as_stream(s)));
    return HE_OK;
}

extern "C" int he_keyword_pir_hash_indices_device(const uint64_t* hashes, size_t count, uint64_t bucket_count,
                                                  uint32_t hash_function_count, uint32_t* out_indices, he_stream s) {
    if (bucket_count == 0 || bucket_count > kMaxCount) return invalid_argument("bucket count outside 1 .. 2^32 - 1");
    if (hash_function_count == 0) return invalid_argument("no hash function");
    if (hash_function_count > heamd::kKeywordPirMaxHashFunctions) {
        heamd::set_last_error("more than 8 hash functions are not supported");
        return HE_ERR_UNSUPPORTED;
    }
    if (count == 0) return HE_OK;
    if (hashes == nullptr || out_indices == nullptr) return invalid_argument("null pointer");
    if (count > kMaxCount) return invalid_argument("more than 2^32 - 1 keywords");
    HEAMD_HIP_TRY(heamd::launch_keyword_hash_indices(hashes, count, bucket_count, hash_function_count, out_indices, as_stream(s)));
    return HE_OK;
}

extern "C" int he_keyword_pir_shard_indices_device(const uint64_t* hashes, size_t count, uint64_t shard_count,
                                                   uint64_t other_shard_count, uint32_t* out, he_stream s) {
    if (shard_count == 0 || shard_count > kMaxCount) return invalid_argument("shard count outside 1 .. 2^32 - 1");
    if (count == 0) return HE_OK;
    if (hashes == nullptr || out == nullptr) return invalid_argument("null pointer");
    if (count > kMaxCount) return invalid_argument("more than 2^32 - 1 keywords");
    HEAMD_HIP_TRY(heamd::launch_keyword_shard_indices(hashes, count, shard_count, other_shard_count, out, as_stream(s)));
    return HE_OK;
}

extern "C" int he_keyword_pir_serialize_buckets_device(const uint64_t* hashes, const uint8_t* values,
                                                       const uint64_t* value_offsets, const uint32_t* bucket_offsets,
                                                       const uint32_t* slot_entries, size_t slot_count, size_t bucket_count,
                                                       size_t entry_size_in_bytes, uint8_t* out, uint32_t* device_mismatch,
                                                       he_stream s) {
    if (bucket_count == 0 || entry_size_in_bytes == 0) return HE_OK;
    if (bucket_offsets == nullptr || out == nullptr) return invalid_argument("null pointer");
    if (slot_count != 0 && (hashes == nullptr || value_offsets == nullptr || slot_entries == nullptr))
        return invalid_argument("null pointer");
    if (bucket_count > kMaxCount || slot_count > kMaxCount) return invalid_argument("more than 2^32 - 1 buckets or slots");
    if (entry_size_in_bytes > (uint64_t(1) << 48)) return invalid_argument("entry size too large");
    heamd::HashBucketTable table;
    table.hashes = hashes;
    table.values = values;
    table.value_offsets = value_offsets;
    table.bucket_offsets = bucket_offsets;
    table.slot_entries = slot_entries;
    table.bucket_count = bucket_count;
    table.entry_size = entry_size_in_bytes;
    return serialize_buckets(table, slot_count, out, device_mismatch, as_stream(s));
}

extern "C" int he_keyword_pir_table_create_device(const he_cuckoo_table_config* config, const uint8_t* keywords,
                                                  const uint64_t* keyword_offsets, const uint8_t* values,
                                                  const uint64_t* value_offsets, size_t count, uint64_t seed,
                                                  he_keyword_pir_table** out_table, he_stream s) {
    (void)values;  // the blob is read by the entries calls; here only its offsets matter
    const int valid = he_keyword_pir_config_validate(config);
    if (valid != HE_OK) return valid;
    if (out_table == nullptr) return invalid_argument("null table");
    *out_table = nullptr;
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
    size_t bucket_count = 0;
    {  // the bucket count's errors return here, before a copy out of the borrowed keyword_offsets is in flight
        std::vector<uint64_t> sizes(count);
        for (size_t i = 0; i < count; ++i) sizes[i] = value_offsets[i + 1] - value_offsets[i];
        const int counted = he_keyword_pir_bucket_count(config, sizes.data(), count, &bucket_count);
        if (counted != HE_OK) return counted;
        if (bucket_count > kMaxCount) return invalid_argument("more than 2^32 - 1 buckets");
    }
    hipStream_t stream = as_stream(s);
    Scratch hashes_mem(stream), offsets_mem(stream);
    HEAMD_HIP_TRY(hashes_mem.allocate(count * sizeof(uint64_t)));
    HEAMD_HIP_TRY(offsets_mem.allocate((count + 1) * sizeof(uint64_t)));
    uint64_t* hashes_device = static_cast<uint64_t*>(hashes_mem.get());
    HEAMD_HIP_TRY(hipMemcpyAsync(offsets_mem.get(), keyword_offsets, (count + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    HEAMD_HIP_TRY(heamd::launch_keyword_hash(keywords, static_cast<const uint64_t*>(offsets_mem.get()), count, hashes_device, stream));
    // (the call below synchronises the stream before it returns: keyword_offsets is a borrowed pageable host buffer)
    return heamd::keyword_pir_table_from_hashes(config, hashes_device, value_offsets, count, seed, out_table, stream);
}

// The table behind its hashing (keyword_shard.hpp): the sharded database builds one per shard from hashes it has gathered.
int heamd::keyword_pir_table_from_hashes(const he_cuckoo_table_config* config, const uint64_t* hashes_device,
                                         const uint64_t* value_offsets, size_t count, uint64_t seed,
                                         he_keyword_pir_table** out_table, hipStream_t stream) {
    std::vector<uint64_t> sizes(count);
    for (size_t i = 0; i < count; ++i) {
        if (value_offsets[i + 1] < value_offsets[i]) return invalid_argument("offsets decrease");
        sizes[i] = value_offsets[i + 1] - value_offsets[i];
        if (sizes[i] > 0xffff) {
            heamd::set_last_error("Invalid hash bucket entry value size: maximum 65535");
            return HE_ERR_INVALID_HASH_BUCKET_ENTRY_VALUE_SIZE;
        }
    }
    size_t bucket_count = 0;
    const int counted = he_keyword_pir_bucket_count(config, sizes.data(), count, &bucket_count);
    if (counted != HE_OK) return counted;
    if (bucket_count > kMaxCount) return invalid_argument("more than 2^32 - 1 buckets");

    const uint32_t h = config->hash_function_count;
    const size_t tables = config->multiple_tables ? h : 1;
    std::vector<uint64_t> hashes(count);
    std::vector<uint32_t> indices(count * h), bucket_offsets, slot_entries(count);
    Scratch indices_mem(stream);
    HEAMD_HIP_TRY(indices_mem.allocate(count * h * sizeof(uint32_t)));
    if (count != 0)
        HEAMD_HIP_TRY(hipMemcpyAsync(hashes.data(), hashes_device, count * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    size_t placed = 0, duplicates = 0, expansions = 0;
    for (;;) {
        HEAMD_HIP_TRY(heamd::launch_keyword_hash_indices(hashes_device, count, bucket_count / tables, h,
                                                         static_cast<uint32_t*>(indices_mem.get()), stream));
        if (count != 0)
            HEAMD_HIP_TRY(hipMemcpyAsync(indices.data(), indices_mem.get(), count * h * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                         stream));
        HEAMD_HIP_TRY(hipStreamSynchronize(stream));  // also: keyword_offsets is a borrowed pageable host buffer
        bucket_offsets.assign(bucket_count + 1, 0);
        size_t next = 0;
        const int status = he_keyword_pir_cuckoo_place(config, hashes.data(), indices.data(), sizes.data(), count, bucket_count,
                                                       seed, bucket_offsets.data(), slot_entries.data(), &placed, &duplicates,
                                                       &next);
        if (status == HE_OK) break;
        if (status != HE_ERR_CUCKOO_TABLE_NEEDS_EXPANSION) return status;
        if (next <= bucket_count || next > kMaxCount) {
            heamd::set_last_error("Expanding Cuckoo table failed");
            return HE_ERR_FAILED_TO_CONSTRUCT_CUCKOO_TABLE;
        }
        bucket_count = next;
        ++expansions;
    }

    std::unique_ptr<he_keyword_pir_table> table(new he_keyword_pir_table);
    table->config = *config;
    table->count = count;
    table->bucket_count = bucket_count;
    table->table_count = tables;
    table->placed = placed;
    table->duplicates = duplicates;
    table->expansions = expansions;
    uint64_t serialized = 0;
    for (size_t b = 0; b < bucket_count; ++b) {
        uint64_t size = 1;
        for (uint32_t slot = bucket_offsets[b]; slot < bucket_offsets[b + 1]; ++slot) size += 10 + sizes[slot_entries[slot]];
        serialized += size;
        if (size > table->largest) table->largest = size;
    }
    // summarize() (:366-367)
    table->load_factor = static_cast<float>(serialized) /
                         static_cast<float>(static_cast<uint64_t>(bucket_count) * config->max_serialized_bucket_size);
    HEAMD_HIP_TRY(hipGetDevice(&table->device));
    const size_t hash_bytes = count * sizeof(uint64_t), offset_bytes = (count + 1) * sizeof(uint64_t);
    const size_t bucket_bytes = (bucket_count + 1) * sizeof(uint32_t), slot_bytes = placed * sizeof(uint32_t);
    HEAMD_HIP_TRY(hipMalloc(&table->block, hash_bytes + offset_bytes + bucket_bytes + slot_bytes));
    char* base = static_cast<char*>(table->block);
    table->hashes = reinterpret_cast<const uint64_t*>(base);
    table->value_offsets = reinterpret_cast<const uint64_t*>(base + hash_bytes);
    table->bucket_offsets = reinterpret_cast<const uint32_t*>(base + hash_bytes + offset_bytes);
    table->slot_entries = reinterpret_cast<const uint32_t*>(base + hash_bytes + offset_bytes + bucket_bytes);
    if (count != 0)
        HEAMD_HIP_TRY(hipMemcpyAsync(base, hashes_device, hash_bytes, hipMemcpyDeviceToDevice, stream));
    HEAMD_HIP_TRY(hipMemcpyAsync(base + hash_bytes, value_offsets, offset_bytes, hipMemcpyHostToDevice, stream));
    HEAMD_HIP_TRY(hipMemcpyAsync(base + hash_bytes + offset_bytes, bucket_offsets.data(), bucket_bytes, hipMemcpyHostToDevice,
                                 stream));
    if (placed != 0)
        HEAMD_HIP_TRY(hipMemcpyAsync(base + hash_bytes + offset_bytes + bucket_bytes, slot_entries.data(), slot_bytes,
                                     hipMemcpyHostToDevice, stream));
    HEAMD_HIP_TRY(hipStreamSynchronize(stream));  // the host buffers above are borrowed or local
    *out_table = table.release();
    return HE_OK;
}

extern "C" void he_keyword_pir_table_destroy(he_keyword_pir_table* table) {
    if (table == nullptr) return;
    heamd::RelaxedCapture relaxed;
    delete table;
}

extern "C" size_t he_keyword_pir_table_bucket_count(const he_keyword_pir_table* table) { return table ? table->bucket_count : 0; }
extern "C" size_t he_keyword_pir_table_buckets_per_table(const he_keyword_pir_table* table) {
    return table ? table->bucket_count / table->table_count : 0;
}
extern "C" size_t he_keyword_pir_table_table_count(const he_keyword_pir_table* table) { return table ? table->table_count : 0; }
extern "C" size_t he_keyword_pir_table_largest_bucket_size(const he_keyword_pir_table* table) { return table ? table->largest : 0; }
extern "C" size_t he_keyword_pir_table_entry_count(const he_keyword_pir_table* table) { return table ? table->placed : 0; }
extern "C" size_t he_keyword_pir_table_duplicates_dropped(const he_keyword_pir_table* table) {
    return table ? table->duplicates : 0;
}
extern "C" size_t he_keyword_pir_table_expansion_count(const he_keyword_pir_table* table) { return table ? table->expansions : 0; }
extern "C" float he_keyword_pir_table_load_factor(const he_keyword_pir_table* table) { return table ? table->load_factor : 0; }

extern "C" int he_keyword_pir_table_entries_device(const he_keyword_pir_table* table, const uint8_t* values,
                                                   size_t entry_size_in_bytes, uint8_t* out, he_stream s) {
    const int usable = table_on_device(table);
    if (usable != HE_OK) return usable;
    const int fits = check_entry_size(table, entry_size_in_bytes);
    if (fits != HE_OK) return fits;
    if (out == nullptr) return invalid_argument("null output");
    return serialize_buckets(bucket_table(table, values, entry_size_in_bytes), table->placed, out, nullptr, as_stream(s));
}

extern "C" int he_keyword_pir_process_database_device(const he_bfv_context* ctx, const he_keyword_pir_table* table,
                                                      const uint8_t* values, const uint32_t* dimensions,
                                                      uint32_t dimension_count, size_t entry_size_in_bytes, void* database,
                                                      uint8_t* present, he_stream s) {
    if (ctx == nullptr) return invalid_argument("null context");
    if (table == nullptr) return invalid_argument("null keyword PIR table");
    const int fits = check_entry_size(table, entry_size_in_bytes);
    if (fits != HE_OK) return fits;
    size_t chunk_count = 0, per_chunk = 0;
    const int planned = he_pir_database_shape(ctx, dimensions, dimension_count, table->bucket_count / table->table_count,
                                              entry_size_in_bytes, 0, &chunk_count, &per_chunk, nullptr, nullptr, nullptr);
    if (planned != HE_OK) return planned;
    if (database == nullptr || present == nullptr) return invalid_argument("null database");
    const int usable = table_on_device(table);
    if (usable != HE_OK) return usable;
    if (heamd::bfv_impl(ctx).word_bits() == 32)
        return process_database(ctx, table, values, dimensions, dimension_count, entry_size_in_bytes, chunk_count, per_chunk,
                                static_cast<uint32_t*>(database), present, s);
    return process_database(ctx, table, values, dimensions, dimension_count, entry_size_in_bytes, chunk_count, per_chunk,
                            static_cast<uint64_t*>(database), present, s);
}
