// keyword_pir.cpp -- the sequential step of KeywordPirServer.process: CuckooTable.insert / insertLoop (reference
// Sources/PrivateInformationRetrieval/KeywordPir/CuckooTable.swift:386-458) over integers only -- per entry its keyword hash, its
// h candidate indices and its value size -- plus CuckooTableConfig.validate() (:138-156) and the initial bucket count
// (:339-349).  Plain C++ with no device: a host compiler builds this file alone.
//
// canInsert (:202-205), swapIndices (:209-217), index(tableIndex:index:) (:461-463), the size guard of insert (:387-396) and
// maxEvictionCount are the reference's.  Three things are not:
//   1. Duplicates go by the 64-bit keyword hash, first one wins.  Equal hashes have the same candidates, so the check has the
//      form of the reference's "already exists" (:423-428); the reference compares keyword bytes and would store two different
//      keywords of one hash, of which a client finds only the first (HashBucket.find(hash:)).  The number dropped is reported.
//   2. The random choice among the swappable slots is splitmix64 over the caller's seed, next() % candidateCount (the modulo
//      bias does not matter here); the reference draws from SystemRandomNumberGenerator and builds no reproducible table.
//   3. No entry is lost.  Where no resident value can be swapped out, the reference's insertLoop calls expand() and returns
//      without inserting the pair it holds (:449-457).  Here an expansion is a status: the caller places EVERY entry again in
//      the larger table, the held pair among them.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/he_amd.h"

namespace heamd {
void set_last_error(const std::string& message);
}

namespace {

constexpr uint64_t kMaxValueSize = 0xffff;  // HashBucketEntry.maxValueSize (HashBucket.swift:28-31)
constexpr uint32_t kMaxSlotCount = 0xff;    // HashBucket.maxSlotCount (HashBucket.swift:109)
constexpr uint64_t kSlotOverhead = 10;      // the keyword hash and the UInt16 value size (HashBucket.swift:82-87)

int fail(int status, const std::string& what) {
    heamd::set_last_error(what);
    return status;
}

uint64_t table_count(const he_cuckoo_table_config& c) { return c.multiple_tables ? c.hash_function_count : 1; }

uint64_t next_multiple(uint64_t value, uint64_t of) { return (value + of - 1) / of * of; }

int validate(const he_cuckoo_table_config* c) {
    if (c == nullptr) return fail(HE_ERR_INVALID_ARGUMENT, "invalid argument: null cuckoo table config");
    // HashBucket.serializedSize(singleValueSize: 0) = 1 + 10
    bool valid = c->hash_function_count > 0 && c->max_serialized_bucket_size >= 1 + kSlotOverhead && c->slot_count > 0 &&
                 c->slot_count <= kMaxSlotCount;
    if (c->fixed_size) {
        valid = valid && c->bucket_count > 0;
    } else {  // (a load factor that is not above 0: the reference would divide by it)
        valid = valid && c->expansion_factor > 1.0 && c->target_load_factor < 1.0 && c->target_load_factor > 0.0;
    }
    return valid ? HE_OK : fail(HE_ERR_INVALID_CUCKOO_CONFIG, "Invalid cuckoo table config");
}

struct SplitMix64 {
    uint64_t state;
    uint64_t next() {
        uint64_t z = (state += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
};

struct Bucket {
    std::vector<uint32_t> slots;  // entry indices
    uint64_t size = 1;            // HashBucket.serializedSize: the slot count byte and the records
};

}  // namespace

extern "C" int he_keyword_pir_config_validate(const he_cuckoo_table_config* config) { return validate(config); }

extern "C" int he_keyword_pir_bucket_count(const he_cuckoo_table_config* config, const uint64_t* value_sizes, size_t count,
                                           size_t* out) {
    const int status = validate(config);
    if (status != HE_OK) return status;
    if (out == nullptr || (value_sizes == nullptr && count != 0))
        return fail(HE_ERR_INVALID_ARGUMENT, "invalid argument: null pointer");
    const uint64_t tables = table_count(*config);
    if (config->fixed_size) {
        *out = next_multiple(config->bucket_count, tables);
        return HE_OK;
    }
    uint64_t serialized = 1;
    for (size_t i = 0; i < count; ++i) serialized += kSlotOverhead + value_sizes[i];
    const uint64_t least = (serialized + config->max_serialized_bucket_size - 1) / config->max_serialized_bucket_size;
    const double target = std::ceil(static_cast<double>(least) / config->target_load_factor);
    if (!(target < 4294967296.0)) return fail(HE_ERR_INVALID_ARGUMENT, "invalid argument: more than 2^32 - 1 buckets");
    *out = next_multiple(static_cast<uint64_t>(target), tables);
    return HE_OK;
}

extern "C" int he_keyword_pir_cuckoo_place(const he_cuckoo_table_config* config, const uint64_t* hashes,
                                           const uint32_t* indices, const uint64_t* value_sizes, size_t count,
                                           size_t bucket_count, uint64_t seed, uint32_t* out_bucket_offsets,
                                           uint32_t* out_slot_entries, size_t* out_placed, size_t* out_duplicates_dropped,
                                           size_t* out_next_bucket_count) {
    const int status = validate(config);
    if (status != HE_OK) return status;
    if (count != 0 && (hashes == nullptr || indices == nullptr || value_sizes == nullptr || out_slot_entries == nullptr))
        return fail(HE_ERR_INVALID_ARGUMENT, "invalid argument: null pointer");
    if (out_bucket_offsets == nullptr) return fail(HE_ERR_INVALID_ARGUMENT, "invalid argument: null pointer");
    if (count > 0xffffffffull) return fail(HE_ERR_INVALID_ARGUMENT, "invalid argument: more than 2^32 - 1 entries");
    const uint32_t h = config->hash_function_count;
    const uint64_t tables = table_count(*config), limit = config->max_serialized_bucket_size;
    if (bucket_count == 0 || bucket_count % tables != 0 || bucket_count > 0xffffffffull)
        return fail(HE_ERR_INVALID_ARGUMENT, "invalid argument: the bucket count is zero or no multiple of the table count");
    const uint64_t per_table = bucket_count / tables;
    for (size_t i = 0; i < count; ++i) {
        if (value_sizes[i] > kMaxValueSize)
            return fail(HE_ERR_INVALID_HASH_BUCKET_ENTRY_VALUE_SIZE, "Invalid hash bucket entry value size: maximum 65535");
        for (uint32_t t = 0; t < h; ++t)
            if (indices[i * h + t] >= per_table)
                return fail(HE_ERR_INVALID_ARGUMENT, "invalid argument: a candidate index is not below the buckets per table");
    }
    // index(tableIndex:index:) (:461-463)
    auto bucket_of = [&](uint32_t entry, uint32_t t) -> size_t {
        return tables == 1 ? indices[size_t(entry) * h + t] : t * per_table + indices[size_t(entry) * h + t];
    };
    auto needs_expansion = [&](const std::string& why) {
        if (config->fixed_size) return fail(HE_ERR_FAILED_TO_CONSTRUCT_CUCKOO_TABLE, why);
        const double grown = std::ceil(static_cast<double>(bucket_count) * config->expansion_factor);
        if (!(grown < 4294967296.0)) return fail(HE_ERR_FAILED_TO_CONSTRUCT_CUCKOO_TABLE, "Expanding Cuckoo table failed");
        if (out_next_bucket_count != nullptr) *out_next_bucket_count = next_multiple(static_cast<uint64_t>(grown), tables);
        return fail(HE_ERR_CUCKOO_TABLE_NEEDS_EXPANSION, why);
    };

    std::vector<Bucket> buckets(bucket_count);
    SplitMix64 rng{seed};
    size_t duplicates = 0;
    struct Swap {
        size_t bucket;
        uint32_t slot;
    };
    std::vector<Swap> swaps;
    for (size_t i = 0; i < count; ++i) {
        if (1 + kSlotOverhead + value_sizes[i] > limit)  // the guard of insert (:387-396)
            return fail(HE_ERR_FAILED_TO_CONSTRUCT_CUCKOO_TABLE,
                        "Unable to insert entry " + std::to_string(i) + " (" + std::to_string(value_sizes[i]) +
                            " byte value), because the resulting hashbucket would be larger than 'maxSerializedBucketSize'.");
        uint32_t held = static_cast<uint32_t>(i);
        for (uint32_t remaining = config->max_eviction_count;; --remaining) {  // insertLoop (:401-458)
            if (remaining == 0)
                return needs_expansion("Unable to insert entry " + std::to_string(held) +
                                       " within maxEvictionCount. Consider setting `allowExpansion` or increasing `bucketCount`.");
            bool exists = false;
            for (uint32_t t = 0; t < h && !exists; ++t)
                for (uint32_t resident : buckets[bucket_of(held, t)].slots) exists |= hashes[resident] == hashes[held];
            if (exists) {  // (an evicted entry never gets here: no two stored entries share a hash)
                ++duplicates;
                break;
            }
            const uint64_t record = kSlotOverhead + value_sizes[held];
            bool inserted = false;
            for (uint32_t t = 0; t < h && !inserted; ++t) {  // canInsert (:202-205)
                Bucket& b = buckets[bucket_of(held, t)];
                if (b.slots.size() < config->slot_count && b.size + record <= limit) {
                    b.slots.push_back(held);
                    b.size += record;
                    inserted = true;
                }
            }
            if (inserted) break;
            swaps.clear();
            for (uint32_t t = 0; t < h; ++t) {  // swapIndices (:209-217): the bucket with one resident value replaced still fits
                const size_t at = bucket_of(held, t);
                const Bucket& b = buckets[at];
                for (uint32_t slot = 0; slot < b.slots.size(); ++slot)
                    if (b.size - (kSlotOverhead + value_sizes[b.slots[slot]]) + record <= limit) swaps.push_back({at, slot});
            }
            if (swaps.empty()) return needs_expansion("No resident value of the candidate buckets can be swapped out");
            const Swap pick = swaps[rng.next() % swaps.size()];
            Bucket& b = buckets[pick.bucket];
            const uint32_t evicted = b.slots[pick.slot];
            b.size = b.size - (kSlotOverhead + value_sizes[evicted]) + record;
            b.slots[pick.slot] = held;
            held = evicted;
        }
    }
    uint32_t placed = 0;
    for (size_t b = 0; b < bucket_count; ++b) {
        out_bucket_offsets[b] = placed;
        for (uint32_t entry : buckets[b].slots) out_slot_entries[placed++] = entry;
    }
    out_bucket_offsets[bucket_count] = placed;
    if (out_placed != nullptr) *out_placed = placed;
    if (out_duplicates_dropped != nullptr) *out_duplicates_dropped = duplicates;
    return HE_OK;
}
