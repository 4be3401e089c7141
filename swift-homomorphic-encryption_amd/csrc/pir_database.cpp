// pir_database.cpp -- MulPirServer.process(database:with:using:) (reference Sources/PrivateInformationRetrieval/IndexPir/
// MulPir.swift:431-556) on the device: the host plan (chunk count, mode, validation in the reference's order) and the
// grouped pass that turns raw entry bytes into the [chunk][prod(dimensions)][L][N] Eval database and its present mask.
//
// Per group of database slots: the unpack kernel (pir_database_kernels.hip) writes the slots' coefficients into a staging slab
// and their present bytes, then Plaintext.convertToEvalFormat (he_bfv_plaintext_to_eval_device: centred lift fused into the
// forward NTT's load where the degree has a tiled kernel) takes the staging slab into the database.  A nil slot's bytes are
// all zero, so its staging row is zero and so is its Eval plaintext -- the layout every he_pir_compute_response_* reads.
#include <cstdlib>
#include <string>
#include <vector>

#include "api_internal.hpp"
#include "bfv_context.hpp"
#include "pir_database.hpp"

using heamd::as_stream;
using heamd::invalid_argument;
using heamd::Scratch;

namespace {

// the database plan of one (context, IndexPirParameter)
struct DatabasePlan {
    uint64_t chunk_count = 0, per_chunk = 0, bytes_per_plaintext = 0, entries_per_plaintext = 0, width = 0;
    heamd::PirDatabaseLayout layout;
};

// IndexPirConfig.entrySizeEncodingWidth (IndexPirProtocol.swift:106-120)
uint64_t encoding_width(uint64_t entry_size) {
    if (entry_size <= 0xffu) return 1;
    if (entry_size <= 0xffffu) return 2;
    if (entry_size <= 0xffffffffu) return 4;
    return 8;
}

int database_error(const std::string& what) {
    heamd::set_last_error("invalid argument: " + what);
    return HE_ERR_INVALID_ARGUMENT;
}

// MulPir.swift:433-450 and the shapes the reorders (:486-495, :545-553) need; entry_sizes (host) NULL: none to check
int database_plan(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count, size_t entry_count,
                  size_t entry_size_in_bytes, int encoding_entry_size, const uint64_t* entry_sizes, DatabasePlan& plan) {
    if (ctx == nullptr) return invalid_argument("null context");
    if (entry_sizes != nullptr) {
        uint64_t largest = 0;
        for (size_t e = 0; e < entry_count; ++e) largest = entry_sizes[e] > largest ? entry_sizes[e] : largest;
        if (largest > entry_size_in_bytes)  // PirError.invalidDatabaseEntrySize (PrivateInformationRetrieval/Util/Error.swift:82-85)
            return database_error("Invalid database: Database has entry with size " + std::to_string(largest) +
                                  " plaintexts, expected all entry sizes to be <= " + std::to_string(entry_size_in_bytes));
    }
    if (dimensions == nullptr || dimension_count == 0) return invalid_argument("empty dimensions");
    uint64_t per_chunk = 1;
    for (uint32_t i = 0; i < dimension_count; ++i) {
        if (dimensions[i] == 0) return invalid_argument("zero dimension");
        if (per_chunk > (uint64_t(1) << 40) / dimensions[i]) return invalid_argument("dimensions too large");
        per_chunk *= dimensions[i];
    }
    if (entry_size_in_bytes > (uint64_t(1) << 48)) return invalid_argument("entry size too large");
    const heamd::BfvContext& bfv = heamd::bfv_impl(ctx);
    const uint64_t t = bfv.plaintext_modulus();
    uint32_t bits = 0;
    while ((t >> (bits + 1)) != 0) ++bits;  // floor(log2 t) (EncryptionParameters.swift:101-110)
    const uint64_t n = bfv.degree();
    const uint64_t width = encoding_entry_size ? encoding_width(entry_size_in_bytes) : 0;
    const uint64_t encoded = width + entry_size_in_bytes;
    const uint64_t bpp = n * bits / 8;
    if (encoded == 0) return invalid_argument("entries of zero bytes without a size prefix");
    if (bpp == 0) return invalid_argument("plaintexts hold no byte");
    plan = DatabasePlan{};
    plan.per_chunk = per_chunk;
    plan.bytes_per_plaintext = bpp;
    plan.width = width;
    plan.chunk_count = (encoded + bpp - 1) / bpp;
    heamd::PirDatabaseLayout& l = plan.layout;
    l.entry_count = entry_count;
    l.entry_stride = entry_size_in_bytes;
    l.width = width;
    l.encoded = encoded;
    l.bytes_per_plaintext = bpp;
    l.per_chunk = per_chunk;
    l.d0 = dimensions[0];
    l.columns = per_chunk / dimensions[0];
    l.bits = bits;
    for (uint64_t m = n; m > 1; m >>= 1) ++l.log_degree;
    if (plan.chunk_count > 1) {  // processSplitLargeEntries: one row of chunk_count plaintexts per entry
        if (entry_count > per_chunk)
            return database_error("split mode: " + std::to_string(entry_count) + " entries do not fit " +
                                  std::to_string(per_chunk) + " plaintexts per chunk");
        l.plaintexts = entry_count;
    } else {  // processPackEntries: floor(bpp / encoded) entries per plaintext, none straddling two
        plan.entries_per_plaintext = bpp / encoded;
        l.packed_bytes = plan.entries_per_plaintext * encoded;
        l.plaintexts = (entry_count + plan.entries_per_plaintext - 1) / plan.entries_per_plaintext;
        if (l.plaintexts > per_chunk)
            return database_error("pack mode: " + std::to_string(l.plaintexts) + " plaintexts do not fit " +
                                  std::to_string(per_chunk) + " plaintexts per chunk");
    }
    return HE_OK;
}

// Slots per group: the staging slab stays near 1 GiB and no launch of a group reaches 2^31 lanes, however large the database.
// HEAMD_PIR_PROCESS_GROUP=<slots> forces smaller groups (the tests: many groups must give the words of one).
size_t group_slots(size_t n, uint32_t L, size_t word_bytes) {
    size_t slots = (size_t(1) << 30) / (n * word_bytes);
    const size_t ntt_bound = (size_t(1) << 30) / (n * L);  // the lift / transform launches: slots * L * N words
    if (ntt_bound < slots) slots = ntt_bound;
    if (const char* forced = std::getenv("HEAMD_PIR_PROCESS_GROUP")) {
        const size_t want = static_cast<size_t>(std::strtoull(forced, nullptr, 10));
        if (want != 0 && want < slots) slots = want;
    }
    return slots ? slots : 1;
}

int to_eval(const he_bfv_context* ctx, uint32_t L, const uint64_t* staging, uint64_t* out, size_t batch, he_stream s) {
    return he_bfv_plaintext_to_eval_device(ctx, L, staging, out, batch, s);
}
int to_eval(const he_bfv_context* ctx, uint32_t L, const uint32_t* staging, uint32_t* out, size_t batch, he_stream s) {
    return he_bfv_plaintext_to_eval_device_u32(ctx, L, staging, out, batch, s);
}

template <typename W>
int process_database(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count, const uint8_t* entries,
                     const uint64_t* entry_sizes, size_t entry_count, size_t entry_size_in_bytes, int encoding_entry_size,
                     W* database, uint8_t* present, he_stream s) {
    DatabasePlan plan;
    const int status = database_plan(ctx, dimensions, dimension_count, entry_count, entry_size_in_bytes, encoding_entry_size,
                                     entry_sizes, plan);
    if (status != HE_OK) return status;
    if (entries == nullptr && entry_count != 0 && entry_size_in_bytes != 0) return invalid_argument("null entries");
    if (database == nullptr || present == nullptr) return invalid_argument("null database");
    const heamd::BfvContext& bfv = heamd::bfv_impl(ctx);
    if (sizeof(W) == 4 && bfv.word_bits() != 32) return invalid_argument("4-byte slabs need a Bfv<UInt32> context");
    const uint32_t L = he_bfv_ciphertext_moduli_count(ctx);
    // the level checks of Plaintext.convertToEvalFormat (host-only context: HE_ERR_DEVICE) before anything is enqueued
    const int ready = to_eval(ctx, L, static_cast<const W*>(nullptr), static_cast<W*>(nullptr), 0, s);
    if (ready != HE_OK) return ready;
    hipStream_t stream = as_stream(s);
    const size_t n = bfv.degree();
    Scratch sizes_mem(stream);
    if (entry_sizes != nullptr && entry_count != 0) {
        HEAMD_HIP_TRY(sizes_mem.allocate(entry_count * sizeof(uint64_t)));
        HEAMD_HIP_TRY(hipMemcpyAsync(sizes_mem.get(), entry_sizes, entry_count * sizeof(uint64_t), hipMemcpyHostToDevice,
                                     stream));
        HEAMD_HIP_TRY(hipStreamSynchronize(stream));  // `entry_sizes` is a borrowed pageable host buffer
        plan.layout.entry_sizes = static_cast<const uint64_t*>(sizes_mem.get());
    }
    plan.layout.entries = entries;
    const size_t total = plan.chunk_count * plan.per_chunk;
    const size_t group = group_slots(n, L, sizeof(W));
    Scratch staging_mem(stream);
    HEAMD_HIP_TRY(staging_mem.allocate((total < group ? total : group) * n * sizeof(W)));
    W* staging = static_cast<W*>(staging_mem.get());
    for (size_t first = 0; first < total; first += group) {
        const size_t slots = total - first < group ? total - first : group;
        HEAMD_HIP_TRY(heamd::launch_pir_database_unpack<W>(plan.layout, first, slots, staging, present, stream));
        const int converted = to_eval(ctx, L, staging, database + first * L * n, slots, s);
        if (converted != HE_OK) return converted;
    }
    return HE_OK;
}

}  // namespace

extern "C" int he_pir_database_shape(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count,
                                     size_t entry_count, size_t entry_size_in_bytes, int encoding_entry_size,
                                     size_t* out_chunk_count, size_t* out_plaintexts_per_chunk,
                                     size_t* out_bytes_per_plaintext, size_t* out_entries_per_plaintext,
                                     size_t* out_entry_size_encoding_width) {
    DatabasePlan plan;
    const int status = database_plan(ctx, dimensions, dimension_count, entry_count, entry_size_in_bytes, encoding_entry_size,
                                     nullptr, plan);
    if (status != HE_OK) return status;
    if (out_chunk_count != nullptr) *out_chunk_count = plan.chunk_count;
    if (out_plaintexts_per_chunk != nullptr) *out_plaintexts_per_chunk = plan.per_chunk;
    if (out_bytes_per_plaintext != nullptr) *out_bytes_per_plaintext = plan.bytes_per_plaintext;
    if (out_entries_per_plaintext != nullptr) *out_entries_per_plaintext = plan.entries_per_plaintext;
    if (out_entry_size_encoding_width != nullptr) *out_entry_size_encoding_width = plan.width;
    return HE_OK;
}

extern "C" int he_pir_process_database_device(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count,
                                              const uint8_t* entries, const uint64_t* entry_sizes, size_t entry_count,
                                              size_t entry_size_in_bytes, int encoding_entry_size, uint64_t* database,
                                              uint8_t* present, he_stream s) {
    return process_database(ctx, dimensions, dimension_count, entries, entry_sizes, entry_count, entry_size_in_bytes,
                            encoding_entry_size, database, present, s);
}

extern "C" int he_pir_process_database_device_u32(const he_bfv_context* ctx, const uint32_t* dimensions,
                                                  uint32_t dimension_count, const uint8_t* entries,
                                                  const uint64_t* entry_sizes, size_t entry_count,
                                                  size_t entry_size_in_bytes, int encoding_entry_size, uint32_t* database,
                                                  uint8_t* present, he_stream s) {
    return process_database(ctx, dimensions, dimension_count, entries, entry_sizes, entry_count, entry_size_in_bytes,
                            encoding_entry_size, database, present, s);
}
