// simple_pir_api.cpp -- SimplePirServer (reference Sources/PrivateInformationRetrieval/SimplePir/) behind the C ABI: the
// plan (computingParams), process (database and hint) and computeResponse.  Kernels: simple_pir_kernels.hip, and
// simple_pir_matrix_kernels.hip for the batch entries (path and tile: simple_pir_batch_plan.hpp).
//
// The hint, database x A mod p with A the concatenated transposed negacyclic matrices of the seeded polynomials a_k
// (SimplePir+Database.swift:178-206,252-290), is never formed from a materialised A.  Row i of negacyclicMatrix() is
// a x^i, so column j of the transposed block is a x^j and, with d_{r,k} the k-th block of N elements of database row r,
//     hint[r][j] = sum_k <d_{r,k}, a_k x^j> = sum_k (d_{r,k} * sigma(a_k))[j],   sigma: x -> x^(2N-1) = x^-1,
// a sum of negacyclic products: per block of rows, widen -> forward NTT -> multiply-accumulate over k -> inverse NTT.
#include <cmath>
#include <cstdlib>
#include <memory>
#include <vector>

#include "api_internal.hpp"
#include "kernels.hpp"
#include "simple_pir_batch_plan.hpp"
#include "simple_pir_context.hpp"

using heamd::as_stream;
using heamd::invalid_argument;
using heamd::Scratch;
using heamd::SimplePirPlan;

namespace {

uint32_t element_bytes_of(uint32_t plaintext_bits) {
    return plaintext_bits <= 8 ? 1 : plaintext_bits <= 16 ? 2 : plaintext_bits <= 32 ? 4 : 8;
}

// SimplePirEncryptionParams.init's guards (SimplePir.swift:56-65) and what the word holds: the NTT-friendly modulus has
// ciphertext_bits + 1 significant bits and must be a PolyRq<UInt32> modulus (<= 2^30 - 1) or stay below 2^61
int check_bits(uint32_t plaintext_bits, uint32_t ciphertext_bits, uint32_t word_bits) {
    if (word_bits != 32 && word_bits != 64) return invalid_argument("word_bits must be 32 or 64");
    if (plaintext_bits == 0) return invalid_argument("plaintext_bits must be positive");
    if (ciphertext_bits <= plaintext_bits) return invalid_argument("ciphertext_bits must be > plaintext_bits");
    if (ciphertext_bits > (word_bits == 32 ? 29u : 60u)) return invalid_argument("ciphertext_bits does not fit the word");
    return HE_OK;
}

}  // namespace

// computingParams (SimplePir+Database.swift:209-243), the padded column size of process (:262-268) and SimplePirContext.init's
// modulus (SimplePirContext.swift:76-87).  Double.rounded() rounds halves away from zero, as std::round does.
int heamd::simple_pir_plan(uint32_t plaintext_bits, uint32_t ciphertext_bits, uint32_t lattice_dimension, uint32_t word_bits,
                           size_t entry_count, size_t entry_size_in_bytes, SimplePirPlan& plan) {
    const int status = check_bits(plaintext_bits, ciphertext_bits, word_bits);
    if (status != HE_OK) return status;
    if (lattice_dimension < 2 || (lattice_dimension & (lattice_dimension - 1)) != 0)
        return invalid_argument("lattice_dimension must be a power of two");
    if (entry_count == 0 || entry_size_in_bytes == 0) return invalid_argument("empty database");
    if (entry_size_in_bytes > (size_t(1) << 40) || entry_count > (size_t(1) << 40)) return invalid_argument("database too large");
    plan = SimplePirPlan{};
    plan.plaintext_bits = plaintext_bits;
    plan.ciphertext_bits = ciphertext_bits;
    plan.lattice_dimension = lattice_dimension;
    plan.word_bits = word_bits;
    plan.element_bytes = element_bytes_of(plaintext_bits);
    plan.entry_count = entry_count;
    plan.entry_size_in_bytes = entry_size_in_bytes;
    const size_t scalars = (8 * entry_size_in_bytes + plaintext_bits - 1) / plaintext_bits;
    if (scalars > (size_t(1) << 52) / entry_count) return invalid_argument("database too large");
    const size_t database_size = entry_count * scalars;
    size_t ideal_column_size = static_cast<size_t>(std::round(std::sqrt(static_cast<double>(database_size))));
    if (ideal_column_size > scalars) ideal_column_size = scalars;
    const size_t ideal_entries =
        static_cast<size_t>(std::round(static_cast<double>(ideal_column_size) / static_cast<double>(scalars)));
    const size_t entries_per_column = ideal_entries > 1 ? ideal_entries : 1;
    // Int(Double(entrySizeInScalar) / Double(idealColumnSize).rounded()): only the divisor is rounded, the quotient truncates
    const size_t ideal_chunks =
        static_cast<size_t>(static_cast<double>(scalars) / std::round(static_cast<double>(ideal_column_size)));
    const size_t chunks_per_entry = ideal_chunks > 1 ? ideal_chunks : 1;
    if (entries_per_column != 1 && chunks_per_entry != 1)  // SimplePirParameters.init's precondition (SimplePir.swift:157)
        return invalid_argument("entries_per_column and chunks_per_entry both above 1");
    size_t columns;
    if (entries_per_column == 1) {
        columns = entry_count * chunks_per_entry;
    } else {
        columns = (entry_count + entries_per_column - 1) / entries_per_column;
        if (columns < 1) columns = 1;
    }
    const size_t padded =
        chunks_per_entry == 1 ? scalars : (scalars + chunks_per_entry - 1) / chunks_per_entry * chunks_per_entry;
    plan.entry_size_in_scalar = scalars;
    plan.entries_per_column = entries_per_column;
    plan.chunks_per_entry = chunks_per_entry;
    plan.database_columns = columns;
    plan.padded_entry_size = padded;
    plan.column_size = padded * entries_per_column / chunks_per_entry;
    plan.a_poly_count = (columns + lattice_dimension - 1) / lattice_dimension;
    std::vector<heamd::u64> primes;
    if (!heamd::generate_primes({static_cast<int>(ciphertext_bits) + 1}, true, lattice_dimension, primes))
        return HE_ERR_NOT_ENOUGH_PRIMES;
    plan.modulus = primes[0];
    return HE_OK;
}

using heamd::simple_pir_plan;

namespace {

// Rows per block of the hint: the widened staging slab ([rows][a_poly_count][N] 8-byte words) stays near 1 GiB.
// HEAMD_SIMPLE_PIR_ROW_BLOCK=<rows> forces smaller blocks (the tests: many blocks must give the words of one).
size_t hint_row_block(const SimplePirPlan& plan) {
    size_t rows = (size_t(1) << 27) / (plan.a_poly_count * plan.lattice_dimension);
    if (const char* forced = std::getenv("HEAMD_SIMPLE_PIR_ROW_BLOCK")) {
        const size_t want = static_cast<size_t>(std::strtoull(forced, nullptr, 10));
        if (want != 0 && want < rows) rows = want;
    }
    return rows ? rows : 1;
}

hipError_t store_hint(const uint64_t* rows, uint64_t* hint, size_t words, hipStream_t stream) {
    return hipMemcpyAsync(hint, rows, words * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream);
}
hipError_t store_hint(const uint64_t* rows, uint32_t* hint, size_t words, hipStream_t stream) {
    return heamd::launch_narrow_words(rows, hint, words, stream);
}

template <typename W>
int process_database(const he_simple_pir_context* ctx, const uint8_t* entries, const uint8_t* seed, void* database, W* hint,
                     he_stream s) {
    if (ctx == nullptr) return invalid_argument("null context");
    const SimplePirPlan& plan = ctx->plan;
    if (plan.word_bits != 8 * sizeof(W)) return invalid_argument("context of the other word size");
    if (entries == nullptr || seed == nullptr || database == nullptr || hint == nullptr) return invalid_argument("null buffer");
    if ((reinterpret_cast<uintptr_t>(hint) & 15u) != 0) return invalid_argument("hint must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(database) & (plan.element_bytes - 1)) != 0)
        return invalid_argument("database must be aligned to element_bytes");
    const heamd::PolyContext& ring = *ctx->ring;
    const int status = ring.check_device();
    if (status != HE_OK) return status;
    hipStream_t stream = as_stream(s);
    const heamd::DeviceContext dc = ring.device_context();
    const size_t n = plan.lattice_dimension;
    const uint32_t blocks = static_cast<uint32_t>(plan.a_poly_count);

    heamd::SimplePirLayout layout{};
    layout.entry_count = plan.entry_count;
    layout.entry_size_in_bytes = plan.entry_size_in_bytes;
    layout.entry_size_in_scalar = plan.entry_size_in_scalar;
    layout.padded_entry_size = plan.padded_entry_size;
    layout.column_size = plan.column_size;
    layout.database_columns = plan.database_columns;
    layout.plaintext_bits = plan.plaintext_bits;
    layout.element_bytes = plan.element_bytes;
    HEAMD_HIP_TRY(heamd::launch_simple_pir_database(layout, entries, database, stream));

    // generateAPolynomials (SimplePir+Database.swift:178-181): a_poly_count polynomials drawn one after the other from ONE
    // NistAes128Ctr(seed) -- the stream of a single "polynomial" of a_poly_count rows over the same modulus
    Scratch table_mem(stream), chain_mem(stream), a_mem(stream), a_eval_mem(stream);
    HEAMD_HIP_TRY(table_mem.allocate(blocks * sizeof(heamd::DeviceModulus)));
    heamd::DeviceModulus* table = static_cast<heamd::DeviceModulus*>(table_mem.get());
    HEAMD_HIP_TRY(heamd::launch_simple_pir_replicate_modulus(dc, table, blocks, stream));
    heamd::DeviceContext stream_ctx = dc;
    stream_ctx.moduli = table;
    stream_ctx.moduli_count = blocks;
    HEAMD_HIP_TRY(chain_mem.allocate(heamd::seeded_uniform_scratch_bytes(stream_ctx, 1)));
    HEAMD_HIP_TRY(a_mem.allocate(blocks * n * sizeof(uint64_t)));
    HEAMD_HIP_TRY(a_eval_mem.allocate(blocks * n * sizeof(uint64_t)));
    uint64_t* a = static_cast<uint64_t*>(a_mem.get());
    uint64_t* a_eval = static_cast<uint64_t*>(a_eval_mem.get());
    HEAMD_HIP_TRY(heamd::launch_seeded_uniform(seed, a, size_t(0), stream_ctx, 1, chain_mem.get(), stream));
    // sigma(a_k) = a_k(x^(2N-1)); 2N - 1 is its own inverse mod 2N
    HEAMD_HIP_TRY(heamd::launch_galois_coeff<uint64_t>(a, a_eval, dc, static_cast<uint32_t>(2 * n - 1), blocks, stream));
    HEAMD_HIP_TRY(heamd::launch_ntt(false, a_eval, dc, 0, 1, blocks, stream));

    const size_t group = hint_row_block(plan);
    const size_t most = plan.column_size < group ? plan.column_size : group;
    // the accumulator restarts from a reduced word (< p), so one product fewer than maxLazyProductAccumulationCount fits
    const uint64_t lazy = ring.max_lazy_product_accumulation_count(1);
    const uint64_t cadence = lazy > 2 ? lazy - 1 : 1;
    Scratch staging_mem(stream), rows_mem(stream);
    HEAMD_HIP_TRY(staging_mem.allocate(most * blocks * n * sizeof(uint64_t)));
    HEAMD_HIP_TRY(rows_mem.allocate(most * n * sizeof(uint64_t)));
    uint64_t* staging = static_cast<uint64_t*>(staging_mem.get());
    uint64_t* rows_out = static_cast<uint64_t*>(rows_mem.get());
    for (size_t first = 0; first < plan.column_size; first += group) {
        const size_t rows = plan.column_size - first < group ? plan.column_size - first : group;
        HEAMD_HIP_TRY(heamd::launch_simple_pir_widen(database, plan.element_bytes, plan.database_columns, first, rows, blocks,
                                                     dc.log_degree, staging, stream));
        HEAMD_HIP_TRY(heamd::launch_ntt(false, staging, dc, 0, 1, rows * blocks, stream));
        HEAMD_HIP_TRY(heamd::launch_simple_pir_hint_mac(staging, a_eval, rows_out, rows, blocks, cadence, dc, stream));
        HEAMD_HIP_TRY(heamd::launch_ntt(true, rows_out, dc, 0, 1, rows, stream));
        HEAMD_HIP_TRY(store_hint(rows_out, hint + first * n, rows * n, stream));
    }
    return HE_OK;
}

int check_database_call(uint32_t plaintext_bits, uint32_t word_bits, const void* a, const void* b, size_t elements) {
    if (plaintext_bits == 0 || plaintext_bits > word_bits) return invalid_argument("plaintext_bits does not fit the word");
    if (elements != 0 && (a == nullptr || b == nullptr)) return invalid_argument("null buffer");
    const uintptr_t both = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b);
    if ((both & (element_bytes_of(plaintext_bits) - 1)) != 0) return invalid_argument("database must be aligned to element_bytes");
    return HE_OK;
}

template <typename W>
int compute_response(uint32_t plaintext_bits, uint32_t ciphertext_bits, const void* database, size_t column_size,
                     size_t database_columns, const W* requests, size_t query_count, W* responses, he_stream s) {
    if (plaintext_bits == 0 || ciphertext_bits <= plaintext_bits) return invalid_argument("ciphertext_bits must be > plaintext_bits");
    if (ciphertext_bits > 8 * sizeof(W)) return invalid_argument("ciphertext_bits does not fit the word");
    if (column_size == 0 || database_columns == 0 || query_count == 0) return HE_OK;
    if (database == nullptr || requests == nullptr || responses == nullptr) return invalid_argument("null buffer");
    if ((reinterpret_cast<uintptr_t>(database) & (element_bytes_of(plaintext_bits) - 1)) != 0)
        return invalid_argument("database must be aligned to element_bytes");
    HEAMD_HIP_TRY(heamd::launch_simple_pir_response<W>(database, element_bytes_of(plaintext_bits), column_size,
                                                       database_columns, requests, query_count, responses, ciphertext_bits,
                                                       as_stream(s)));
    return HE_OK;
}

// The checks shared by computeResponse's entries and the batch plan, in the order of compute_response above
int check_response_bits(uint32_t plaintext_bits, uint32_t ciphertext_bits, uint32_t word_bits) {
    if (plaintext_bits == 0 || ciphertext_bits <= plaintext_bits) return invalid_argument("ciphertext_bits must be > plaintext_bits");
    if (ciphertext_bits > word_bits) return invalid_argument("ciphertext_bits does not fit the word");
    return HE_OK;
}

// computeResponse for large batches: the int8 matrix kernel where the plan has one, the existing launcher elsewhere
template <typename W>
int compute_response_batch(uint32_t plaintext_bits, uint32_t ciphertext_bits, const void* database, size_t column_size,
                           size_t database_columns, const W* requests, size_t query_count, W* responses, he_stream s) {
    const int status = check_response_bits(plaintext_bits, ciphertext_bits, 8 * sizeof(W));
    if (status != HE_OK) return status;
    if (column_size == 0 || database_columns == 0 || query_count == 0) return HE_OK;
    if (database == nullptr || requests == nullptr || responses == nullptr) return invalid_argument("null buffer");
    if ((reinterpret_cast<uintptr_t>(database) & (element_bytes_of(plaintext_bits) - 1)) != 0)
        return invalid_argument("database must be aligned to element_bytes");
    const heamd::simple_pir_batch::Plan plan = heamd::simple_pir_batch::plan_for(plaintext_bits, ciphertext_bits, 8 * sizeof(W));
    if (plan.matrix_path) {
        HEAMD_HIP_TRY(heamd::launch_simple_pir_matrix_response<W>(database, plan.database_limbs, column_size, database_columns,
                                                                  requests, query_count, responses, ciphertext_bits,
                                                                  plan.fold_columns, as_stream(s)));
    } else {
        HEAMD_HIP_TRY(heamd::launch_simple_pir_response<W>(database, element_bytes_of(plaintext_bits), column_size,
                                                           database_columns, requests, query_count, responses,
                                                           ciphertext_bits, as_stream(s)));
    }
    return HE_OK;
}

}  // namespace

extern "C" int he_simple_pir_shape(uint32_t plaintext_bits, uint32_t ciphertext_bits, uint32_t lattice_dimension,
                                   uint32_t word_bits, size_t entry_count, size_t entry_size_in_bytes,
                                   size_t* out_entry_size_in_scalar, size_t* out_entries_per_column,
                                   size_t* out_chunks_per_entry, size_t* out_database_columns, size_t* out_column_size,
                                   size_t* out_a_poly_count, uint64_t* out_modulus, uint32_t* out_element_bytes) {
    SimplePirPlan plan;
    const int status =
        simple_pir_plan(plaintext_bits, ciphertext_bits, lattice_dimension, word_bits, entry_count, entry_size_in_bytes, plan);
    if (status != HE_OK) return status;
    if (out_entry_size_in_scalar != nullptr) *out_entry_size_in_scalar = plan.entry_size_in_scalar;
    if (out_entries_per_column != nullptr) *out_entries_per_column = plan.entries_per_column;
    if (out_chunks_per_entry != nullptr) *out_chunks_per_entry = plan.chunks_per_entry;
    if (out_database_columns != nullptr) *out_database_columns = plan.database_columns;
    if (out_column_size != nullptr) *out_column_size = plan.column_size;
    if (out_a_poly_count != nullptr) *out_a_poly_count = plan.a_poly_count;
    if (out_modulus != nullptr) *out_modulus = plan.modulus;
    if (out_element_bytes != nullptr) *out_element_bytes = plan.element_bytes;
    return HE_OK;
}

extern "C" int he_simple_pir_context_create(uint32_t plaintext_bits, uint32_t ciphertext_bits, uint32_t lattice_dimension,
                                            uint32_t word_bits, size_t entry_count, size_t entry_size_in_bytes,
                                            he_simple_pir_context** out) {
    if (out == nullptr) return invalid_argument("null out");
    *out = nullptr;
    auto ctx = std::make_unique<he_simple_pir_context>();
    int status = simple_pir_plan(plaintext_bits, ciphertext_bits, lattice_dimension, word_bits, entry_count,
                                 entry_size_in_bytes, ctx->plan);
    if (status != HE_OK) return status;
    if (ctx->plan.a_poly_count > (size_t(1) << 20)) return invalid_argument("too many database columns");
    status = heamd::PolyContext::create(lattice_dimension, &ctx->plan.modulus, 1, ctx->ring);
    if (status != HE_OK) return status;
    *out = ctx.release();
    return HE_OK;
}

extern "C" void he_simple_pir_context_destroy(he_simple_pir_context* ctx) {
    heamd::RelaxedCapture relaxed;
    delete ctx;
}

extern "C" int he_simple_pir_process_database_device(const he_simple_pir_context* ctx, const uint8_t* entries,
                                                     const uint8_t* seed, void* database, uint64_t* hint, he_stream s) {
    return process_database(ctx, entries, seed, database, hint, s);
}

extern "C" int he_simple_pir_process_database_device_u32(const he_simple_pir_context* ctx, const uint8_t* entries,
                                                         const uint8_t* seed, void* database, uint32_t* hint, he_stream s) {
    return process_database(ctx, entries, seed, database, hint, s);
}

extern "C" int he_simple_pir_pack_database_device(uint32_t plaintext_bits, const uint64_t* wide, void* database,
                                                  size_t elements, he_stream s) {
    const int status = check_database_call(plaintext_bits, 64, wide, database, elements);
    if (status != HE_OK) return status;
    HEAMD_HIP_TRY(heamd::launch_simple_pir_pack<uint64_t>(wide, database, element_bytes_of(plaintext_bits), plaintext_bits,
                                                          elements, as_stream(s)));
    return HE_OK;
}

extern "C" int he_simple_pir_pack_database_device_u32(uint32_t plaintext_bits, const uint32_t* wide, void* database,
                                                      size_t elements, he_stream s) {
    const int status = check_database_call(plaintext_bits, 32, wide, database, elements);
    if (status != HE_OK) return status;
    HEAMD_HIP_TRY(heamd::launch_simple_pir_pack<uint32_t>(wide, database, element_bytes_of(plaintext_bits), plaintext_bits,
                                                          elements, as_stream(s)));
    return HE_OK;
}

extern "C" int he_simple_pir_unpack_database_device(uint32_t plaintext_bits, const void* database, uint64_t* wide,
                                                    size_t elements, he_stream s) {
    const int status = check_database_call(plaintext_bits, 64, database, wide, elements);
    if (status != HE_OK) return status;
    HEAMD_HIP_TRY(heamd::launch_simple_pir_unpack<uint64_t>(database, element_bytes_of(plaintext_bits), wide, elements,
                                                            as_stream(s)));
    return HE_OK;
}

extern "C" int he_simple_pir_unpack_database_device_u32(uint32_t plaintext_bits, const void* database, uint32_t* wide,
                                                        size_t elements, he_stream s) {
    const int status = check_database_call(plaintext_bits, 32, database, wide, elements);
    if (status != HE_OK) return status;
    HEAMD_HIP_TRY(heamd::launch_simple_pir_unpack<uint32_t>(database, element_bytes_of(plaintext_bits), wide, elements,
                                                            as_stream(s)));
    return HE_OK;
}

extern "C" int he_simple_pir_compute_response_device(uint32_t plaintext_bits, uint32_t ciphertext_bits, const void* database,
                                                     size_t column_size, size_t database_columns, const uint64_t* requests,
                                                     size_t query_count, uint64_t* responses, he_stream s) {
    return compute_response(plaintext_bits, ciphertext_bits, database, column_size, database_columns, requests, query_count,
                            responses, s);
}

extern "C" int he_simple_pir_compute_response_device_u32(uint32_t plaintext_bits, uint32_t ciphertext_bits,
                                                         const void* database, size_t column_size, size_t database_columns,
                                                         const uint32_t* requests, size_t query_count, uint32_t* responses,
                                                         he_stream s) {
    return compute_response(plaintext_bits, ciphertext_bits, database, column_size, database_columns, requests, query_count,
                            responses, s);
}

extern "C" int he_simple_pir_compute_response_batch_device(uint32_t plaintext_bits, uint32_t ciphertext_bits,
                                                           const void* database, size_t column_size, size_t database_columns,
                                                           const uint64_t* requests, size_t query_count, uint64_t* responses,
                                                           he_stream s) {
    return compute_response_batch(plaintext_bits, ciphertext_bits, database, column_size, database_columns, requests,
                                  query_count, responses, s);
}

extern "C" int he_simple_pir_compute_response_batch_device_u32(uint32_t plaintext_bits, uint32_t ciphertext_bits,
                                                               const void* database, size_t column_size,
                                                               size_t database_columns, const uint32_t* requests,
                                                               size_t query_count, uint32_t* responses, he_stream s) {
    return compute_response_batch(plaintext_bits, ciphertext_bits, database, column_size, database_columns, requests,
                                  query_count, responses, s);
}

extern "C" int he_simple_pir_batch_response_plan(uint32_t plaintext_bits, uint32_t ciphertext_bits, uint32_t word_bits,
                                                 size_t database_columns, size_t query_count, uint32_t* out_matrix_path,
                                                 uint32_t* out_database_limbs, uint32_t* out_request_limbs,
                                                 uint32_t* out_requests_per_pass, size_t* out_fold_columns,
                                                 size_t* out_workspace_bytes) {
    if (word_bits != 32 && word_bits != 64) return invalid_argument("word_bits must be 32 or 64");
    const int status = check_response_bits(plaintext_bits, ciphertext_bits, word_bits);
    if (status != HE_OK) return status;
    // the tile depends on the widths alone today; the shape is part of the question so that a later split over the columns
    // or a pre-split of the requests into scratch can answer it without another entry
    (void)database_columns;
    (void)query_count;
    const heamd::simple_pir_batch::Plan plan = heamd::simple_pir_batch::plan_for(plaintext_bits, ciphertext_bits, word_bits);
    if (out_matrix_path != nullptr) *out_matrix_path = plan.matrix_path;
    if (out_database_limbs != nullptr) *out_database_limbs = plan.database_limbs;
    if (out_request_limbs != nullptr) *out_request_limbs = plan.request_limbs;
    if (out_requests_per_pass != nullptr) *out_requests_per_pass = plan.requests_per_pass;
    if (out_fold_columns != nullptr) *out_fold_columns = plan.fold_columns;
    if (out_workspace_bytes != nullptr) *out_workspace_bytes = plan.workspace_bytes;
    return HE_OK;
}
