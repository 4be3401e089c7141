// simple_pir_client_api.cpp -- the SimplePIR client (reference Sources/PrivateInformationRetrieval/SimplePir/
// SimplePir+Client.swift, SimplePir+Precompute.swift:191-311) behind the C ABI: the host plan of simple_pir_client_plan.hpp, the
// a-polynomials DefaultQueryGenerator caches, batches of PrecomputedQueries.WithoutIndices -- encryptZero and the product of the
// ternary secrets with the hint on the same resident secrets --, add(index:) and the decryption of responses.  Kernels:
// simple_pir_client_kernels.hip, the seeded samplers and the transforms.
// Every random value is a function of a caller-supplied 32-byte seed through NistAes128Ctr(seed:).  The workspace is the caller's;
// whatever a call parks there depends on secrets, errors, indices or entries, and is set to zero on the stream when the call is
// done with it, however it ends (ZeroizedWorkspace, the helper and the rule of encrypt_api.cpp).  The word check, the word
// dispatch and the host-only refusal: word_layer.hpp.  (The plan keeps part sizes: a host probe and a Python mirror hold it.)
#include <cstdlib>

#include "aes_ctr_drbg.hpp"
#include "api_internal.hpp"
#include "encrypt_kernels.hpp"
#include "kernels.hpp"
#include "simple_pir_client_kernels.hpp"
#include "simple_pir_client_plan.hpp"
#include "simple_pir_context.hpp"
#include "word_layer.hpp"
#include "zeroized_workspace.hpp"

using heamd::as_stream;
using heamd::DeviceContext;
using heamd::invalid_argument;
using heamd::PolyContext;
using heamd::SimplePirPlan;
using heamd::ZeroizedWorkspace;
namespace client = heamd::simple_pir_client;

static_assert(sizeof(heamd::DeviceModulus) == client::kDeviceModulusBytes, "simple_pir_client_plan.hpp sizes the modulus table");
static_assert(heamd::kChainRecordBytes == client::kChainRecordBytes, "simple_pir_client_plan.hpp sizes the DRBG records");

extern "C++" {
namespace {

client::Shape shape_of(const SimplePirPlan& plan) {
    client::Shape s;
    s.plaintext_bits = plan.plaintext_bits;
    s.ciphertext_bits = plan.ciphertext_bits;
    s.lattice_dimension = plan.lattice_dimension;
    s.word_bits = plan.word_bits;
    s.entry_count = plan.entry_count;
    s.entry_size_in_bytes = plan.entry_size_in_bytes;
    s.entry_size_in_scalar = plan.entry_size_in_scalar;
    s.entries_per_column = plan.entries_per_column;
    s.chunks_per_entry = plan.chunks_per_entry;
    s.database_columns = plan.database_columns;
    s.column_size = plan.column_size;
    s.a_poly_count = plan.a_poly_count;
    s.modulus = plan.modulus;
    return s;
}

// HEAMD_SIMPLE_PIR_CLIENT_ROW_BLOCK=<rows> forces smaller blocks of staged secret rows (the tests: many blocks must give the
// words of one)
size_t forced_row_block() {
    const char* forced = std::getenv("HEAMD_SIMPLE_PIR_CLIENT_ROW_BLOCK");
    return forced != nullptr ? static_cast<size_t>(std::strtoull(forced, nullptr, 10)) : 0;
}

int client_plan(const SimplePirPlan& shape, int error_std_dev, size_t batch, client::Plan& plan) {
    client::ErrorSampler sampler;
    if (!client::error_sampler(error_std_dev, sampler)) return invalid_argument("unknown error standard deviation");
    if (batch > client::kMaxBatch) return invalid_argument("too many queries for one call");
    if (!client::plan(shape_of(shape), error_std_dev, batch, forced_row_block(), plan)) return invalid_argument("no plan");
    if (plan.error_chunks > 0xffffffffull) return invalid_argument("error stream too long");
    return HE_OK;
}

// the checks every device entry makes first, in this order: the word, the context, the word against the context's
int check_word_and_context(const he_simple_pir_context* ctx, uint32_t word_bits) {
    HEAMD_TRY_STATUS(heamd::check_word_bits(word_bits));
    if (ctx == nullptr) return invalid_argument("null context");
    if (ctx->plan.word_bits != word_bits) return invalid_argument("context of the other word size");
    return HE_OK;
}

// a workspace of `needed` bytes: the caller's, 16-byte aligned (the entries take no scratch of the library's)
int resolve_workspace(ZeroizedWorkspace& ws, void* workspace, size_t workspace_bytes, size_t needed) {
    if (workspace == nullptr) return invalid_argument("null workspace");
    return ws.resolve(workspace, workspace_bytes, needed);
}

heamd::SimplePirClientLayout layout_of(const SimplePirPlan& shape, const client::Plan& plan) {
    heamd::SimplePirClientLayout layout{};
    layout.chunks = shape.chunks_per_entry;
    layout.entries_per_column = shape.entries_per_column;
    layout.database_columns = shape.database_columns;
    layout.column_size = shape.column_size;
    layout.chunk_size = plan.chunk_size;
    layout.entry_count = shape.entry_count;
    layout.entry_size_in_bytes = shape.entry_size_in_bytes;
    layout.shift = shape.ciphertext_bits - shape.plaintext_bits;
    layout.delta = uint64_t(1) << layout.shift;                // SimplePirEncryptionParams.getDelta
    layout.mask = (uint64_t(1) << shape.ciphertext_bits) - 1;  // getCiphertextMask
    layout.plaintext_bits = shape.plaintext_bits;
    return layout;
}

// ---- generateAPolynomials + convertToEvalFormat ---------------------------------------------------------------------------------
hipError_t store_words(const uint64_t* rows, uint32_t* out, size_t words, hipStream_t stream) {
    return heamd::launch_narrow_words(rows, out, words, stream);
}
hipError_t store_words(const uint64_t*, uint64_t*, size_t, hipStream_t) { return hipSuccess; }  // drawn in place

template <typename W>
int a_polynomials(const he_simple_pir_context* ctx, const client::Plan& plan, const uint8_t* seed, W* out, uint8_t* ws,
                  hipStream_t stream) {
    const PolyContext& ring = *ctx->ring;
    const DeviceContext dc = ring.device_context();
    const uint32_t blocks = static_cast<uint32_t>(ctx->plan.a_poly_count);
    const size_t words = size_t(blocks) * ctx->plan.lattice_dimension;
    // ONE NistAes128Ctr(seed) for all a_poly_count polynomials (SimplePir+Database.swift:178-181): the stream of a single
    // "polynomial" of a_poly_count rows over the same modulus, as process draws them
    heamd::DeviceModulus* table = reinterpret_cast<heamd::DeviceModulus*>(ws);
    HEAMD_HIP_TRY(heamd::launch_simple_pir_replicate_modulus(dc, table, blocks, stream));
    DeviceContext stream_ctx = dc;
    stream_ctx.moduli = table;
    stream_ctx.moduli_count = blocks;
    uint64_t* wide = sizeof(W) == 8 ? reinterpret_cast<uint64_t*>(out)
                                    : reinterpret_cast<uint64_t*>(ws + plan.a_table_bytes + plan.a_chain_bytes);
    HEAMD_HIP_TRY(heamd::launch_seeded_uniform(seed, wide, size_t(0), stream_ctx, 1, ws + plan.a_table_bytes, stream));
    HEAMD_HIP_TRY(heamd::launch_ntt(false, wide, dc, 0, 1, blocks, stream));
    HEAMD_HIP_TRY(store_words(wide, out, words, stream));
    return HE_OK;
}

// ---- encryptZero ------------------------------------------------------------------------------------------------------------------
// `ws`: [error chain | secrets in Eval form | staged sample] (client::Plan)
template <typename W>
int encrypt_zero(const he_simple_pir_context* ctx, const client::Plan& plan, const W* a_eval, const W* secrets,
                 const uint8_t* error_seeds, W* queries, size_t batch, uint8_t* ws, hipStream_t stream) {
    const SimplePirPlan& shape = ctx->plan;
    const DeviceContext dc = ctx->ring->device_context();
    const uint32_t blocks = static_cast<uint32_t>(shape.a_poly_count);
    const size_t n = shape.lattice_dimension, row_words = size_t(blocks) * n;
    uint32_t* chain = reinterpret_cast<uint32_t*>(ws);
    uint64_t* secret_eval = reinterpret_cast<uint64_t*>(ws + plan.error_chain_bytes);
    uint64_t* staging = reinterpret_cast<uint64_t*>(ws + plan.error_chain_bytes + plan.secret_eval_bytes);
    // the refill chain of every query's error generator: serial per seed, parallel across the batch
    HEAMD_HIP_TRY(heamd::launch_seeded_chain(error_seeds, chain, batch, static_cast<uint32_t>(plan.error_chunks), stream));
    const client::Division division = client::division_for(shape.modulus, shape.ciphertext_bits);
    for (size_t first = 0; first < plan.rows; first += plan.row_block) {
        const size_t rows = plan.rows - first < plan.row_block ? plan.rows - first : plan.row_block;
        // noiselessSample (SimplePir+Client.swift:29-50): NTT(s), a_k NTT(s) for every k, back to Coeff, cut to database_columns
        HEAMD_HIP_TRY(heamd::launch_simple_pir_client_widen(secrets + first * n, secret_eval, rows * n, stream));
        HEAMD_HIP_TRY(heamd::launch_ntt(false, secret_eval, dc, 0, 1, rows, stream));
        HEAMD_HIP_TRY(heamd::launch_simple_pir_client_products(a_eval, secret_eval, staging, rows, blocks, dc, stream));
        HEAMD_HIP_TRY(heamd::launch_ntt(true, staging, dc, 0, 1, rows * blocks, stream));
        // modSwitch, the error, the mask (:64-81)
        HEAMD_HIP_TRY(heamd::launch_simple_pir_client_finish(staging, row_words, chain, plan.error_chunks, plan.sampler, division,
                                                             shape.chunks_per_entry, shape.database_columns, first, rows,
                                                             queries, stream));
    }
    return HE_OK;
}

// ---- secretMatrix.multiply(transposing: hint, modulus: p) ---------------------------------------------------------------------
template <typename W>
int secret_times_hint(const he_simple_pir_context* ctx, const client::Plan& plan, const W* secrets, size_t rows, const W* hint,
                      size_t column_size, W* results, uint8_t* ws, hipStream_t stream) {
    const PolyContext& ring = *ctx->ring;
    const heamd::DeviceModulus& m = ring.host_constants()[0];
    uint32_t* codes = reinterpret_cast<uint32_t*>(ws);
    HEAMD_HIP_TRY(heamd::launch_simple_pir_client_pack_codes(secrets, codes, rows, ring.degree(), m.p, stream));
    HEAMD_HIP_TRY(heamd::launch_simple_pir_client_hint_product(codes, rows, hint, column_size, results,
                                                               plan.secret_rows_per_pass, plan.fold_terms, ring.degree(), m.p,
                                                               m.barrett64, stream));
    return HE_OK;
}

// ---- PrecomputedQueries.WithoutIndices.init -----------------------------------------------------------------------------------
// `ws`: [ternary chain | secrets | encrypt_zero's | codes]
template <typename W>
int precompute(const he_simple_pir_context* ctx, const client::Plan& plan, const W* a_eval, const W* hint,
               const uint8_t* secret_seeds, const uint8_t* error_seeds, W* queries, W* results, size_t batch, uint8_t* ws,
               hipStream_t stream) {
    const PolyContext& ring = *ctx->ring;
    const DeviceContext dc = ring.device_context();
    uint32_t* chain = reinterpret_cast<uint32_t*>(ws);
    W* secrets = reinterpret_cast<W*>(ws + plan.secret_chain_bytes);
    uint8_t* rest = ws + plan.secret_chain_bytes + plan.secrets_bytes;
    // generateSecretPolys (SimplePir+Client.swift:21-27): randomizeTernary, one generator per polynomial
    HEAMD_HIP_TRY(heamd::launch_seeded_chain(secret_seeds, chain, plan.rows, heamd::ternary_chunks(ring.degree()), stream));
    HEAMD_HIP_TRY(heamd::launch_sample_ternary(chain, secrets, size_t(ring.degree()), dc, plan.rows, stream));
    HEAMD_TRY_STATUS(encrypt_zero(ctx, plan, a_eval, secrets, error_seeds, queries, batch, rest, stream));
    return secret_times_hint(ctx, plan, secrets, plan.rows, hint, ctx->plan.column_size, results,
                             rest + plan.encrypt_zero_bytes(), stream);
}

int check_device(const he_simple_pir_context* ctx) {
    const PolyContext& ring = *ctx->ring;
    if (ring.host_only()) return heamd::host_only_refusal();
    return ring.check_device();
}

}  // namespace
}  // extern "C++"

int he_simple_pir_client_plan(uint32_t plaintext_bits, uint32_t ciphertext_bits, uint32_t lattice_dimension, uint32_t word_bits,
                              size_t entry_count, size_t entry_size_in_bytes, int error_std_dev, size_t batch,
                              size_t* out_chunk_size, size_t* out_query_words, size_t* out_result_words,
                              uint32_t* out_error_stream_bytes, uint32_t* out_secret_rows_per_pass, uint64_t* out_fold_terms,
                              size_t* out_row_block, size_t* out_hint_product_lds_bytes,
                              size_t* out_a_polynomials_workspace_bytes, size_t* out_encrypt_zero_workspace_bytes,
                              size_t* out_secret_times_hint_workspace_bytes, size_t* out_precompute_workspace_bytes,
                              size_t* out_decrypt_responses_workspace_bytes) {
    SimplePirPlan shape;
    HEAMD_TRY_STATUS(heamd::simple_pir_plan(plaintext_bits, ciphertext_bits, lattice_dimension, word_bits, entry_count,
                                            entry_size_in_bytes, shape));
    client::Plan plan;
    HEAMD_TRY_STATUS(client_plan(shape, error_std_dev, batch, plan));
    if (out_chunk_size != nullptr) *out_chunk_size = plan.chunk_size;
    if (out_query_words != nullptr) *out_query_words = plan.query_words;
    if (out_result_words != nullptr) *out_result_words = plan.result_words;
    if (out_error_stream_bytes != nullptr) *out_error_stream_bytes = plan.sampler.stream_bytes;
    if (out_secret_rows_per_pass != nullptr) *out_secret_rows_per_pass = plan.secret_rows_per_pass;
    if (out_fold_terms != nullptr) *out_fold_terms = plan.fold_terms;
    if (out_row_block != nullptr) *out_row_block = plan.row_block;
    if (out_hint_product_lds_bytes != nullptr) *out_hint_product_lds_bytes = plan.hint_product_lds_bytes;
    if (out_a_polynomials_workspace_bytes != nullptr) *out_a_polynomials_workspace_bytes = plan.a_polynomials_bytes();
    if (out_encrypt_zero_workspace_bytes != nullptr) *out_encrypt_zero_workspace_bytes = plan.encrypt_zero_bytes();
    if (out_secret_times_hint_workspace_bytes != nullptr) *out_secret_times_hint_workspace_bytes = plan.codes_bytes;
    if (out_precompute_workspace_bytes != nullptr) *out_precompute_workspace_bytes = plan.precompute_bytes();
    if (out_decrypt_responses_workspace_bytes != nullptr) *out_decrypt_responses_workspace_bytes = plan.coefficients_bytes;
    return HE_OK;
}

size_t he_simple_pir_client_workspace_bytes(const he_simple_pir_context* ctx, int operation, int error_std_dev, size_t count) {
    if (ctx == nullptr) return 0;
    client::Plan plan;
    // secret x hint takes rows, not queries: its codes depend on nothing else
    if (operation == HE_SIMPLE_PIR_CLIENT_OP_SECRET_TIMES_HINT)
        return client::codes_bytes(ctx->plan.lattice_dimension, count);
    if (client_plan(ctx->plan, error_std_dev, count, plan) != HE_OK) return 0;
    switch (operation) {
        case HE_SIMPLE_PIR_CLIENT_OP_A_POLYNOMIALS:
            return plan.a_polynomials_bytes();
        case HE_SIMPLE_PIR_CLIENT_OP_ENCRYPT_ZERO:
            return plan.encrypt_zero_bytes();
        case HE_SIMPLE_PIR_CLIENT_OP_PRECOMPUTE:
            return plan.precompute_bytes();
        case HE_SIMPLE_PIR_CLIENT_OP_DECRYPT_RESPONSES:
            return plan.coefficients_bytes;
        default:
            return 0;
    }
}

int he_simple_pir_a_polynomials_device(const he_simple_pir_context* ctx, uint32_t word_bits, const uint8_t* seed, void* out,
                                       void* workspace, size_t workspace_bytes, he_stream s) {
    HEAMD_TRY_STATUS(check_word_and_context(ctx, word_bits));
    client::Plan plan;
    HEAMD_TRY_STATUS(client_plan(ctx->plan, client::kStdDev32, 0, plan));
    if (seed == nullptr || out == nullptr) return invalid_argument("null seed or polynomials");
    const size_t out_bytes = ctx->plan.a_poly_count * ctx->plan.lattice_dimension * (word_bits / 8);
    HEAMD_TRY_STATUS(heamd::check_slabs("aPolynomials", {{"out", out, out_bytes, true},
                                                         {"workspace", workspace, workspace_bytes, true},
                                                         {"seed", seed, 32, false}}));
    if (workspace == nullptr || workspace_bytes < plan.a_polynomials_bytes()) return invalid_argument("null or short workspace");
    if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return invalid_argument("workspace not 16-byte aligned");
    if (word_bits == 64 && (reinterpret_cast<uintptr_t>(out) & 7u) != 0) return invalid_argument("misaligned polynomials");
    HEAMD_TRY_STATUS(check_device(ctx));
    uint8_t* ws = static_cast<uint8_t*>(workspace);  // (the seed is the database's: nothing here is secret)
    return heamd::with_word(word_bits, [&](auto word) {
        return a_polynomials(ctx, plan, seed, static_cast<decltype(word)*>(out), ws, as_stream(s));
    });
}

int he_simple_pir_encrypt_zero_device(const he_simple_pir_context* ctx, uint32_t word_bits, int error_std_dev,
                                      const void* a_polynomials, const void* secrets, const uint8_t* error_seeds, void* queries,
                                      size_t batch, void* workspace, size_t workspace_bytes, he_stream s) {
    HEAMD_TRY_STATUS(check_word_and_context(ctx, word_bits));
    client::Plan plan;
    HEAMD_TRY_STATUS(client_plan(ctx->plan, error_std_dev, batch, plan));
    if (batch == 0) return HE_OK;
    if (a_polynomials == nullptr || secrets == nullptr || error_seeds == nullptr || queries == nullptr)
        return invalid_argument("null polynomials, secrets, seeds or queries");
    const size_t word_bytes = word_bits / 8, n = ctx->plan.lattice_dimension;
    HEAMD_TRY_STATUS(heamd::check_slabs("encryptZero", {{"queries", queries, batch * plan.query_words * word_bytes, true},
                                                        {"workspace", workspace, workspace_bytes, true},
                                                        {"a_polynomials", a_polynomials, ctx->plan.a_poly_count * n * word_bytes, false},
                                                        {"secrets", secrets, plan.rows * n * word_bytes, false},
                                                        {"error_seeds", error_seeds, batch * 32, false}}));
    HEAMD_TRY_STATUS(check_device(ctx));
    const hipStream_t stream = as_stream(s);
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(resolve_workspace(ws, workspace, workspace_bytes, plan.encrypt_zero_bytes()));
    return heamd::with_word(word_bits, [&](auto word) {
        using W = decltype(word);
        return encrypt_zero(ctx, plan, static_cast<const W*>(a_polynomials), static_cast<const W*>(secrets), error_seeds,
                            static_cast<W*>(queries), batch, ws.at(0), stream);
    });
}

int he_simple_pir_secret_times_hint_device(const he_simple_pir_context* ctx, uint32_t word_bits, const void* secrets, size_t rows,
                                           const void* hint, size_t column_size, void* results, void* workspace,
                                           size_t workspace_bytes, he_stream s) {
    HEAMD_TRY_STATUS(check_word_and_context(ctx, word_bits));
    if (rows > client::kMaxBatch * ctx->plan.chunks_per_entry) return invalid_argument("too many secret rows for one call");
    client::Plan plan;
    HEAMD_TRY_STATUS(client_plan(ctx->plan, client::kStdDev32, 0, plan));
    if (column_size > (size_t(1) << 40)) return invalid_argument("too many hint rows");
    if (rows == 0 || column_size == 0) return HE_OK;
    if (secrets == nullptr || hint == nullptr || results == nullptr) return invalid_argument("null secrets, hint or results");
    if ((reinterpret_cast<uintptr_t>(hint) & 15u) != 0) return invalid_argument("hint must be 16-byte aligned");
    const size_t word_bytes = word_bits / 8, n = ctx->plan.lattice_dimension;
    HEAMD_TRY_STATUS(heamd::check_slabs("multiply(transposing: hint)",
                                        {{"results", results, rows * column_size * word_bytes, true},
                                         {"workspace", workspace, workspace_bytes, true},
                                         {"secrets", secrets, rows * n * word_bytes, false},
                                         {"hint", hint, column_size * n * word_bytes, false}}));
    HEAMD_TRY_STATUS(check_device(ctx));
    const hipStream_t stream = as_stream(s);
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(resolve_workspace(ws, workspace, workspace_bytes, client::codes_bytes(ctx->plan.lattice_dimension, rows)));
    return heamd::with_word(word_bits, [&](auto word) {
        using W = decltype(word);
        return secret_times_hint(ctx, plan, static_cast<const W*>(secrets), rows, static_cast<const W*>(hint), column_size,
                                 static_cast<W*>(results), ws.at(0), stream);
    });
}

int he_simple_pir_precompute_queries_device(const he_simple_pir_context* ctx, uint32_t word_bits, int error_std_dev,
                                            const void* a_polynomials, const void* hint, const uint8_t* secret_seeds,
                                            const uint8_t* error_seeds, void* queries, void* results_without_response,
                                            size_t batch, void* workspace, size_t workspace_bytes, he_stream s) {
    HEAMD_TRY_STATUS(check_word_and_context(ctx, word_bits));
    client::Plan plan;
    HEAMD_TRY_STATUS(client_plan(ctx->plan, error_std_dev, batch, plan));
    if (batch == 0) return HE_OK;
    if (a_polynomials == nullptr || hint == nullptr || secret_seeds == nullptr || error_seeds == nullptr || queries == nullptr ||
        results_without_response == nullptr)
        return invalid_argument("null polynomials, hint, seeds, queries or results");
    if ((reinterpret_cast<uintptr_t>(hint) & 15u) != 0) return invalid_argument("hint must be 16-byte aligned");
    const size_t word_bytes = word_bits / 8, n = ctx->plan.lattice_dimension;
    HEAMD_TRY_STATUS(heamd::check_slabs(
        "PrecomputedQueries.WithoutIndices", {{"queries", queries, batch * plan.query_words * word_bytes, true},
                                              {"results_without_response", results_without_response,
                                               batch * plan.result_words * word_bytes, true},
                                              {"workspace", workspace, workspace_bytes, true},
                                              {"a_polynomials", a_polynomials, ctx->plan.a_poly_count * n * word_bytes, false},
                                              {"hint", hint, ctx->plan.column_size * n * word_bytes, false},
                                              {"secret_seeds", secret_seeds, plan.rows * 32, false},
                                              {"error_seeds", error_seeds, batch * 32, false}}));
    HEAMD_TRY_STATUS(check_device(ctx));
    const hipStream_t stream = as_stream(s);
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(resolve_workspace(ws, workspace, workspace_bytes, plan.precompute_bytes()));
    return heamd::with_word(word_bits, [&](auto word) {
        using W = decltype(word);
        return precompute(ctx, plan, static_cast<const W*>(a_polynomials), static_cast<const W*>(hint), secret_seeds, error_seeds,
                          static_cast<W*>(queries), static_cast<W*>(results_without_response), batch, ws.at(0), stream);
    });
}

int he_simple_pir_add_indices_device(const he_simple_pir_context* ctx, uint32_t word_bits, void* queries, const uint64_t* indices,
                                     uint32_t* flags, size_t batch, he_stream s) {
    HEAMD_TRY_STATUS(check_word_and_context(ctx, word_bits));
    client::Plan plan;
    HEAMD_TRY_STATUS(client_plan(ctx->plan, client::kStdDev32, batch, plan));
    if (batch == 0) return HE_OK;
    if (queries == nullptr || indices == nullptr) return invalid_argument("null queries or indices");
    HEAMD_TRY_STATUS(heamd::check_slabs("add(index:)", {{"queries", queries, batch * plan.query_words * (word_bits / 8), true},
                                                        {"flags", flags, batch * sizeof(uint32_t), true},
                                                        {"indices", indices, batch * sizeof(uint64_t), false}}));
    HEAMD_TRY_STATUS(check_device(ctx));
    const heamd::SimplePirClientLayout layout = layout_of(ctx->plan, plan);
    return heamd::with_word(word_bits, [&](auto word) {
        HEAMD_HIP_TRY(heamd::launch_simple_pir_client_add_indices(static_cast<decltype(word)*>(queries), indices, flags, layout, batch,
                                                                  as_stream(s)));
        return int(HE_OK);
    });
}

int he_simple_pir_decrypt_responses_device(const he_simple_pir_context* ctx, uint32_t word_bits, const void* responses,
                                           const void* results_without_response, const uint64_t* indices, uint8_t* entries,
                                           uint32_t* flags, size_t batch, void* workspace, size_t workspace_bytes, he_stream s) {
    HEAMD_TRY_STATUS(check_word_and_context(ctx, word_bits));
    client::Plan plan;
    HEAMD_TRY_STATUS(client_plan(ctx->plan, client::kStdDev32, batch, plan));
    if (batch == 0) return HE_OK;
    if (responses == nullptr || results_without_response == nullptr || indices == nullptr || entries == nullptr)
        return invalid_argument("null responses, results, indices or entries");
    const size_t slab_bytes = batch * plan.result_words * (word_bits / 8);
    HEAMD_TRY_STATUS(heamd::check_slabs("decrypt(responses:)", {{"entries", entries, batch * ctx->plan.entry_size_in_bytes, true},
                                                                {"flags", flags, batch * sizeof(uint32_t), true},
                                                                {"workspace", workspace, workspace_bytes, true},
                                                                {"responses", responses, slab_bytes, false},
                                                                {"results_without_response", results_without_response, slab_bytes, false},
                                                                {"indices", indices, batch * sizeof(uint64_t), false}}));
    HEAMD_TRY_STATUS(check_device(ctx));
    const hipStream_t stream = as_stream(s);
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(resolve_workspace(ws, workspace, workspace_bytes, plan.coefficients_bytes));
    const heamd::SimplePirClientLayout layout = layout_of(ctx->plan, plan);
    return heamd::with_word(word_bits, [&](auto word) {
        using W = decltype(word);
        W* coefficients = ws.at<W>(0);
        HEAMD_HIP_TRY(heamd::launch_simple_pir_client_integrate(static_cast<const W*>(responses),
                                                                static_cast<const W*>(results_without_response), indices,
                                                                coefficients, flags, layout, batch, stream));
        HEAMD_HIP_TRY(heamd::launch_simple_pir_client_entry_bytes(coefficients, entries, layout, batch, stream));
        return int(HE_OK);
    });
}
