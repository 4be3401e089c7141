// pir_client_api.cpp -- the MulPIR client (reference Sources/PrivateInformationRetrieval/IndexPir/MulPir.swift:117-289) behind
// the C ABI: the host plans of pir_client_plan.hpp, MulPirClient.generateQuery(at:using:) -- the selection plaintexts of
// PirUtil.compressBinaryInputs (pir_client_kernels.hip), then he_bfv_encrypt_device -- and MulPirClient.decrypt(response:at:
// using:) / decryptFull -- he_bfv_decrypt_device, then coefficientsToBytes and the entry extraction in one kernel.
// Whatever a call parks in memory between its kernels says which entries a user asks for or what they hold: it lies in a
// ZeroizedWorkspace, the helper and the rule of encrypt_api.cpp.  The first checks and the word dispatch: word_layer.hpp; the parts
// of a workspace: workspace_layout.hpp; the checks and plans the keyword client builds on: pir_client_layer.hpp, defined here.
#include "bfv_context.hpp"
#include "launch_grid.hpp"
#include "pir_client_kernels.hpp"
#include "pir_client_layer.hpp"
#include "word_layer.hpp"
#include "workspace_layout.hpp"
#include "zeroized_workspace.hpp"

using heamd::as_stream;
using heamd::BfvContext;
using heamd::check_word_and_context;
using heamd::invalid_argument;
using heamd::ZeroizedWorkspace;
using namespace heamd::pir_client;

extern "C++" {
namespace {

constexpr uint64_t kMaxIndices = uint64_t(1) << 20;  // indices of a query (S I stays far below 2^64)

// queries x per_query items of `lanes_each` lanes: one launch holds them, and no byte count below wraps
int check_batch(size_t queries, uint64_t per_query, uint64_t lanes_each) {
    const uint64_t limit = heamd::launch_grid::kMaxLanes;
    if (per_query > limit || lanes_each > limit || per_query * lanes_each > limit || queries > limit / (per_query * lanes_each))
        return invalid_argument("too many queries for one call");
    return HE_OK;
}

// ---- generateQuery ----------------------------------------------------------------------------------------------------------------
template <typename W>
int generate_query(const he_bfv_context* ctx, const QueryPlan& plan, const uint64_t* indices, size_t queries,
                   const void* secret_key, const uint8_t* a_seeds, const uint8_t* error_seeds, void* out, uint32_t* out_of_range,
                   void* workspace, size_t workspace_bytes, he_stream s) {
    hipStream_t stream = as_stream(s);
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(ws.resolve(workspace, workspace_bytes, plan.total));
    W* plaintexts = ws.at<W>(0);
    HEAMD_HIP_TRY(heamd::launch_pir_selection_plaintexts(indices, plan.client, queries, plan.first, plan.last, plaintexts,
                                                         out_of_range, stream));
    // plaintexts.map { try $0.encrypt(using: secretKey) } (PirUtil.swift:403): Coeff at the top level
    return he_bfv_encrypt_device(ctx, 8 * sizeof(W), heamd::bfv_impl(ctx).top_level(), secret_key, a_seeds, error_seeds, plaintexts,
                                 out, queries * plan.client.query_ciphertexts, ws.at(plan.nested), plan.total - plan.nested, s);
}

// ---- decrypt(response:) -----------------------------------------------------------------------------------------------------------
template <typename W>
int decrypt_response(const he_bfv_context* ctx, const ResponsePlan& plan, uint32_t moduli_count, const void* response,
                     const uint64_t* indices, size_t queries, const void* secret_key, uint8_t* out_entries, uint64_t* out_sizes,
                     void* workspace, size_t workspace_bytes, he_stream s) {
    hipStream_t stream = as_stream(s);
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(ws.resolve(workspace, workspace_bytes, plan.total));
    W* plaintexts = ws.at<W>(0);  // [queries][I][R][N]
    // ciphertext.decrypt(using:) and decode(format: .coefficient) (MulPir.swift:257-258)
    HEAMD_TRY_STATUS(he_bfv_decrypt_device(ctx, 8 * sizeof(W), moduli_count, 2, 0, response, secret_key, 1, plaintexts, plan.replies,
                                           ws.at(plan.nested), plan.total - plan.nested, s));
    HEAMD_HIP_TRY(heamd::launch_pir_reply_entries(plaintexts, indices, plan.client, queries, out_entries, out_sizes, stream));
    return HE_OK;
}

}  // namespace

// ---- pir_client_layer.hpp ---------------------------------------------------------------------------------------------------------
// he_pir_database_shape's errors, then the client's own
int heamd::pir_client::client_plan(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count,
                                   size_t entry_count, size_t entry_size_in_bytes, int encoding_entry_size, size_t indices_count,
                                   Plan& plan) {
    HEAMD_TRY_STATUS(he_pir_database_shape(ctx, dimensions, dimension_count, entry_count, entry_size_in_bytes, encoding_entry_size,
                                           nullptr, nullptr, nullptr, nullptr, nullptr));
    if (indices_count == 0) return invalid_argument("a query has at least one index");
    if (indices_count > kMaxIndices) return invalid_argument("too many indices");
    if (dimension_count > kMaxDimensions) {
        heamd::set_last_error("the client takes at most 16 dimensions");
        return HE_ERR_UNSUPPORTED;
    }
    const BfvContext& bfv = heamd::bfv_impl(ctx);
    plan = heamd::pir_client::plan(bfv.degree(), bfv.plaintext_modulus(), dimensions, dimension_count, entry_count,
                                   entry_size_in_bytes, encoding_entry_size != 0, indices_count);
    if (plan.bytes_per_plaintext * 8 != plan.degree * plan.bits) return invalid_argument("plaintexts hold no whole bytes");
    return HE_OK;
}

int heamd::pir_client::plan_query(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                  uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes, int encoding_entry_size,
                                  size_t indices_count, size_t queries, QueryPlan& plan) {
    HEAMD_TRY_STATUS(check_word_and_context(ctx, word_bits));
    HEAMD_TRY_STATUS(client_plan(ctx, dimensions, dimension_count, entry_count, entry_size_in_bytes, encoding_entry_size,
                                 indices_count, plan.client));
    const Plan& p = plan.client;
    HEAMD_TRY_STATUS(check_batch(queries, p.query_ciphertexts, p.degree));
    const BfvContext& bfv = heamd::bfv_impl(ctx);
    const heamd::u64 t = bfv.plaintext_modulus();
    if (!selection_value(input_count(p, 0), t, plan.first) ||
        !selection_value(input_count(p, p.query_ciphertexts - 1), t, plan.last)) {
        heamd::set_last_error("the input count's power of two has no inverse mod t");
        return HE_ERR_NOT_INVERTIBLE;
    }
    const size_t count = queries * p.query_ciphertexts;
    heamd::WorkspaceLayout layout;
    layout.add(count * p.degree * (word_bits / 8));
    plan.nested = layout.add(he_bfv_encrypt_workspace_bytes(ctx, word_bits, HE_ENCRYPT_OP_ENCRYPT, bfv.top_level(), 0, count));
    plan.total = layout.total();
    return HE_OK;
}

int heamd::pir_client::plan_response(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                     uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                     int encoding_entry_size, size_t indices_count, uint32_t moduli_count, bool full, size_t queries,
                                     ResponsePlan& plan) {
    HEAMD_TRY_STATUS(check_word_and_context(ctx, word_bits));
    HEAMD_TRY_STATUS(client_plan(ctx, dimensions, dimension_count, entry_count, entry_size_in_bytes, encoding_entry_size,
                                 indices_count, plan.client));
    const Plan& p = plan.client;
    if (!heamd::bfv_impl(ctx).valid(moduli_count)) return invalid_argument("moduli_count out of range");
    HEAMD_TRY_STATUS(check_batch(queries, p.indices_count * p.reply_ciphertexts, p.degree));
    plan.out_stride = full ? p.reply_ciphertexts * p.bytes_per_plaintext : p.entry_size;
    HEAMD_TRY_STATUS(check_batch(queries, p.indices_count, plan.out_stride ? plan.out_stride : 1));
    plan.replies = queries * p.indices_count * p.reply_ciphertexts;
    heamd::WorkspaceLayout layout;
    layout.add(plan.replies * p.degree * (word_bits / 8));
    plan.nested = layout.add(he_bfv_decrypt_workspace_bytes(ctx, word_bits, moduli_count, 2, 0, plan.replies));
    plan.total = layout.total();
    return HE_OK;
}
}  // extern "C++"

int he_pir_client_plan(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count, size_t entry_count,
                       size_t entry_size_in_bytes, int encoding_entry_size, size_t indices_count, size_t* out_expanded_query_count,
                       size_t* out_query_ciphertext_count, size_t* out_reply_ciphertext_count, size_t* out_entries_per_plaintext,
                       size_t* out_bytes_per_plaintext, size_t* out_entry_size_encoding_width) {
    Plan plan;
    HEAMD_TRY_STATUS(client_plan(ctx, dimensions, dimension_count, entry_count, entry_size_in_bytes, encoding_entry_size,
                                 indices_count, plan));
    if (out_expanded_query_count != nullptr) *out_expanded_query_count = plan.expanded_query_count;
    if (out_query_ciphertext_count != nullptr) *out_query_ciphertext_count = plan.query_ciphertexts;
    if (out_reply_ciphertext_count != nullptr) *out_reply_ciphertext_count = plan.reply_ciphertexts;
    if (out_entries_per_plaintext != nullptr) *out_entries_per_plaintext = plan.entries_per_plaintext;
    if (out_bytes_per_plaintext != nullptr) *out_bytes_per_plaintext = plan.bytes_per_plaintext;
    if (out_entry_size_encoding_width != nullptr) *out_entry_size_encoding_width = plan.width;
    return HE_OK;
}

int he_pir_evaluation_key_elements(uint32_t degree, size_t expanded_query_count, int key_compression, uint64_t* out_elements,
                                   size_t capacity, size_t* out_count) {
    if (degree < 2 || (degree & (degree - 1)) != 0) return invalid_argument("degree must be a power of two");
    if (expanded_query_count == 0) return invalid_argument("expanded_query_count must be positive");
    if (key_compression < HE_PIR_KEY_COMPRESSION_NONE || key_compression > HE_PIR_KEY_COMPRESSION_MAX)
        return invalid_argument("unknown key compression strategy");
    const std::vector<uint64_t> elements = heamd::pir_client::evaluation_key_elements(degree, expanded_query_count, key_compression);
    if (out_count != nullptr) *out_count = elements.size();
    if (out_elements != nullptr) {
        if (capacity < elements.size()) return invalid_argument("out_elements too small");
        for (size_t i = 0; i < elements.size(); ++i) out_elements[i] = elements[i];
    }
    return HE_OK;
}

size_t he_pir_generate_query_workspace_bytes(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                             uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                             int encoding_entry_size, size_t indices_count, size_t queries) {
    QueryPlan plan;
    const int status = plan_query(ctx, word_bits, dimensions, dimension_count, entry_count, entry_size_in_bytes, encoding_entry_size,
                                  indices_count, queries, plan);
    return status == HE_OK ? plan.total : 0;
}

int he_pir_generate_query_device(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                 uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes, int encoding_entry_size,
                                 size_t indices_count, const uint64_t* indices, size_t queries, const void* secret_key,
                                 const uint8_t* a_seeds, const uint8_t* error_seeds, void* out, uint32_t* out_of_range,
                                 void* workspace, size_t workspace_bytes, he_stream s) {
    QueryPlan plan;
    HEAMD_TRY_STATUS(plan_query(ctx, word_bits, dimensions, dimension_count, entry_count, entry_size_in_bytes, encoding_entry_size,
                                indices_count, queries, plan));
    if (queries == 0) return HE_OK;
    if (indices == nullptr || secret_key == nullptr || a_seeds == nullptr || error_seeds == nullptr || out == nullptr)
        return invalid_argument("null indices, secret key, seeds or ciphertexts");
    const BfvContext& bfv = heamd::bfv_impl(ctx);
    const size_t count = queries * plan.client.query_ciphertexts, row_bytes = size_t(bfv.degree()) * (word_bits / 8);
    HEAMD_TRY_STATUS(heamd::check_slabs("generateQuery", {{"out", out, count * 2 * bfv.top_level() * row_bytes, true},
                                                          {"workspace", workspace, workspace_bytes, true},
                                                          {"out_of_range", out_of_range, sizeof(uint32_t), true},
                                                          {"indices", indices, queries * indices_count * sizeof(uint64_t), false},
                                                          {"secret_key", secret_key, bfv.top_level() * row_bytes, false},
                                                          {"a_seeds", a_seeds, count * 32, false},
                                                          {"error_seeds", error_seeds, count * 32, false}}));
    HEAMD_TRY_STATUS(heamd::bfv_encrypt_check_device(ctx, word_bits, bfv.top_level()));
    return heamd::with_word(word_bits, [&](auto word) {
        return generate_query<decltype(word)>(ctx, plan, indices, queries, secret_key, a_seeds, error_seeds, out, out_of_range,
                                              workspace, workspace_bytes, s);
    });
}

size_t he_pir_decrypt_response_workspace_bytes(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                               uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                               int encoding_entry_size, size_t indices_count, uint32_t moduli_count,
                                               size_t queries) {
    ResponsePlan plan;
    const int status = plan_response(ctx, word_bits, dimensions, dimension_count, entry_count, entry_size_in_bytes,
                                     encoding_entry_size, indices_count, moduli_count, false, queries, plan);
    return status == HE_OK ? plan.total : 0;
}

int he_pir_decrypt_response_device(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                   uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                   int encoding_entry_size, size_t indices_count, uint32_t moduli_count, const void* response,
                                   const uint64_t* indices, size_t queries, const void* secret_key, uint8_t* out_entries,
                                   uint64_t* out_sizes, void* workspace, size_t workspace_bytes, he_stream s) {
    ResponsePlan plan;
    HEAMD_TRY_STATUS(plan_response(ctx, word_bits, dimensions, dimension_count, entry_count, entry_size_in_bytes,
                                   encoding_entry_size, indices_count, moduli_count, indices == nullptr, queries, plan));
    if (queries == 0) return HE_OK;
    const bool needs_sizes = indices != nullptr && plan.client.width != 0;
    if (response == nullptr || secret_key == nullptr || (out_entries == nullptr && plan.out_stride != 0) ||
        (out_sizes == nullptr && needs_sizes))
        return invalid_argument("null response, secret key, entries or sizes");
    const BfvContext& bfv = heamd::bfv_impl(ctx);
    const size_t entries = queries * indices_count, row_bytes = size_t(bfv.degree()) * (word_bits / 8);
    HEAMD_TRY_STATUS(heamd::check_slabs("decrypt(response:)", {{"out_entries", out_entries, entries * plan.out_stride, true},
                                                               {"out_sizes", out_sizes, entries * sizeof(uint64_t), true},
                                                               {"workspace", workspace, workspace_bytes, true},
                                                               {"response", response, plan.replies * 2 * moduli_count * row_bytes, false},
                                                               {"indices", indices, entries * sizeof(uint64_t), false},
                                                               {"secret_key", secret_key, moduli_count * row_bytes, false}}));
    HEAMD_TRY_STATUS(heamd::bfv_decrypt_check_device(ctx, word_bits, moduli_count));
    return heamd::with_word(word_bits, [&](auto word) {
        return decrypt_response<decltype(word)>(ctx, plan, moduli_count, response, indices, queries, secret_key, out_entries,
                                                out_sizes, workspace, workspace_bytes, s);
    });
}
