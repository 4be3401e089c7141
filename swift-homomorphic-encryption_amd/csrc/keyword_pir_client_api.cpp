// keyword_pir_client_api.cpp -- KeywordPirClient (reference Sources/PrivateInformationRetrieval/KeywordPir/
// KeywordPirProtocol.swift:279-392) behind the C ABI: the plan of keyword_pir_client_plan.hpp, generateQuery(at:using:) --
// HashKeyword.hash and .hashIndices (keyword_pir_kernels.hip), then he_pir_generate_query_device -- decrypt(response:at:using:) --
// the same indices, he_pir_decrypt_response_device into bucket rows, then the bucket search of keyword_pir_client_kernels.hip --
// and countEntriesInResponse -- decryptFull, then the scan.  Hashes, indices, bucket rows and records say which keyword a user
// asks for and what it maps to: they lie in a ZeroizedWorkspace, the helper and the rule of encrypt_api.cpp.  The index client's
// checks and plans, its nested workspace included, come from one call into pir_client_layer.hpp per entry; the first checks:
// word_layer.hpp; the parts of a workspace: workspace_layout.hpp.
#include "bfv_context.hpp"
#include "keyword_pir.hpp"
#include "keyword_pir_client_kernels.hpp"
#include "keyword_pir_client_plan.hpp"
#include "launch_grid.hpp"
#include "pir_client_layer.hpp"
#include "word_layer.hpp"
#include "workspace_layout.hpp"
#include "zeroized_workspace.hpp"

using heamd::as_stream;
using heamd::BfvContext;
using heamd::invalid_argument;
using heamd::ZeroizedWorkspace;
namespace plan = heamd::keyword_pir_client;

extern "C++" {
namespace {

constexpr uint64_t kMaxCount = 0xffffffffull;          // keywords of one call, buckets of a table (keyword_pir_api.cpp)
constexpr uint64_t kMaxEntrySize = uint64_t(1) << 48;  // (keyword_pir_api.cpp)
constexpr uint64_t kMaxBytes = uint64_t(1) << 62;      // of one slab: no byte count below wraps

// h serialized HashBuckets of E bytes a query
int check_buckets(uint32_t h, size_t entry_size) {
    if (h == 0) return invalid_argument("no hash function");
    if (h > plan::kMaxHashFunctions) {
        heamd::set_last_error("more than 8 hash functions are not supported");
        return HE_ERR_UNSUPPORTED;
    }
    if (entry_size == 0) return invalid_argument("a serialized HashBucket is not empty");
    if (entry_size > kMaxEntrySize) return invalid_argument("entry size too large");
    return HE_OK;
}

// queries x h rows of E bytes: the rows and the lines of out_values fit one launch each, and the row bytes do not wrap
int check_rows(uint64_t entry_size, uint32_t h, size_t queries) {
    if (queries > kMaxCount || queries * h > heamd::launch_grid::kMaxLanes)
        return invalid_argument("too many queries for one call");
    if (queries != 0 && entry_size > kMaxBytes / (queries * h)) return invalid_argument("too many queries for one call");
    const uint64_t lines = plan::value_capacity(entry_size) / 16 + 2;
    if (queries != 0 && lines > heamd::launch_grid::kMaxLanes / queries) return invalid_argument("too many queries for one call");
    return HE_OK;
}

// What the bucket search adds to the index-PIR parameter of a keyword database (no size prefix, h indices a query), behind the
// index client's errors (pir_client_layer.hpp)
int keyword_plan(const heamd::pir_client::Plan& index, size_t entry_count, size_t entry_size, uint32_t h, plan::Plan& out) {
    HEAMD_TRY_STATUS(check_buckets(h, entry_size));
    if (entry_count == 0 || entry_count > kMaxCount) return invalid_argument("bucket count outside 1 .. 2^32 - 1");
    out = plan::plan(entry_size, index.reply_ciphertexts, index.bytes_per_plaintext);
    return HE_OK;
}

// The plan of a composite entry: the index client's counts, what the bucket search adds, and where the parts of the workspace
// lie, in this order, each where the entry has it: hashes [queries] at 0 | 4-byte indices [queries][h] | 8-byte indices
// [queries][h] (what both directions derive from the keywords) | bucket rows | search records | from `nested` to `total` the
// index client's workspace
struct ClientPlan {
    heamd::pir_client::Plan index;
    plan::Plan keyword;
    size_t narrow = 0, wide = 0, rows = 0, records = 0, nested = 0, total = 0;
};
void add_index_parts(heamd::WorkspaceLayout& layout, size_t queries, uint32_t h, ClientPlan& out) {
    layout.add(queries * sizeof(uint64_t));
    out.narrow = layout.add(queries * h * sizeof(uint32_t));
    out.wide = layout.add(queries * h * sizeof(uint64_t));
}

// HashKeyword.hash (unless the hashes are given) and .hashIndices as the uint64 the MulPIR client reads
int derive_indices(const uint8_t* keywords, const uint64_t* keyword_offsets, const uint64_t* hashes, size_t queries,
                   size_t entry_count, uint32_t h, const ClientPlan& p, const ZeroizedWorkspace& ws, const uint64_t*& out_hashes,
                   uint64_t*& out_indices, hipStream_t stream) {
    uint64_t* own = ws.at<uint64_t>(0);
    uint32_t* narrow = ws.at<uint32_t>(p.narrow);
    out_indices = ws.at<uint64_t>(p.wide);
    if (hashes == nullptr) {
        HEAMD_HIP_TRY(heamd::launch_keyword_hash(keywords, keyword_offsets, queries, own, stream));
        hashes = own;
    }
    out_hashes = hashes;
    HEAMD_HIP_TRY(heamd::launch_keyword_hash_indices(hashes, queries, entry_count, h, narrow, stream));
    HEAMD_HIP_TRY(heamd::launch_keyword_client_widen_indices(narrow, out_indices, queries * h, stream));
    return HE_OK;
}

// ---- generateQuery ----------------------------------------------------------------------------------------------------------------
int plan_query(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions, uint32_t dimension_count,
               size_t entry_count, size_t entry_size, uint32_t h, size_t queries, ClientPlan& out) {
    // every check of he_pir_generate_query_device in front of its buffers (its batch refusal and HE_ERR_NOT_INVERTIBLE included)
    heamd::pir_client::QueryPlan pir;
    HEAMD_TRY_STATUS(heamd::pir_client::plan_query(ctx, word_bits, dimensions, dimension_count, entry_count, entry_size, 0, h,
                                                   queries, pir));
    out.index = pir.client;
    HEAMD_TRY_STATUS(keyword_plan(out.index, entry_count, entry_size, h, out.keyword));
    if (queries > kMaxCount) return invalid_argument("too many queries for one call");
    heamd::WorkspaceLayout layout;
    add_index_parts(layout, queries, h, out);
    out.nested = layout.add(pir.total);
    out.total = layout.total();
    return HE_OK;
}

// ---- decrypt(response:) and countEntriesInResponse ---------------------------------------------------------------------------
int plan_response(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions, uint32_t dimension_count,
                  size_t entry_count, size_t entry_size, uint32_t h, uint32_t moduli_count, bool count_only, size_t queries,
                  ClientPlan& out) {
    heamd::pir_client::ResponsePlan pir;  // (the count's nested call is decryptFull)
    HEAMD_TRY_STATUS(heamd::pir_client::plan_response(ctx, word_bits, dimensions, dimension_count, entry_count, entry_size, 0, h,
                                                      moduli_count, count_only, queries, pir));
    out.index = pir.client;
    HEAMD_TRY_STATUS(keyword_plan(out.index, entry_count, entry_size, h, out.keyword));
    HEAMD_TRY_STATUS(check_rows(count_only ? out.keyword.reply_bytes : entry_size, h, queries));
    heamd::WorkspaceLayout layout;
    if (!count_only) add_index_parts(layout, queries, h, out);
    out.rows = layout.add(queries * h * (count_only ? out.keyword.reply_bytes : entry_size));
    if (!count_only) out.records = layout.add(queries * h * plan::kRecordBytes);
    out.nested = layout.add(pir.total);
    out.total = layout.total();
    return HE_OK;
}

int check_find_form(int form, size_t entry_size, plan::FindForm& out) {
    if (form < HE_KEYWORD_PIR_FIND_FORM_PLAN || form > HE_KEYWORD_PIR_FIND_FORM_DIRECT) return invalid_argument("unknown form");
    if (form == HE_KEYWORD_PIR_FIND_FORM_STAGED && entry_size > plan::kStagedRowLimit)
        return invalid_argument("the row is too long for the staged form");
    out = form == HE_KEYWORD_PIR_FIND_FORM_PLAN ? plan::find_form(entry_size)
                                                : (form == HE_KEYWORD_PIR_FIND_FORM_STAGED ? plan::kFindStaged : plan::kFindDirect);
    return HE_OK;
}

int check_find_shape(size_t entry_size, uint32_t h, size_t queries, int form, plan::FindForm& out) {
    HEAMD_TRY_STATUS(check_buckets(h, entry_size));
    HEAMD_TRY_STATUS(check_find_form(form, entry_size, out));
    return check_rows(entry_size, h, queries);
}

}  // namespace
}  // extern "C++"

int he_keyword_client_plan(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count, size_t entry_count,
                               size_t entry_size_in_bytes, uint32_t hash_function_count, size_t* out_expanded_query_count,
                               size_t* out_query_ciphertext_count, size_t* out_reply_ciphertext_count,
                               size_t* out_entries_per_plaintext, size_t* out_bytes_per_plaintext, size_t* out_value_capacity,
                               int* out_find_form, size_t* out_staged_lds_bytes, size_t* out_reply_bytes) {
    heamd::pir_client::Plan p;
    HEAMD_TRY_STATUS(heamd::pir_client::client_plan(ctx, dimensions, dimension_count, entry_count, entry_size_in_bytes, 0,
                                                    hash_function_count, p));
    plan::Plan keyword;
    HEAMD_TRY_STATUS(keyword_plan(p, entry_count, entry_size_in_bytes, hash_function_count, keyword));
    if (out_expanded_query_count != nullptr) *out_expanded_query_count = p.expanded_query_count;
    if (out_query_ciphertext_count != nullptr) *out_query_ciphertext_count = p.query_ciphertexts;
    if (out_reply_ciphertext_count != nullptr) *out_reply_ciphertext_count = p.reply_ciphertexts;
    if (out_entries_per_plaintext != nullptr) *out_entries_per_plaintext = p.entries_per_plaintext;
    if (out_bytes_per_plaintext != nullptr) *out_bytes_per_plaintext = p.bytes_per_plaintext;
    if (out_value_capacity != nullptr) *out_value_capacity = keyword.value_capacity;
    if (out_find_form != nullptr)
        *out_find_form = keyword.form == plan::kFindStaged ? HE_KEYWORD_PIR_FIND_FORM_STAGED : HE_KEYWORD_PIR_FIND_FORM_DIRECT;
    if (out_staged_lds_bytes != nullptr) *out_staged_lds_bytes = keyword.lds_bytes;
    if (out_reply_bytes != nullptr) *out_reply_bytes = keyword.reply_bytes;
    return HE_OK;
}

size_t he_keyword_client_generate_query_workspace_bytes(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                                     uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                                     uint32_t hash_function_count, size_t queries) {
    ClientPlan p;
    const int status = plan_query(ctx, word_bits, dimensions, dimension_count, entry_count, entry_size_in_bytes, hash_function_count,
                                  queries, p);
    return status == HE_OK ? p.total : 0;
}

int he_keyword_client_generate_query_device(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                         uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                         uint32_t hash_function_count, const uint8_t* keywords, const uint64_t* keyword_offsets,
                                         size_t queries, const void* secret_key, const uint8_t* a_seeds, const uint8_t* error_seeds,
                                         void* out, uint64_t* out_hashes, void* workspace, size_t workspace_bytes, he_stream s) {
    ClientPlan p;
    HEAMD_TRY_STATUS(plan_query(ctx, word_bits, dimensions, dimension_count, entry_count, entry_size_in_bytes, hash_function_count,
                                queries, p));
    if (queries == 0) return HE_OK;
    if (keywords == nullptr || keyword_offsets == nullptr || secret_key == nullptr || a_seeds == nullptr || error_seeds == nullptr ||
        out == nullptr)
        return invalid_argument("null keywords, offsets, secret key, seeds or ciphertexts");
    const BfvContext& bfv = heamd::bfv_impl(ctx);
    const size_t count = queries * p.index.query_ciphertexts, row_bytes = size_t(bfv.degree()) * (word_bits / 8);
    // (the keyword blob's length lies on the device: of `keywords` only the first byte takes part)
    HEAMD_TRY_STATUS(heamd::check_slabs("keyword generateQuery",
                                        {{"out", out, count * 2 * bfv.top_level() * row_bytes, true},
                                         {"out_hashes", out_hashes, queries * sizeof(uint64_t), true},
                                         {"workspace", workspace, workspace_bytes, true},
                                         {"keywords", keywords, 1, false},
                                         {"keyword_offsets", keyword_offsets, (queries + 1) * sizeof(uint64_t), false},
                                         {"secret_key", secret_key, bfv.top_level() * row_bytes, false},
                                         {"a_seeds", a_seeds, count * 32, false},
                                         {"error_seeds", error_seeds, count * 32, false}}));
    HEAMD_TRY_STATUS(heamd::bfv_encrypt_check_device(ctx, word_bits, bfv.top_level()));
    hipStream_t stream = as_stream(s);
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(ws.resolve(workspace, workspace_bytes, p.total));
    const uint64_t* hashes = nullptr;
    uint64_t* indices = nullptr;
    HEAMD_TRY_STATUS(derive_indices(keywords, keyword_offsets, nullptr, queries, entry_count, hash_function_count, p, ws, hashes,
                                    indices, stream));
    if (out_hashes != nullptr)
        HEAMD_HIP_TRY(hipMemcpyAsync(out_hashes, hashes, queries * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
    // indexPirClient.generateQuery(at: indices, using: secretKey) (:333); hashIndices stays below entry_count: no flag
    return he_pir_generate_query_device(ctx, word_bits, dimensions, dimension_count, entry_count, entry_size_in_bytes, 0,
                                        hash_function_count, indices, queries, secret_key, a_seeds, error_seeds, out, nullptr,
                                        ws.at(p.nested), p.total - p.nested, s);
}

size_t he_keyword_client_find_in_buckets_workspace_bytes(size_t entry_size_in_bytes, uint32_t hash_function_count, size_t queries) {
    plan::FindForm form;
    if (check_find_shape(entry_size_in_bytes, hash_function_count, queries, HE_KEYWORD_PIR_FIND_FORM_PLAN, form) != HE_OK) return 0;
    return heamd::round16(queries * hash_function_count * plan::kRecordBytes);
}

int he_keyword_client_find_in_buckets_device(const uint8_t* buckets, const uint64_t* hashes, size_t entry_size_in_bytes,
                                          uint32_t hash_function_count, size_t queries, int form, uint8_t* out_values,
                                          uint64_t* out_sizes, uint32_t* out_status, void* workspace, size_t workspace_bytes,
                                          he_stream s) {
    plan::FindForm chosen;
    HEAMD_TRY_STATUS(check_find_shape(entry_size_in_bytes, hash_function_count, queries, form, chosen));
    if (queries == 0) return HE_OK;
    const size_t capacity = plan::value_capacity(entry_size_in_bytes);
    if (buckets == nullptr || hashes == nullptr || out_sizes == nullptr || out_status == nullptr ||
        (out_values == nullptr && capacity != 0))
        return invalid_argument("null buckets, hashes, values, sizes or status");
    HEAMD_TRY_STATUS(heamd::check_slabs("find(hash:)",
                                        {{"out_values", out_values, queries * capacity, true},
                                         {"out_sizes", out_sizes, queries * sizeof(uint64_t), true},
                                         {"out_status", out_status, queries * sizeof(uint32_t), true},
                                         {"workspace", workspace, workspace_bytes, true},
                                         {"buckets", buckets, queries * hash_function_count * entry_size_in_bytes, false},
                                         {"hashes", hashes, queries * sizeof(uint64_t), false}}));
    hipStream_t stream = as_stream(s);
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(ws.resolve(workspace, workspace_bytes, heamd::round16(queries * hash_function_count * plan::kRecordBytes)));
    HEAMD_HIP_TRY(heamd::launch_keyword_client_find(buckets, hashes, entry_size_in_bytes, hash_function_count, queries, chosen,
                                                    ws.at(0), out_values, out_sizes, out_status, stream));
    return HE_OK;
}

size_t he_keyword_client_decrypt_response_workspace_bytes(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                                       uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                                       uint32_t hash_function_count, uint32_t moduli_count, size_t queries) {
    ClientPlan p;
    const int status = plan_response(ctx, word_bits, dimensions, dimension_count, entry_count, entry_size_in_bytes,
                                     hash_function_count, moduli_count, false, queries, p);
    return status == HE_OK ? p.total : 0;
}

int he_keyword_client_decrypt_response_device(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                           uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                           uint32_t hash_function_count, uint32_t moduli_count, const void* response,
                                           const uint8_t* keywords, const uint64_t* keyword_offsets, const uint64_t* hashes,
                                           size_t queries, const void* secret_key, uint8_t* out_values, uint64_t* out_sizes,
                                           uint32_t* out_status, void* workspace, size_t workspace_bytes, he_stream s) {
    ClientPlan p;
    HEAMD_TRY_STATUS(plan_response(ctx, word_bits, dimensions, dimension_count, entry_count, entry_size_in_bytes, hash_function_count,
                                   moduli_count, false, queries, p));
    if (queries == 0) return HE_OK;
    const size_t capacity = p.keyword.value_capacity;
    if (response == nullptr || secret_key == nullptr || out_sizes == nullptr || out_status == nullptr ||
        (out_values == nullptr && capacity != 0) || (keywords == nullptr ? hashes == nullptr : keyword_offsets == nullptr))
        return invalid_argument("null response, keywords or hashes, secret key, values, sizes or status");
    if (keywords != nullptr) hashes = nullptr;  // the keywords are hashed
    const BfvContext& bfv = heamd::bfv_impl(ctx);
    const size_t replies = queries * hash_function_count * p.index.reply_ciphertexts;
    const size_t row_bytes = size_t(bfv.degree()) * (word_bits / 8);
    HEAMD_TRY_STATUS(heamd::check_slabs("keyword decrypt(response:)",
                                        {{"out_values", out_values, queries * capacity, true},
                                         {"out_sizes", out_sizes, queries * sizeof(uint64_t), true},
                                         {"out_status", out_status, queries * sizeof(uint32_t), true},
                                         {"workspace", workspace, workspace_bytes, true},
                                         {"response", response, replies * 2 * moduli_count * row_bytes, false},
                                         {"keywords", keywords, 1, false},
                                         {"keyword_offsets", keywords != nullptr ? keyword_offsets : nullptr,
                                          (queries + 1) * sizeof(uint64_t), false},
                                         {"hashes", hashes, queries * sizeof(uint64_t), false},
                                         {"secret_key", secret_key, moduli_count * row_bytes, false}}));
    HEAMD_TRY_STATUS(heamd::bfv_decrypt_check_device(ctx, word_bits, moduli_count));
    hipStream_t stream = as_stream(s);
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(ws.resolve(workspace, workspace_bytes, p.total));
    const uint64_t* keys = nullptr;
    uint64_t* indices = nullptr;
    HEAMD_TRY_STATUS(derive_indices(keywords, keyword_offsets, hashes, queries, entry_count, hash_function_count, p, ws, keys,
                                    indices, stream));
    uint8_t* rows = ws.at(p.rows);
    // indexPirClient.decrypt(response:at:using:) (:351): the serialized buckets [queries][h][E]; no prefix, so no sizes
    HEAMD_TRY_STATUS(he_pir_decrypt_response_device(ctx, word_bits, dimensions, dimension_count, entry_count, entry_size_in_bytes, 0,
                                                    hash_function_count, moduli_count, response, indices, queries, secret_key, rows,
                                                    nullptr, ws.at(p.nested), p.total - p.nested, s));
    HEAMD_HIP_TRY(heamd::launch_keyword_client_find(rows, keys, entry_size_in_bytes, hash_function_count, queries,
                                                    p.keyword.form, ws.at(p.records), out_values, out_sizes, out_status,
                                                    stream));
    return HE_OK;
}

size_t he_keyword_client_count_entries_workspace_bytes(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                                    uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                                    uint32_t hash_function_count, uint32_t moduli_count, size_t queries) {
    ClientPlan p;
    const int status = plan_response(ctx, word_bits, dimensions, dimension_count, entry_count, entry_size_in_bytes,
                                     hash_function_count, moduli_count, true, queries, p);
    return status == HE_OK ? p.total : 0;
}

int he_keyword_client_count_entries_device(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                        uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                        uint32_t hash_function_count, uint32_t moduli_count, const void* response, size_t queries,
                                        const void* secret_key, uint64_t* out_counts, void* workspace, size_t workspace_bytes,
                                        he_stream s) {
    ClientPlan p;
    HEAMD_TRY_STATUS(plan_response(ctx, word_bits, dimensions, dimension_count, entry_count, entry_size_in_bytes, hash_function_count,
                                   moduli_count, true, queries, p));
    if (queries == 0) return HE_OK;
    if (response == nullptr || secret_key == nullptr || out_counts == nullptr)
        return invalid_argument("null response, secret key or counts");
    const BfvContext& bfv = heamd::bfv_impl(ctx);
    const size_t replies = queries * hash_function_count * p.index.reply_ciphertexts;
    const size_t row_bytes = size_t(bfv.degree()) * (word_bits / 8);
    HEAMD_TRY_STATUS(heamd::check_slabs("countEntriesInResponse",
                                        {{"out_counts", out_counts, queries * sizeof(uint64_t), true},
                                         {"workspace", workspace, workspace_bytes, true},
                                         {"response", response, replies * 2 * moduli_count * row_bytes, false},
                                         {"secret_key", secret_key, moduli_count * row_bytes, false}}));
    HEAMD_TRY_STATUS(heamd::bfv_decrypt_check_device(ctx, word_bits, moduli_count));
    hipStream_t stream = as_stream(s);
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(ws.resolve(workspace, workspace_bytes, p.total));
    // indexPirClient.decryptFull(response:using:) (:378): [queries][h][R bpp]
    HEAMD_TRY_STATUS(he_pir_decrypt_response_device(ctx, word_bits, dimensions, dimension_count, entry_count, entry_size_in_bytes, 0,
                                                    hash_function_count, moduli_count, response, nullptr, queries, secret_key,
                                                    ws.at(p.rows), nullptr, ws.at(p.nested), p.total - p.nested, s));
    HEAMD_HIP_TRY(heamd::launch_keyword_client_count(ws.at(p.rows), p.keyword.reply_bytes, hash_function_count, queries, out_counts,
                                                     stream));
    return HE_OK;
}

int he_keyword_client_count_bucket_entries_device(const uint8_t* bytes, size_t reply_bytes, size_t replies_per_query, size_t queries,
                                               uint64_t* out_counts, he_stream s) {
    if (queries > kMaxCount || replies_per_query > kMaxCount || reply_bytes > kMaxEntrySize)
        return invalid_argument("too many queries, replies or bytes for one call");
    if (queries == 0) return HE_OK;
    if (replies_per_query != 0 && reply_bytes > kMaxBytes / (queries * replies_per_query))
        return invalid_argument("too many queries, replies or bytes for one call");
    const size_t total = queries * replies_per_query * reply_bytes;
    if (out_counts == nullptr || (bytes == nullptr && total != 0)) return invalid_argument("null bytes or counts");
    HEAMD_TRY_STATUS(heamd::check_slabs("count entries", {{"out_counts", out_counts, queries * sizeof(uint64_t), true},
                                                          {"bytes", bytes, total, false}}));
    HEAMD_HIP_TRY(heamd::launch_keyword_client_count(bytes, reply_bytes, replies_per_query, queries, out_counts, as_stream(s)));
    return HE_OK;
}
