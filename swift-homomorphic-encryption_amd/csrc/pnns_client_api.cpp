// pnns_client_api.cpp -- the PNNS client (reference Sources/PrivateNearestNeighborSearch/Client.swift:74-127) behind the C ABI,
// in three layers over the kernels of pnns_client_kernels.hip and the transforms over [t]:
//   1  Context.encodeSimd / decodeSimd (Encoding.swift:222-245) for batches of plaintexts;
//   2  PlaintextMatrix(packing: .denseRow, signedValues:reduce:) and PlaintextMatrix.unpack() for .denseColumn and .denseRow
//      (PlaintextMatrix.swift:165-236, 341-406, 489-590);
//   3  Client.generateQuery(for:using:) -- normalizedScaledAndRounded, layer 2 per plaintext modulus, he_bfv_encrypt_device -- and
//      Client.decrypt(response:using:) -- he_bfv_decrypt_device and forwardNtt per plaintext modulus, then one kernel that gathers,
//      composes (CrtComposer.swift:76-97), centres and scales every distance.
// Whatever a call parks in memory between its kernels is the user's query or the distances in the clear: it lies in a
// ZeroizedWorkspace, the helper and the rule of encrypt_api.cpp.  The word check, the word dispatch and the named device checks of
// the nested entries: word_layer.hpp; the parts of a workspace: workspace_layout.hpp.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "api_internal.hpp"
#include "bfv_context.hpp"
#include "host_math.hpp"
#include "kernels.hpp"
#include "pnns_context.hpp"
#include "word_layer.hpp"
#include "workspace_layout.hpp"
#include "zeroized_workspace.hpp"

using heamd::as_stream;
using heamd::BfvContext;
using heamd::invalid_argument;
using heamd::MatrixPlan;
using heamd::PolyContext;
using heamd::ZeroizedWorkspace;

extern "C++" {
namespace {

// the checks every entry of one context makes first, in this order: the word, the context, the word against the context's kind
int check_word_and_context(const he_pnns_context* ctx, uint32_t word_bits) {
    HEAMD_TRY_STATUS(heamd::check_word_bits(word_bits));
    if (ctx == nullptr) return invalid_argument("null context");
    if (heamd::bfv_impl(ctx->bfv).word_bits() != static_cast<int>(word_bits))
        return invalid_argument("word_bits is not the word of the context's scheme");
    return HE_OK;
}
// ... and last, behind every argument check
int check_device(const he_pnns_context* ctx) {
    if (heamd::bfv_impl(ctx->bfv).host_only()) return heamd::host_only_refusal();
    return ctx->plaintext->check_device();
}

template <typename W>
int transform(const he_pnns_context* ctx, bool inverse, W* slab, size_t rows, hipStream_t stream) {
    const PolyContext& ring = *ctx->plaintext;
    HEAMD_HIP_TRY(heamd::ntt_rows(inverse, slab, ring, ring.device_context(), 1, rows, stream));
    return HE_OK;
}

// ---- layer 1 ----------------------------------------------------------------------------------------------------------------------
template <typename W>
int simd_encode(const he_pnns_context* ctx, const void* slots, size_t batch, void* out, uint32_t* out_of_range, hipStream_t stream) {
    const PolyContext& ring = *ctx->plaintext;
    W* staging = static_cast<W*>(out);  // the slab encodeSimd hands to inverseNtt, transformed where it lies
    HEAMD_HIP_TRY(heamd::launch_pnns_simd_scatter(static_cast<const W*>(slots), ctx->slot_of_word_device, ring.log_degree(),
                                                  ring.moduli()[0], batch, staging, out_of_range, stream));
    return transform(ctx, true, staging, batch, stream);
}

template <typename W>
int simd_decode(const he_pnns_context* ctx, const void* plaintexts, size_t batch, void* out_slots, hipStream_t stream) {
    const PolyContext& ring = *ctx->plaintext;
    const size_t bytes = batch * ring.degree() * sizeof(W);
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(ws.resolve(nullptr, 0, bytes));
    W* copy = ws.at<W>(0);
    HEAMD_HIP_TRY(hipMemcpyAsync(copy, plaintexts, bytes, hipMemcpyDeviceToDevice, stream));
    HEAMD_TRY_STATUS(transform(ctx, false, copy, batch, stream));
    HEAMD_HIP_TRY(heamd::launch_pnns_simd_gather(copy, ctx->word_of_slot_device(), ring.log_degree(), batch,
                                                 static_cast<W*>(out_slots), stream));
    return HE_OK;
}

// ---- layer 2 ----------------------------------------------------------------------------------------------------------------------
constexpr size_t kMaxValues = size_t(1) << 40;  // values of a matrix (no product of sizes below wraps)

// packing: HE_PNNS_PACKING_DENSE_ROW or HE_PNNS_PACKING_DENSE_COLUMN
int dense_plan(const he_pnns_context* ctx, int packing, size_t rows, size_t cols, MatrixPlan& plan) {
    HEAMD_TRY_STATUS(heamd::matrix_plan(ctx, rows, cols, packing, 0, plan));
    if (rows > kMaxValues / cols || plan.plaintext_count > kMaxValues / ctx->plaintext->degree())
        return invalid_argument("matrix too large");
    return HE_OK;
}

// denseRowPlaintexts of everything validated: staging [K][N] becomes the Coeff plaintexts
template <typename W>
int pack_dense_rows(const he_pnns_context* ctx, const MatrixPlan& plan, const int64_t* values, size_t rows, size_t cols,
                    bool reduce, W* staging, uint32_t* out_of_range, hipStream_t stream) {
    const PolyContext& ring = *ctx->plaintext;
    heamd::PnnsDenseRowLayout layout{};
    layout.rows = rows;
    layout.cols = cols;
    layout.padded_cols = plan.padded_cols;
    layout.plaintext_modulus = ring.moduli()[0];
    layout.log_degree = ring.log_degree();
    layout.reduce = reduce;
    HEAMD_HIP_TRY(heamd::launch_pnns_dense_row_pack(values, ctx->slot_of_word_device, layout, plan.plaintext_count, staging,
                                                    out_of_range, stream));
    return transform(ctx, true, staging, plan.plaintext_count, stream);
}

template <typename W>
int unpack(const he_pnns_context* ctx, const MatrixPlan& plan, bool dense_row, const void* plaintexts, size_t rows, size_t cols,
           uint64_t* out_values, hipStream_t stream) {
    const PolyContext& ring = *ctx->plaintext;
    const size_t bytes = plan.plaintext_count * ring.degree() * sizeof(W);
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(ws.resolve(nullptr, 0, bytes));
    W* copy = ws.at<W>(0);
    HEAMD_HIP_TRY(hipMemcpyAsync(copy, plaintexts, bytes, hipMemcpyDeviceToDevice, stream));
    HEAMD_TRY_STATUS(transform(ctx, false, copy, plan.plaintext_count, stream));
    heamd::PnnsUnpackLayout layout{};
    layout.rows = rows;
    layout.cols = cols;
    layout.padded_cols = plan.padded_cols;
    layout.log_degree = ring.log_degree();
    layout.dense_row = dense_row;
    HEAMD_HIP_TRY(heamd::launch_pnns_unpack(copy, ctx->word_of_slot_device(), layout, out_values, stream));
    return HE_OK;
}

// ---- layer 3 ----------------------------------------------------------------------------------------------------------------------
// the secret-key context's moduli: every coefficient modulus (Context.swift:128-131)
const std::vector<heamd::u64>& all_moduli(const BfvContext& bfv) {
    return bfv.has_key_switching() ? bfv.key_switching(bfv.top_level())->moduli() : bfv.ciphertext(bfv.top_level())->moduli();
}

// Client.init's contexts (Client.swift:46-65, Config.swift validateContexts) and CrtComposer.init / compose's precondition:
// the word, the array, every context and its word, one degree and one set of coefficient moduli, distinct plaintext moduli,
// 2 q <= UInt64.max.  tables: what compose needs, inversePuncturedProducts from the host (CrtComposer.swift:34-47).
int check_client_contexts(const he_pnns_context* const* ctxs, size_t count, uint32_t word_bits, heamd::PnnsComposeTables& tables) {
    HEAMD_TRY_STATUS(heamd::check_word_bits(word_bits));
    if (ctxs == nullptr) return invalid_argument("null contexts");
    if (count == 0 || count > heamd::kPnnsMaxClientContexts) return invalid_argument("context_count must be 1..8");
    for (size_t i = 0; i < count; ++i) HEAMD_TRY_STATUS(check_word_and_context(ctxs[i], word_bits));
    const BfvContext& first = heamd::bfv_impl(ctxs[0]->bfv);
    tables = heamd::PnnsComposeTables{};
    tables.count = static_cast<uint32_t>(count);
    heamd::u128 q = 1;
    for (size_t i = 0; i < count; ++i) {
        const BfvContext& bfv = heamd::bfv_impl(ctxs[i]->bfv);
        if (bfv.degree() != first.degree() || bfv.top_level() != first.top_level() || all_moduli(bfv) != all_moduli(first))
            return invalid_argument("the contexts differ in degree or coefficient moduli");
        if (bfv.host_only() != first.host_only()) return invalid_argument("the contexts differ in where they live");
        tables.t[i] = bfv.plaintext_modulus();
        for (size_t j = 0; j < i; ++j)
            if (tables.t[j] == tables.t[i]) return invalid_argument("two contexts share a plaintext modulus");
        q *= tables.t[i];
        if (2 * q > ~uint64_t(0)) return invalid_argument("2 x the product of the plaintext moduli exceeds UInt64.max");
    }
    tables.q = static_cast<uint64_t>(q);
    for (size_t i = 0; i < count; ++i) {
        const heamd::u64 t = tables.t[i];
        heamd::u64 punctured = 1;  // (q / t_i) mod t_i, factor by factor as CrtComposer.init
        for (size_t j = 0; j < count; ++j)
            if (tables.t[j] != t) punctured = heamd::mul_mod(punctured, tables.t[j] % t, t);
        heamd::u64 inverse = 0;
        if (!heamd::inverse_mod(punctured, t, inverse)) {
            heamd::set_last_error("the plaintext moduli are not pairwise coprime");
            return HE_ERR_NOT_INVERTIBLE;
        }
        tables.inverse[i] = inverse;
        tables.inverse_shoup[i] = heamd::shoup_factor(inverse, t);
        tables.punctured[i] = tables.q / t;
    }
    return HE_OK;
}

// Where the parts of a generateQuery workspace lie, in bytes from its start: the quantised query at 0, the staged plaintexts,
// and from `encrypt` to `total` he_bfv_encrypt_device's workspace, the largest any context asks for
struct QueryPlan {
    MatrixPlan matrix;
    size_t staging = 0, encrypt = 0, total = 0;
};
int plan_query(const he_pnns_context* const* ctxs, size_t count, uint32_t word_bits, size_t query_rows, size_t cols, QueryPlan& plan) {
    HEAMD_TRY_STATUS(dense_plan(ctxs[0], HE_PNNS_PACKING_DENSE_ROW, query_rows, cols, plan.matrix));
    const BfvContext& bfv = heamd::bfv_impl(ctxs[0]->bfv);
    heamd::WorkspaceLayout layout;
    layout.add(query_rows * cols * sizeof(int64_t));
    plan.staging = layout.add(plan.matrix.plaintext_count * bfv.degree() * (word_bits / 8));
    size_t encrypt_bytes = 0;
    for (size_t i = 0; i < count; ++i)
        encrypt_bytes = std::max(encrypt_bytes, he_bfv_encrypt_workspace_bytes(ctxs[i]->bfv, word_bits, HE_ENCRYPT_OP_ENCRYPT,
                                                                               bfv.top_level(), 0, plan.matrix.plaintext_count));
    plan.encrypt = layout.add(encrypt_bytes);
    plan.total = layout.total();
    return HE_OK;
}

template <typename W>
int generate_query(const he_pnns_context* const* ctxs, size_t count, const QueryPlan& plan, const float* vectors, size_t query_rows,
                   size_t cols, float scaling_factor, const void* secret_key, const uint8_t* a_seeds, const uint8_t* error_seeds,
                   void* out, uint32_t* out_of_range, void* workspace, size_t workspace_bytes, he_stream s) {
    hipStream_t stream = as_stream(s);
    const BfvContext& bfv = heamd::bfv_impl(ctxs[0]->bfv);
    const uint32_t L = bfv.top_level();
    const size_t K = plan.matrix.plaintext_count, ct_words = size_t(2) * L * bfv.degree();
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(ws.resolve(workspace, workspace_bytes, plan.total));
    int64_t* quantised = ws.at<int64_t>(0);
    W* staging = ws.at<W>(plan.staging);
    // vectors.normalizedScaledAndRounded(scalingFactor:) (Client.swift:77-78), once for every context
    HEAMD_HIP_TRY(heamd::launch_pnns_quantize_rows(vectors, query_rows, cols, scaling_factor, quantised, stream));
    for (size_t i = 0; i < count; ++i) {
        // shouldReduce = contexts.count > 1 (:81); PlaintextMatrix(.denseRow), then encrypt: Coeff at the top level (:82-88)
        HEAMD_TRY_STATUS(pack_dense_rows<W>(ctxs[i], plan.matrix, quantised, query_rows, cols, count > 1, staging, out_of_range,
                                            stream));
        HEAMD_TRY_STATUS(he_bfv_encrypt_device(ctxs[i]->bfv, 8 * sizeof(W), L, secret_key, a_seeds + i * K * 32,
                                               error_seeds + i * K * 32, staging, static_cast<W*>(out) + i * K * ct_words, K,
                                               ws.at(plan.encrypt), plan.total - plan.encrypt, s));
    }
    return HE_OK;
}

// Plaintexts of a group of decrypt(response:): the workspace of a group stays near 1 GiB.
// HEAMD_PNNS_CLIENT_GROUP=<plaintexts> forces smaller groups (the tests: many groups must give the distances of one).
size_t response_group(size_t plaintexts, size_t n, size_t count, uint32_t moduli_count, size_t word_bytes) {
    size_t group = (size_t(1) << 30) / (n * word_bytes * (count + 2 * size_t(moduli_count)));
    if (const char* forced = std::getenv("HEAMD_PNNS_CLIENT_GROUP")) {
        const size_t want = static_cast<size_t>(std::strtoull(forced, nullptr, 10));
        if (want != 0 && want < group) group = want;
    }
    if (group > plaintexts) group = plaintexts;
    return group ? group : 1;
}

// ... of a decrypt(response:) workspace: the plaintexts of a group at 0, from `decrypt` to `total` he_bfv_decrypt_device's
struct ResponsePlan {
    MatrixPlan matrix;
    size_t group = 0, decrypt = 0, total = 0;
};
int plan_response(const he_pnns_context* const* ctxs, size_t count, uint32_t word_bits, uint32_t moduli_count, size_t rows,
                  size_t query_rows, ResponsePlan& plan) {
    HEAMD_TRY_STATUS(dense_plan(ctxs[0], HE_PNNS_PACKING_DENSE_COLUMN, rows, query_rows, plan.matrix));
    const BfvContext& bfv = heamd::bfv_impl(ctxs[0]->bfv);
    if (!bfv.valid(moduli_count)) return invalid_argument("moduli_count out of range");
    plan.group = response_group(plan.matrix.plaintext_count, bfv.degree(), count, moduli_count, word_bits / 8);
    heamd::WorkspaceLayout layout;
    layout.add(count * plan.group * bfv.degree() * (word_bits / 8));
    size_t decrypt_bytes = 0;
    for (size_t i = 0; i < count; ++i)
        decrypt_bytes = std::max(decrypt_bytes, he_bfv_decrypt_workspace_bytes(ctxs[i]->bfv, word_bits, moduli_count, 2, 0, plan.group));
    plan.decrypt = layout.add(decrypt_bytes);
    plan.total = layout.total();
    return HE_OK;
}

// where the values of plaintext p of a dense-column packed R-row matrix begin in the column-major sequence (pnns_client_kernels.hip
// dense_column_place is its inverse)
size_t dense_column_first_value(size_t p, size_t rows, size_t n) {
    const size_t half = n / 2;
    if (rows <= half) return p * 2 * rows * (half / rows);
    const size_t per_column = heamd::dividing_ceil(rows, n);
    return (p / per_column) * rows + (p % per_column) * n;
}

template <typename W>
int decrypt_response(const he_pnns_context* const* ctxs, size_t count, const ResponsePlan& plan,
                     const heamd::PnnsComposeTables& tables, uint32_t moduli_count, const void* response, const void* secret_key,
                     size_t rows, size_t query_rows, float scaling_factor, float* out_distances, void* workspace,
                     size_t workspace_bytes, he_stream s) {
    hipStream_t stream = as_stream(s);
    const BfvContext& bfv = heamd::bfv_impl(ctxs[0]->bfv);
    const size_t n = bfv.degree(), M = plan.matrix.plaintext_count, total = rows * query_rows;
    const size_t ct_words = size_t(2) * moduli_count * n;
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(ws.resolve(workspace, workspace_bytes, plan.total));
    W* plaintexts = ws.at<W>(0);  // [count][group][N]
    for (size_t first = 0; first < M; first += plan.group) {
        const size_t now = M - first < plan.group ? M - first : plan.group;
        for (size_t i = 0; i < count; ++i) {
            // ciphertextMatrix.decrypt(using:) (:105), then decodeSimd's forwardNtt for unpack()
            W* mine = plaintexts + i * plan.group * n;
            HEAMD_TRY_STATUS(he_bfv_decrypt_device(ctxs[i]->bfv, 8 * sizeof(W), moduli_count, 2, 0,
                                                   static_cast<const W*>(response) + (i * M + first) * ct_words, secret_key, 1, mine,
                                                   now, ws.at(plan.decrypt), plan.total - plan.decrypt, s));
            HEAMD_TRY_STATUS(transform(ctxs[i], false, mine, now, stream));
        }
        heamd::PnnsComposeLayout layout{};
        layout.rows = rows;
        layout.cols = query_rows;
        layout.first_plaintext = first;
        layout.first_element = dense_column_first_value(first, rows, n);
        const size_t end = first + now == M ? total : dense_column_first_value(first + now, rows, n);
        layout.elements = (end < total ? end : total) - layout.first_element;
        layout.context_stride = plan.group * n;
        layout.log_degree = ctxs[0]->plaintext->log_degree();
        HEAMD_HIP_TRY(heamd::launch_pnns_compose_distances(plaintexts, ctxs[0]->word_of_slot_device(), layout, tables,
                                                           scaling_factor, out_distances, stream));
    }
    return HE_OK;
}

}  // namespace
}  // extern "C++"

int he_pnns_simd_encode_device(const he_pnns_context* ctx, uint32_t word_bits, const void* slots, size_t batch,
                               void* out_plaintexts, uint32_t* out_of_range, he_stream s) {
    HEAMD_TRY_STATUS(check_word_and_context(ctx, word_bits));
    if (batch == 0) return HE_OK;
    if (batch > kMaxValues / ctx->plaintext->degree()) return invalid_argument("batch too large");
    if (slots == nullptr || out_plaintexts == nullptr) return invalid_argument("null buffer");
    const size_t bytes = batch * ctx->plaintext->degree() * (word_bits / 8);
    HEAMD_TRY_STATUS(heamd::check_slabs("encodeSimd", {{"out_plaintexts", out_plaintexts, bytes, true},
                                                       {"out_of_range", out_of_range, sizeof(uint32_t), true},
                                                       {"slots", slots, bytes, false}}));
    HEAMD_TRY_STATUS(check_device(ctx));
    return heamd::with_word(word_bits, [&](auto word) {
        return simd_encode<decltype(word)>(ctx, slots, batch, out_plaintexts, out_of_range, as_stream(s));
    });
}

int he_pnns_simd_decode_device(const he_pnns_context* ctx, uint32_t word_bits, const void* plaintexts, size_t batch,
                               void* out_slots, he_stream s) {
    HEAMD_TRY_STATUS(check_word_and_context(ctx, word_bits));
    if (batch == 0) return HE_OK;
    if (batch > kMaxValues / ctx->plaintext->degree()) return invalid_argument("batch too large");
    if (plaintexts == nullptr || out_slots == nullptr) return invalid_argument("null buffer");
    const size_t bytes = batch * ctx->plaintext->degree() * (word_bits / 8);
    HEAMD_TRY_STATUS(heamd::check_slabs("decodeSimd", {{"out_slots", out_slots, bytes, true}, {"plaintexts", plaintexts, bytes, false}}));
    HEAMD_TRY_STATUS(check_device(ctx));
    return heamd::with_word(word_bits, [&](auto word) {
        return simd_decode<decltype(word)>(ctx, plaintexts, batch, out_slots, as_stream(s));
    });
}

int he_pnns_pack_dense_rows_device(const he_pnns_context* ctx, uint32_t word_bits, const int64_t* signed_values, size_t rows,
                                   size_t cols, int reduce, void* out_plaintexts, uint32_t* out_of_range, he_stream s) {
    HEAMD_TRY_STATUS(check_word_and_context(ctx, word_bits));
    MatrixPlan plan;
    HEAMD_TRY_STATUS(dense_plan(ctx, HE_PNNS_PACKING_DENSE_ROW, rows, cols, plan));
    if (signed_values == nullptr || out_plaintexts == nullptr) return invalid_argument("null buffer");
    HEAMD_TRY_STATUS(heamd::check_slabs(
        "denseRowPlaintexts", {{"out_plaintexts", out_plaintexts, plan.plaintext_count * ctx->plaintext->degree() * (word_bits / 8), true},
                               {"out_of_range", out_of_range, sizeof(uint32_t), true},
                               {"signed_values", signed_values, rows * cols * sizeof(int64_t), false}}));
    HEAMD_TRY_STATUS(check_device(ctx));
    return heamd::with_word(word_bits, [&](auto word) {
        return pack_dense_rows(ctx, plan, signed_values, rows, cols, reduce != 0, static_cast<decltype(word)*>(out_plaintexts),
                               out_of_range, as_stream(s));
    });
}

int he_pnns_unpack_device(const he_pnns_context* ctx, uint32_t word_bits, int packing, const void* plaintexts, size_t rows,
                          size_t cols, uint64_t* out_values, he_stream s) {
    HEAMD_TRY_STATUS(check_word_and_context(ctx, word_bits));
    MatrixPlan plan;
    if (packing == HE_PNNS_PACKING_DENSE_ROW || packing == HE_PNNS_PACKING_DENSE_COLUMN) {
        HEAMD_TRY_STATUS(dense_plan(ctx, packing, rows, cols, plan));
    } else if (packing == HE_PNNS_PACKING_DIAGONAL) {
        heamd::set_last_error("unpackDiagonal is not on the device");
        return HE_ERR_UNSUPPORTED;
    } else {
        return invalid_argument("unknown packing");
    }
    if (plaintexts == nullptr || out_values == nullptr) return invalid_argument("null buffer");
    HEAMD_TRY_STATUS(heamd::check_slabs(
        "unpack", {{"out_values", out_values, rows * cols * sizeof(uint64_t), true},
                   {"plaintexts", plaintexts, plan.plaintext_count * ctx->plaintext->degree() * (word_bits / 8), false}}));
    HEAMD_TRY_STATUS(check_device(ctx));
    const bool dense_row = packing == HE_PNNS_PACKING_DENSE_ROW;
    return heamd::with_word(word_bits, [&](auto word) {
        return unpack<decltype(word)>(ctx, plan, dense_row, plaintexts, rows, cols, out_values, as_stream(s));
    });
}

size_t he_pnns_generate_query_workspace_bytes(const he_pnns_context* const* ctxs, size_t context_count, uint32_t word_bits,
                                              size_t query_rows, size_t cols) {
    heamd::PnnsComposeTables tables;
    QueryPlan plan;
    const bool ok = check_client_contexts(ctxs, context_count, word_bits, tables) == HE_OK &&
                    plan_query(ctxs, context_count, word_bits, query_rows, cols, plan) == HE_OK;
    return ok ? plan.total : 0;
}

int he_pnns_generate_query_device(const he_pnns_context* const* ctxs, size_t context_count, uint32_t word_bits,
                                  const float* vectors, size_t query_rows, size_t cols, float scaling_factor,
                                  const void* secret_key, const uint8_t* a_seeds, const uint8_t* error_seeds, void* out,
                                  uint32_t* out_of_range, void* workspace, size_t workspace_bytes, he_stream s) {
    heamd::PnnsComposeTables tables;
    HEAMD_TRY_STATUS(check_client_contexts(ctxs, context_count, word_bits, tables));
    QueryPlan plan;
    HEAMD_TRY_STATUS(plan_query(ctxs, context_count, word_bits, query_rows, cols, plan));
    if (vectors == nullptr || secret_key == nullptr || a_seeds == nullptr || error_seeds == nullptr || out == nullptr)
        return invalid_argument("null vectors, secret key, seeds or ciphertexts");
    const BfvContext& bfv = heamd::bfv_impl(ctxs[0]->bfv);
    const size_t K = plan.matrix.plaintext_count, row_bytes = size_t(bfv.degree()) * (word_bits / 8);
    HEAMD_TRY_STATUS(heamd::check_slabs("generateQuery", {{"out", out, context_count * K * 2 * bfv.top_level() * row_bytes, true},
                                                          {"workspace", workspace, workspace_bytes, true},
                                                          {"out_of_range", out_of_range, sizeof(uint32_t), true},
                                                          {"vectors", vectors, query_rows * cols * sizeof(float), false},
                                                          {"secret_key", secret_key, bfv.top_level() * row_bytes, false},
                                                          {"a_seeds", a_seeds, context_count * K * 32, false},
                                                          {"error_seeds", error_seeds, context_count * K * 32, false}}));
    for (size_t i = 0; i < context_count; ++i) {
        HEAMD_TRY_STATUS(check_device(ctxs[i]));
        HEAMD_TRY_STATUS(heamd::bfv_encrypt_check_device(ctxs[i]->bfv, word_bits, bfv.top_level()));
    }
    return heamd::with_word(word_bits, [&](auto word) {
        return generate_query<decltype(word)>(ctxs, context_count, plan, vectors, query_rows, cols, scaling_factor, secret_key,
                                              a_seeds, error_seeds, out, out_of_range, workspace, workspace_bytes, s);
    });
}

size_t he_pnns_decrypt_response_workspace_bytes(const he_pnns_context* const* ctxs, size_t context_count, uint32_t word_bits,
                                                uint32_t moduli_count, size_t rows, size_t query_rows) {
    heamd::PnnsComposeTables tables;
    ResponsePlan plan;
    const bool ok = check_client_contexts(ctxs, context_count, word_bits, tables) == HE_OK &&
                    plan_response(ctxs, context_count, word_bits, moduli_count, rows, query_rows, plan) == HE_OK;
    return ok ? plan.total : 0;
}

int he_pnns_decrypt_response_device(const he_pnns_context* const* ctxs, size_t context_count, uint32_t word_bits,
                                    uint32_t moduli_count, const void* response, const void* secret_key, size_t rows,
                                    size_t query_rows, float scaling_factor, float* out_distances, void* workspace,
                                    size_t workspace_bytes, he_stream s) {
    heamd::PnnsComposeTables tables;
    HEAMD_TRY_STATUS(check_client_contexts(ctxs, context_count, word_bits, tables));
    ResponsePlan plan;
    HEAMD_TRY_STATUS(plan_response(ctxs, context_count, word_bits, moduli_count, rows, query_rows, plan));
    if (response == nullptr || secret_key == nullptr || out_distances == nullptr)
        return invalid_argument("null response, secret key or distances");
    const BfvContext& bfv = heamd::bfv_impl(ctxs[0]->bfv);
    const size_t row_bytes = size_t(bfv.degree()) * (word_bits / 8);
    HEAMD_TRY_STATUS(heamd::check_slabs(
        "decrypt(response:)", {{"out_distances", out_distances, rows * query_rows * sizeof(float), true},
                               {"workspace", workspace, workspace_bytes, true},
                               {"response", response, context_count * plan.matrix.plaintext_count * 2 * moduli_count * row_bytes, false},
                               {"secret_key", secret_key, moduli_count * row_bytes, false}}));
    for (size_t i = 0; i < context_count; ++i) {
        HEAMD_TRY_STATUS(check_device(ctxs[i]));
        HEAMD_TRY_STATUS(heamd::bfv_decrypt_check_device(ctxs[i]->bfv, word_bits, moduli_count));
    }
    return heamd::with_word(word_bits, [&](auto word) {
        return decrypt_response<decltype(word)>(ctxs, context_count, plan, tables, moduli_count, response, secret_key, rows,
                                                query_rows, scaling_factor, out_distances, workspace, workspace_bytes, s);
    });
}
