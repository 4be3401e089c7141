// pnns_api.cpp -- the PNNS server database (reference Sources/PrivateNearestNeighborSearch/) behind the C ABI: the SIMD
// encoding context a he_bfv_context lacks, the plan (PlaintextMatrix.plaintextCount, BabyStepGiantStep.init) and
// Database.process for one context (ProcessedDatabase.swift:194-229).  Kernels: pnns_kernels.hip.
//
// Per group of plaintexts: the pack kernel writes the slabs Context.encodeSimd (Encoding.swift:222-234) fills through
// simdEncodingMatrix, the batched inverse NTT over [t] turns them into Coeff plaintexts in place, and
// Plaintext.convertToEvalFormat (he_bfv_plaintext_to_eval_device) takes them into the matrix.  The inverse NTT is in place, so
// one N-word staging slab per plaintext of a group is all the scratch there is.
//
// And the server's answer, Server.computeResponse (Server.swift:61-88) for one-row query vectors: PlaintextMatrix.mulTranspose(
// vector:using:) (MatrixMultiplication.swift:131-226) over Q independent queries, then modSwitchDownToSingle.  Rotations, the
// transforms, additions and the mod-switch are the bodies of the library's own entry points for either word (word_layer.hpp),
// batched over the queries; the one kernel of its own is the pass over the matrix (pnns_kernels.hip,
// pnns_bsgs_inner_product_kernel).
//
// And PlaintextMatrix.mulTranspose(matrix:using:) (MatrixMultiplication.swift:236-298) for query matrices of several rows:
// CiphertextMatrix.extractDenseRow per row (masks and masked products: pnns_row_mask_kernel, pnns_extract_rows_kernel), the
// product above over all rows of all clients, and the dense-column packing of the per-row results.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <vector>

#include "api_internal.hpp"
#include "bfv_context.hpp"
#include "kernels.hpp"
#include "pnns_context.hpp"
#include "word_layer.hpp"

using heamd::as_stream;
using heamd::dividing_ceil;
using heamd::invalid_argument;
using heamd::matrix_plan;
using heamd::MatrixPlan;
using heamd::next_power_of_two;
using heamd::Scratch;

// PlaintextMatrix.plaintextCount (PlaintextMatrix.swift:246-275) and BabyStepGiantStep.init (MatrixMultiplication.swift:33-60)
int heamd::matrix_plan(const he_pnns_context* ctx, size_t rows, size_t cols, int packing, uint32_t baby_step, MatrixPlan& plan) {
    if (ctx == nullptr) return invalid_argument("null context");
    if (rows == 0 || cols == 0) return invalid_argument("matrix dimensions must be positive");  // MatrixDimensions.init
    if (rows > (size_t(1) << 40) || cols > (size_t(1) << 40)) return invalid_argument("matrix too large");
    const size_t n = ctx->plaintext->degree();
    const size_t simd_columns = n / 2;  // SimdEncodingDimensions: 2 rows of N / 2 columns
    plan = MatrixPlan{};
    plan.padded_cols = next_power_of_two(cols);
    plan.plaintexts_per_column = dividing_ceil(rows, n);
    switch (packing) {
        case HE_PNNS_PACKING_DENSE_COLUMN: {
            const size_t columns_per_plaintext = 2 * (simd_columns / rows);
            plan.plaintext_count = columns_per_plaintext > 1 ? dividing_ceil(cols, columns_per_plaintext)
                                                             : cols * dividing_ceil(rows, n);
            break;
        }
        case HE_PNNS_PACKING_DENSE_ROW: {
            if (cols > simd_columns) return invalid_argument("column_count exceeds the SIMD column count");
            const size_t rows_per_plaintext = 2 * (simd_columns / plan.padded_cols);
            plan.plaintext_count = dividing_ceil(rows, rows_per_plaintext);
            break;
        }
        case HE_PNNS_PACKING_DIAGONAL:
            if (cols > simd_columns) return invalid_argument("column_count exceeds the SIMD column count");
            plan.plaintext_count = plan.padded_cols * plan.plaintexts_per_column;
            break;
        default:
            return invalid_argument("unknown packing");
    }
    size_t baby = baby_step;
    if (baby == 0) {  // Int(Double(dimension).squareRoot().rounded(.up)), dimension a power of two
        while (baby * baby < plan.padded_cols) ++baby;
    }
    const size_t giant = dividing_ceil(plan.padded_cols, baby);
    if (baby < giant) return invalid_argument("babyStep cannot be smaller than giantStep");
    plan.baby_step = static_cast<uint32_t>(baby);
    plan.giant_step = static_cast<uint32_t>(giant);
    return HE_OK;
}

namespace {

// generateEncodingMatrix (Encoding.swift:197-219)
std::vector<uint32_t> encoding_matrix(uint32_t degree, uint32_t log_degree) {
    std::vector<uint32_t> matrix(degree, 0);
    auto reversed = [log_degree](uint32_t x) {
        uint32_t r = 0;
        for (uint32_t bit = 0; bit < log_degree; ++bit) r |= ((x >> bit) & 1u) << (log_degree - 1 - bit);
        return r;
    };
    const uint32_t row_size = degree >> 1, mask = (degree << 1) - 1;
    uint32_t power = 1;
    for (uint32_t i = 0; i < row_size; ++i) {
        matrix[i] = reversed((power - 1) >> 1);
        matrix[row_size | i] = reversed((mask - power) >> 1);
        power = (power * 3u) & mask;  // GaloisElementGenerator.value
    }
    return matrix;
}

int pnns_create(const he_bfv_context* bfv_handle, int word_bits, he_pnns_context** out) {
    if (out == nullptr) return invalid_argument("null out");
    *out = nullptr;
    if (bfv_handle == nullptr) return invalid_argument("null context");
    const heamd::BfvContext& bfv = heamd::bfv_impl(bfv_handle);
    if (bfv.word_bits() != word_bits)
        return invalid_argument(word_bits == 32 ? "he_pnns_context_create_u32 needs a Bfv<UInt32> context"
                                                : "he_pnns_context_create needs a Bfv<UInt64> context");
    if (bfv.degree() < 2 || bfv.degree() > (1u << 20)) return invalid_argument("degree out of range");
    if (!bfv.host_only()) {  // the tables go to the device the BFV context lives on
        const int status = bfv.ciphertext(bfv.top_level())->check_device();
        if (status != HE_OK) return status;
    }
    auto ctx = std::make_unique<he_pnns_context>();
    ctx->bfv = bfv_handle;
    const uint64_t t = bfv.plaintext_modulus();
    const int status = heamd::PolyContext::create(bfv.degree(), &t, 1, ctx->plaintext, bfv.host_only());
    if (status != HE_OK) return status;
    if (!ctx->plaintext->all_ntt(1)) {  // generateEncodingMatrix returns [] (Encoding.swift:198-200)
        heamd::set_last_error("the plaintext modulus is not an NTT modulus for the degree: no SIMD encoding");
        return HE_ERR_SIMD_ENCODING_NOT_SUPPORTED;
    }
    ctx->encoding_matrix = encoding_matrix(bfv.degree(), ctx->plaintext->log_degree());
    if (!bfv.host_only()) {
        // slot_of_word, then simdEncodingMatrix itself (decodeSimd reads through it: Encoding.swift:242-244)
        std::vector<uint32_t> tables(2 * size_t(bfv.degree()));
        for (uint32_t slot = 0; slot < bfv.degree(); ++slot) {
            tables[ctx->encoding_matrix[slot]] = slot;
            tables[bfv.degree() + slot] = ctx->encoding_matrix[slot];
        }
        const size_t bytes = tables.size() * sizeof(uint32_t);
        HEAMD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&ctx->slot_of_word_device), bytes));
        HEAMD_HIP_TRY(hipMemcpy(ctx->slot_of_word_device, tables.data(), bytes, hipMemcpyHostToDevice));
    }
    *out = ctx.release();
    return HE_OK;
}

// Plaintexts per group: the group's share of the matrix stays near 1 GiB and no launch of a group reaches 2^31 lanes.
// HEAMD_PNNS_PROCESS_GROUP=<plaintexts> forces smaller groups (the tests: many groups must give the words of one).
size_t group_plaintexts(size_t n, uint32_t L, size_t word_bytes) {
    size_t group = (size_t(1) << 30) / (n * L * word_bytes);
    const size_t ntt_bound = (size_t(1) << 30) / (n * L);  // the lift / transform launches: plaintexts * L * N words
    if (ntt_bound < group) group = ntt_bound;
    if (const char* forced = std::getenv("HEAMD_PNNS_PROCESS_GROUP")) {
        const size_t want = static_cast<size_t>(std::strtoull(forced, nullptr, 10));
        if (want != 0 && want < group) group = want;
    }
    return group ? group : 1;
}

template <typename W>
int diagonal_matrix(const he_pnns_context* ctx, const int64_t* values, size_t rows, size_t cols, uint32_t baby_step,
                    int reduce, uint32_t moduli_count, W* out, uint32_t* out_of_range, he_stream s) {
    MatrixPlan plan;
    const int status = matrix_plan(ctx, rows, cols, HE_PNNS_PACKING_DIAGONAL, baby_step, plan);
    if (status != HE_OK) return status;
    const heamd::BfvContext& bfv = heamd::bfv_impl(ctx->bfv);
    if (bfv.word_bits() != 8 * sizeof(W)) return invalid_argument("context of the other word size");
    // the level checks of Plaintext.convertToEvalFormat (host-only context: HE_ERR_DEVICE) before anything is enqueued
    HEAMD_TRY_STATUS(heamd::bfv_plaintext_to_eval<W>(ctx->bfv, moduli_count, nullptr, nullptr, 0, as_stream(s)));
    if (values == nullptr || out == nullptr) return invalid_argument("null buffer");
    const heamd::PolyContext& ring = *ctx->plaintext;
    const int on_device = ring.check_device();
    if (on_device != HE_OK) return on_device;
    hipStream_t stream = as_stream(s);
    const size_t n = ring.degree();
    heamd::PnnsMatrixLayout layout{};
    layout.rows = rows;
    layout.cols = cols;
    layout.padded_cols = plan.padded_cols;
    layout.plaintexts_per_column = plan.plaintexts_per_column;
    layout.plaintext_modulus = bfv.plaintext_modulus();
    layout.log_degree = ring.log_degree();
    layout.baby_step = plan.baby_step;
    layout.reduce = reduce != 0;
    const size_t total = plan.plaintext_count;
    const size_t group = group_plaintexts(n, moduli_count, sizeof(W));
    Scratch staging_mem(stream);
    HEAMD_HIP_TRY(staging_mem.allocate((total < group ? total : group) * n * sizeof(W)));
    W* staging = static_cast<W*>(staging_mem.get());
    for (size_t first = 0; first < total; first += group) {
        const size_t count = total - first < group ? total - first : group;
        HEAMD_HIP_TRY(heamd::launch_pnns_diagonal_pack<W>(values, ctx->slot_of_word_device, layout, first, count, staging,
                                                           out_of_range, stream));
        HEAMD_HIP_TRY(ntt_rows(true, staging, ring, ring.device_context(), 1, count, stream));
        HEAMD_TRY_STATUS(heamd::bfv_plaintext_to_eval(ctx->bfv, moduli_count, staging, out + first * moduli_count * n, count,
                                                      stream));
    }
    return HE_OK;
}

// ---- mulTranspose(vector:using:) and computeResponse ---------------------------------------------------------------------------
// applyGalois on `groups` runs of `group_size` ciphertexts, run g under keys[g * key_stride]
template <typename W>
int apply_galois(const he_bfv_context* ctx, uint32_t L, const W* in, uint64_t element, const W* const* keys,
                 size_t key_stride, size_t groups, size_t group_size, W* out, he_stream s) {
    std::vector<const W*> per_group(groups);
    for (size_t g = 0; g < groups; ++g) per_group[g] = keys[g * key_stride];
    return heamd::bfv_apply_galois_grouped(ctx, L, in, element, per_group.data(), groups, group_size, out, nullptr, 0,
                                           as_stream(s));
}

// Result ciphertexts per group: the inner products of a group ([G][Q][group][2][L][N]) stay near 2 GiB.
// HEAMD_PNNS_RESPONSE_GROUP=<result ciphertexts> forces smaller groups (the tests: many groups must give the words of one).
size_t response_group(size_t result_count, size_t queries, size_t giant_step, size_t ct_bytes) {
    size_t group = (size_t(2) << 30) / (queries * giant_step * ct_bytes);
    if (const char* forced = std::getenv("HEAMD_PNNS_RESPONSE_GROUP")) {
        const size_t want = static_cast<size_t>(std::strtoull(forced, nullptr, 10));
        if (want != 0 && want < group) group = want;
    }
    if (group > result_count) group = result_count;
    return group ? group : 1;
}

// mulTranspose(vector:using:) (MatrixMultiplication.swift:131-226) for `vectors` one-row vectors already on the device:
// vector v under the keys keys[v * key_stride] (rotatingColumns(by: -1)) and keys[v * key_stride + 1] ((by: -babyStep)).
// Everything has been validated.  out [vectors][C][2][L][N], or [..][2][1][N] through modSwitchDownToSingle.
template <typename W>
int bsgs_product(const he_pnns_context* ctx, const MatrixPlan& plan, const W* matrix, const W* queries,
                 const W* const* galois_keys, size_t key_stride, size_t vectors, W* out, bool to_single, he_stream s) {
    const heamd::BfvContext& bfv = heamd::bfv_impl(ctx->bfv);
    const uint32_t b = plan.baby_step, G = plan.giant_step, L = bfv.top_level();
    const size_t n = bfv.degree(), C = plan.plaintexts_per_column, Q = vectors;
    const bool need_one = b > 1, need_baby = G > 1;
    const heamd::PolyContext* q_ctx = bfv.ciphertext(L);
    const he_poly_context* ring = he_bfv_ciphertext_context(ctx->bfv, L);
    hipStream_t stream = as_stream(s);
    const size_t poly = size_t(L) * n, ct = 2 * poly, ct_bytes = ct * sizeof(W);
    uint64_t element_one = 0, element_baby = 0;
    if (need_one) HEAMD_TRY_STATUS(he_galois_element_rotating_columns(-1, n, &element_one));
    if (need_baby) HEAMD_TRY_STATUS(he_galois_element_rotating_columns(-static_cast<int64_t>(b), n, &element_baby));

    // 1) the baby steps (:178-191): state j = state j - 1 rotated by -1, one batch over the queries per step; then every state
    //    to Eval.  rot [b][Q][2][L][N]
    Scratch rot_mem(stream);
    HEAMD_HIP_TRY(rot_mem.allocate(size_t(b) * Q * ct_bytes));
    W* rot = static_cast<W*>(rot_mem.get());
    HEAMD_HIP_TRY(hipMemcpyAsync(rot, queries, Q * ct_bytes, hipMemcpyDeviceToDevice, stream));
    for (uint32_t j = 1; j < b; ++j)
        HEAMD_TRY_STATUS(apply_galois(ctx->bfv, L, rot + size_t(j - 1) * Q * ct, element_one, galois_keys, key_stride, Q, 1,
                                      rot + size_t(j) * Q * ct, s));
    HEAMD_TRY_STATUS(heamd::poly_ntt(ring, rot, size_t(b) * Q * 2, false, stream));

    heamd::PnnsBsgsLayout layout{};
    layout.rot_step_words = Q * ct;
    layout.log_degree = q_ctx->log_degree();
    layout.moduli_count = L;
    layout.baby_step = b;
    layout.giant_step = G;
    layout.padded_cols = static_cast<uint32_t>(plan.padded_cols);
    layout.columns = static_cast<uint32_t>(C);
    layout.out_queries = static_cast<uint32_t>(Q);
    const heamd::AccumulatorCadence lazy = heamd::accumulator_cadence(*q_ctx, L);
    layout.max_lazy = lazy.max_lazy;
    layout.cadence = lazy.cadence;
    layout.narrow_moduli = lazy.narrow_moduli;
    const unsigned per_pass = heamd::pnns_bsgs_queries_per_pass(layout, sizeof(W), Q);
    const heamd::DeviceContext dc = q_ctx->device_context(L);

    const size_t group = response_group(C, Q, G, ct_bytes);
    const size_t out_ct = to_single ? 2 * n : ct;  // words of a result ciphertext in `out`
    Scratch products_mem(stream), sums_mem(stream);
    HEAMD_HIP_TRY(products_mem.allocate(Q * G * group * ct_bytes));
    HEAMD_HIP_TRY(sums_mem.allocate(2 * Q * group * ct_bytes));
    W* products = static_cast<W*>(products_mem.get());  // [G][Q][now][2][L][N]
    W* sums = static_cast<W*>(sums_mem.get());          // two of [Q][now][2][L][N]
    for (size_t first = 0; first < C; first += group) {
        const size_t now = C - first < group ? C - first : group;
        // 2) the inner products of every giant step (:195-212), per_pass queries to a pass over the group's plaintexts
        layout.first_column = static_cast<uint32_t>(first);
        layout.group_columns = static_cast<uint32_t>(now);
        for (size_t q = 0; q < Q; q += per_pass) {
            const unsigned taken = Q - q < per_pass ? static_cast<unsigned>(Q - q) : per_pass;
            HEAMD_HIP_TRY(heamd::launch_pnns_bsgs_inner_product<W>(rot + q * ct, matrix, products + q * now * ct, dc, layout,
                                                                   taken, stream));
        }
        HEAMD_TRY_STATUS(heamd::poly_ntt(ring, products, Q * G * now * 2, true, stream));
        // 3) rotateColumnsAndSum (HeScheme.swift:113-133): the last giant step's product, then per earlier one rotate by
        //    -babyStep and add it; every step one key switch and one addition over the Q x now accumulators.  The products are
        //    giant-step major, so the last step's slab is the first accumulator where it lies.
        W* current = products + size_t(G - 1) * Q * now * ct;
        W* other = sums;
        for (uint32_t g = G - 1; g-- > 0;) {
            HEAMD_TRY_STATUS(apply_galois(ctx->bfv, L, current, element_baby, galois_keys + 1, key_stride, Q, now, other, s));
            HEAMD_TRY_STATUS(heamd::poly_elementwise(ring, heamd::ElementwiseOp::Add, other, products + size_t(g) * Q * now * ct,
                                                     Q * now * 2, stream));
            current = other;
            other = current == sums ? sums + Q * now * ct : sums;
        }
        // 4) the group's results to their places in out [Q][C]; computeResponse: through modSwitchDownToSingle (Server.swift:84)
        if (to_single && now == C) {
            HEAMD_TRY_STATUS(heamd::bfv_mod_switch_down_to_single(ctx->bfv, L, 2, current, out, Q * C, stream));
        } else if (to_single) {
            HEAMD_TRY_STATUS(heamd::bfv_mod_switch_down_to_single(ctx->bfv, L, 2, current, other, Q * now, stream));
            HEAMD_HIP_TRY(hipMemcpy2DAsync(out + first * out_ct, C * out_ct * sizeof(W), other, now * out_ct * sizeof(W),
                                           now * out_ct * sizeof(W), Q, hipMemcpyDeviceToDevice, stream));
        } else {
            HEAMD_HIP_TRY(hipMemcpy2DAsync(out + first * out_ct, C * out_ct * sizeof(W), current, now * out_ct * sizeof(W),
                                           now * out_ct * sizeof(W), Q, hipMemcpyDeviceToDevice, stream));
        }
    }
    return HE_OK;
}

// the argument checks the one-row and the several-rows entries share, in the documented order, up to the word size
template <typename W>
int response_plan(const he_pnns_context* ctx, size_t matrix_plaintext_count, size_t rows, size_t cols, uint32_t baby_step,
                  MatrixPlan& plan) {
    if (ctx == nullptr) return invalid_argument("null context");
    if (baby_step == 0) return invalid_argument("baby_step must be the one the matrix was packed with");
    const int planned = matrix_plan(ctx, rows, cols, HE_PNNS_PACKING_DIAGONAL, baby_step, plan);
    if (planned != HE_OK) return planned;
    if (matrix_plaintext_count != plan.plaintext_count)  // PnnsError.invalidMatrixDimensions, MatrixMultiplication.swift:147-149
        return invalid_argument("the matrix does not hold nextPowerOfTwo(cols) x ceil(rows / N) plaintexts");
    if (heamd::bfv_impl(ctx->bfv).word_bits() != 8 * sizeof(W)) return invalid_argument("context of the other word size");
    return HE_OK;
}

template <typename W>
int response_buffers(const he_pnns_context* ctx, const W* matrix, const W* queries, const W* out) {
    if (matrix == nullptr || queries == nullptr || out == nullptr) return invalid_argument("null buffer");
    if (reinterpret_cast<uintptr_t>(matrix) % 16 != 0) return invalid_argument("the matrix must be 16-byte aligned");
    const heamd::BfvContext& bfv = heamd::bfv_impl(ctx->bfv);
    if (bfv.degree() < 16 / sizeof(W)) return invalid_argument("degree below one 16-byte access");
    return bfv.ciphertext(bfv.top_level())->check_device();
}

template <typename W>
int mul_transpose(const he_pnns_context* ctx, const W* matrix, size_t matrix_plaintext_count, size_t rows, size_t cols,
                  uint32_t baby_step, const W* queries, size_t query_count, const W* const* galois_keys, W* out,
                  bool to_single, he_stream s) {
    MatrixPlan plan;
    HEAMD_TRY_STATUS(response_plan<W>(ctx, matrix_plaintext_count, rows, cols, baby_step, plan));
    if (query_count == 0) return HE_OK;
    const heamd::BfvContext& bfv = heamd::bfv_impl(ctx->bfv);
    const size_t C = plan.plaintexts_per_column, Q = query_count;
    if (C > (size_t(1) << 24) || Q > (size_t(1) << 16)) return invalid_argument("too many result ciphertexts or queries");
    // rotatingColumns(by: -1) for the baby steps, (by: -babyStep) for the sum (MatrixMultiplication.swift:185,221-224)
    const bool need_one = plan.baby_step > 1, need_baby = plan.giant_step > 1;
    if (need_one || need_baby) {
        bool missing = galois_keys == nullptr || !bfv.has_key_switching();
        for (size_t q = 0; !missing && q < Q; ++q)
            missing = (need_one && galois_keys[2 * q] == nullptr) || (need_baby && galois_keys[2 * q + 1] == nullptr);
        if (missing) {
            heamd::set_last_error("no Galois key for a rotation mulTranspose needs");
            return HE_ERR_MISSING_GALOIS_KEY;
        }
    }
    HEAMD_TRY_STATUS(response_buffers<W>(ctx, matrix, queries, out));
    return bsgs_product(ctx, plan, matrix, queries, galois_keys, 2, Q, out, to_single, s);
}

// ---- mulTranspose(matrix:using:): query matrices of several rows ------------------------------------------------------------
// What extractDenseRow (CiphertextMatrix.swift:252-370) does to row `r` of an R-row dense-row packed query: the mask is 1 on
// slot i iff lower <= i < min(N, lower + copies period) and (i - lower) mod period < P; then `rotate_count` times "rotate the
// running copy by P and add it", then the row swap.
struct QueryRow {
    uint32_t lower, period, copies, rotate_count;
};
enum : uint32_t {  // he_pnns_query_matrix_shape's out_pack_needs: the slots of galois_keys, and the pack plan
    kNeedsOne = 1u << 0, kNeedsBaby = 1u << 1, kNeedsSwap = 1u << 2, kNeedsReplicate = 1u << 3, kNeedsPack = 1u << 4
};
struct QueryPlan {
    size_t padded_cols = 0, rows_per_ciphertext = 0, query_ciphertexts = 0, columns_per_simd_row = 0, result_ciphertexts = 0;
    uint32_t needs = 0;
    std::vector<QueryRow> rows;  // empty for a one-row query: extractDenseRow returns the ciphertext itself (:268-270)
};

// simdSlotIndices and rowCountInBatch restated line for line (:281-318), then reduced to the mask rule.  The closure reads the
// ciphertext index of the row being extracted, also where it is asked about another row, and the backward scan starts at
// rowIndex - 1: both are kept.
QueryRow query_row(size_t n, size_t padded_cols, size_t row_count, size_t row_index, size_t ciphertext_count) {
    const size_t simd_columns = n / 2;
    const size_t rows_per_ciphertext = 2 * (simd_columns / padded_cols);
    const size_t ciphertext_index = row_index / rows_per_ciphertext;
    auto slot_indices = [&](size_t index, size_t& lower, size_t& upper) {
        const size_t batch_start = (index % rows_per_ciphertext) * padded_cols;
        lower = batch_start;
        upper = batch_start + padded_cols;
        if (lower <= simd_columns && simd_columns < upper) {  // overflowsSimdRow
            lower = simd_columns;
            upper = simd_columns + padded_cols;
        } else if (upper > simd_columns) {
            const size_t padding = simd_columns % padded_cols;
            lower += padding;
            upper += padding;
        }
        if (ciphertext_index == ciphertext_count - 1)  // the last ciphertext pads until the end of the ciphertext
            upper = dividing_ceil(upper, simd_columns) * simd_columns;
    };
    size_t lower = 0, upper = 0, other_lower = 0, other_upper = 0;
    slot_indices(row_index, lower, upper);
    size_t last = row_index + 1;
    while (last < row_count && (slot_indices(last, other_lower, other_upper), other_upper == upper)) ++last;
    size_t first = row_index > 0 ? row_index - 1 : 0;
    while (first > 0 && (slot_indices(first, other_lower, other_upper), other_upper == upper)) --first;
    const size_t rows_in_batch = last - first;
    QueryRow row{};
    row.lower = static_cast<uint32_t>(lower);
    row.period = static_cast<uint32_t>(next_power_of_two(padded_cols * rows_in_batch));
    row.copies = static_cast<uint32_t>(dividing_ceil(upper - lower, row.period));  // while mask.count < upperBound: append
    row.rotate_count = static_cast<uint32_t>(simd_columns / (size_t(row.copies) * padded_cols) - 1);
    return row;
}

int query_plan(const he_pnns_context* ctx, size_t matrix_rows, size_t cols, size_t query_rows, uint32_t baby_step,
               uint32_t giant_step, QueryPlan& plan) {
    if (query_rows == 0) return invalid_argument("the query matrix has no rows");  // MatrixDimensions.init
    if (query_rows > (size_t(1) << 16)) return invalid_argument("too many query rows");
    const size_t n = ctx->plaintext->degree(), simd_columns = n / 2;
    plan = QueryPlan{};
    plan.padded_cols = next_power_of_two(cols);
    plan.rows_per_ciphertext = 2 * (simd_columns / plan.padded_cols);
    plan.query_ciphertexts = dividing_ceil(query_rows, plan.rows_per_ciphertext);
    plan.columns_per_simd_row = simd_columns / matrix_rows;
    plan.result_ciphertexts = plan.columns_per_simd_row > 0 ? dividing_ceil(query_rows, 2 * plan.columns_per_simd_row)
                                                            : query_rows * dividing_ceil(matrix_rows, n);
    bool replicate = false;
    if (query_rows > 1) {
        plan.rows.resize(query_rows);
        for (size_t r = 0; r < query_rows; ++r) {
            plan.rows[r] = query_row(n, plan.padded_cols, query_rows, r, plan.query_ciphertexts);
            replicate = replicate || plan.rows[r].rotate_count > 0;
        }
    }
    const size_t cps = plan.columns_per_simd_row;
    plan.needs = (baby_step > 1 ? kNeedsOne : 0u) | (giant_step > 1 ? kNeedsBaby : 0u) |
                 (query_rows > 1 || (cps > 0 && query_rows > cps) ? kNeedsSwap : 0u) | (replicate ? kNeedsReplicate : 0u) |
                 (cps >= 2 && query_rows >= 2 ? kNeedsPack : 0u);
    return HE_OK;
}

// Ciphertexts of (position, client): the rows of the clients' queries, later the half-chunks of their results.  A Galois call
// takes a key per ciphertext, so positions are the outer index and a run of positions over all clients is one contiguous batch.
template <typename W>
struct Grid {
    const he_pnns_context* ctx;
    size_t clients, ct;  // ct: words of a ciphertext
    uint32_t L;
    const std::vector<const W*>* tiled;  // [slot][position-major over clients], as many positions as any grid has
    size_t tiled_stride;
    he_stream s;

    // positions [first, first + count) of every client: out = in under the Galois element, with the clients' keys of `slot`
    int rotate(const W* in, W* out, uint64_t element, size_t slot, size_t first, size_t count) const {
        if (count == 0) return HE_OK;
        return apply_galois(ctx->bfv, L, in + first * clients * ct, element, tiled->data() + slot * tiled_stride, 1,
                            count * clients, 1, out + first * clients * ct, s);
    }
    // lhs positions [first, first + count) += rhs positions [rhs_first, ..)
    int add(const he_poly_context* ring, W* lhs, size_t first, const W* rhs, size_t rhs_first, size_t count) const {
        if (count == 0) return HE_OK;
        return heamd::poly_elementwise(ring, heamd::ElementwiseOp::Add, lhs + first * clients * ct, rhs + rhs_first * clients * ct,
                                       count * clients * 2, as_stream(s));
    }
    // dst positions [first, first + count) = src positions [src_first, ..)
    hipError_t copy(W* dst, size_t first, const W* src, size_t src_first, size_t count) const {
        if (count == 0) return hipSuccess;
        return hipMemcpyAsync(dst + first * clients * ct, src + src_first * clients * ct, count * clients * ct * sizeof(W),
                              hipMemcpyDeviceToDevice, as_stream(s));
    }
};

// src: `unit` words per (position, client) in the layout of Grid; position `from` of every client goes to
// dst [clients][dst_positions][unit] at `to`
template <typename W>
hipError_t to_client_major(W* dst, size_t dst_positions, size_t to, const W* src, size_t from, size_t clients, size_t unit,
                           hipStream_t stream) {
    return hipMemcpy2DAsync(dst + to * unit, dst_positions * unit * sizeof(W), src + from * clients * unit, unit * sizeof(W),
                            unit * sizeof(W), clients, hipMemcpyDeviceToDevice, stream);
}

template <typename W>
int mul_transpose_matrix(const he_pnns_context* ctx, const W* matrix, size_t matrix_plaintext_count, size_t rows, size_t cols,
                         uint32_t baby_step, const W* queries, size_t query_rows, size_t query_count,
                         const he_pnns_pack_step* pack_steps, size_t pack_step_count, const W* const* galois_keys, W* out,
                         bool to_single, he_stream s) {
    MatrixPlan plan;
    HEAMD_TRY_STATUS(response_plan<W>(ctx, matrix_plaintext_count, rows, cols, baby_step, plan));
    QueryPlan query;
    HEAMD_TRY_STATUS(query_plan(ctx, rows, cols, query_rows, plan.baby_step, plan.giant_step, query));
    if (query_count == 0) return HE_OK;
    const heamd::BfvContext& bfv = heamd::bfv_impl(ctx->bfv);
    const size_t n = bfv.degree(), C = plan.plaintexts_per_column, Q = query_count, R = query_rows, V = Q * R;
    const size_t P = plan.padded_cols, K = query.query_ciphertexts, cps = query.columns_per_simd_row;
    const size_t M = query.result_ciphertexts;
    const uint32_t L = bfv.top_level();
    if (C > (size_t(1) << 24) || V > (size_t(1) << 16)) return invalid_argument("too many result ciphertexts or query rows");
    // the plan rotateColumnsMultiStep(by: rows) executes, in the caller's order
    const bool packs = (query.needs & kNeedsPack) != 0;
    const size_t key_stride = 4 + pack_step_count;  // the caller's array, whether or not the plan is read
    if (!packs) pack_step_count = 0;
    if (packs) {
        if (pack_steps == nullptr || pack_step_count == 0) return invalid_argument("the packing needs a rotation plan");
        if (pack_step_count > 64) return invalid_argument("rotation plan too long");
        uint64_t total = 0;
        for (size_t i = 0; i < pack_step_count; ++i) {
            if (pack_steps[i].step < 1 || pack_steps[i].step > static_cast<int64_t>(n / 2) - 1)
                return invalid_argument("a step of the rotation plan is outside [1, N / 2 - 1]");
            total = (total + static_cast<uint64_t>(pack_steps[i].step) * pack_steps[i].count) % (n / 2);
        }
        if (total != rows % (n / 2)) return invalid_argument("the rotation plan does not rotate by the matrix's row count");
    }
    {
        bool missing = false;
        if (query.needs != 0) {
            missing = galois_keys == nullptr || !bfv.has_key_switching();
            for (size_t q = 0; !missing && q < Q; ++q) {
                for (size_t slot = 0; slot < 4; ++slot)
                    missing = missing || ((query.needs >> slot) & 1u && galois_keys[q * key_stride + slot] == nullptr);
                for (size_t i = 0; i < pack_step_count; ++i)
                    missing = missing || (pack_steps[i].count != 0 && galois_keys[q * key_stride + 4 + i] == nullptr);
            }
        }
        if (missing) {
            heamd::set_last_error("no Galois key for a rotation mulTranspose(matrix:) needs");
            return HE_ERR_MISSING_GALOIS_KEY;
        }
    }
    HEAMD_TRY_STATUS(response_buffers<W>(ctx, matrix, queries, out));
    if (R == 1)  // one row: the vector's own ciphertext, and rotateColumnsAndSum of one element
        return bsgs_product(ctx, plan, matrix, queries, galois_keys, key_stride, Q, out, to_single, s);
    if (reinterpret_cast<uintptr_t>(queries) % 16 != 0) return invalid_argument("the queries must be 16-byte aligned");
    HEAMD_TRY_STATUS(ctx->plaintext->check_device());
    const heamd::PolyContext* q_ctx = bfv.ciphertext(L);
    const he_poly_context* ring = he_bfv_ciphertext_context(ctx->bfv, L);
    hipStream_t stream = as_stream(s);
    const size_t poly = size_t(L) * n, ct = 2 * poly, ct_bytes = ct * sizeof(W);

    // the rows in the order of their replication steps, longest first: the rows of step i are a prefix
    std::vector<uint32_t> row_of(R), position_of(R);
    for (size_t r = 0; r < R; ++r) row_of[r] = static_cast<uint32_t>(r);
    std::stable_sort(row_of.begin(), row_of.end(), [&](uint32_t a, uint32_t b) {
            return query.rows[a].rotate_count > query.rows[b].rotate_count;
        });
    for (size_t k = 0; k < R; ++k) position_of[row_of[k]] = static_cast<uint32_t>(k);
    const size_t halves = cps > 0 ? dividing_ceil(R, cps) : 0;
    const size_t most_positions = R > halves ? R : halves;
    // [slot][position][client]: the key of `slot` for every ciphertext of a batch (several rows need the swap: there are keys)
    std::vector<const W*> tiled(key_stride * most_positions * Q);
    for (size_t slot = 0; slot < key_stride; ++slot)
        for (size_t v = 0; v < most_positions * Q; ++v)
            tiled[slot * most_positions * Q + v] = galois_keys[(v % Q) * key_stride + slot];
    Grid<W> grid{ctx, Q, ct, L, &tiled, most_positions * Q, s};

    Scratch rows_mem(stream);
    HEAMD_HIP_TRY(rows_mem.allocate(V * ct_bytes));
    W* extracted = static_cast<W*>(rows_mem.get());  // the grid of extracted rows
    {
        // 1) the masks (:323-338), once for all clients: slot patterns into the [t] slabs, inverse NTT, to Eval at the top level
        Scratch staging_mem(stream), masks_mem(stream), eval_mem(stream), copies_mem(stream);
        HEAMD_HIP_TRY(staging_mem.allocate(R * n * sizeof(W)));
        HEAMD_HIP_TRY(masks_mem.allocate(R * poly * sizeof(W)));
        W* staging = static_cast<W*>(staging_mem.get());
        W* masks = static_cast<W*>(masks_mem.get());
        std::vector<heamd::PnnsRowMask> patterns(R);
        for (size_t r = 0; r < R; ++r) patterns[r] = heamd::PnnsRowMask{query.rows[r].lower, query.rows[r].period, query.rows[r].copies};
        HEAMD_HIP_TRY(heamd::launch_pnns_row_masks<W>(ctx->slot_of_word_device, patterns.data(), R, static_cast<uint32_t>(P),
                                                       ctx->plaintext->log_degree(), staging, stream));
        HEAMD_HIP_TRY(ntt_rows(true, staging, *ctx->plaintext, ctx->plaintext->device_context(), 1, R, stream));
        HEAMD_TRY_STATUS(heamd::bfv_plaintext_to_eval(ctx->bfv, L, staging, masks, R, stream));
        // 2) every query ciphertext to Eval once; each is read once for all the rows packed in it (:340-342)
        HEAMD_HIP_TRY(eval_mem.allocate(Q * K * ct_bytes));
        W* eval = static_cast<W*>(eval_mem.get());
        HEAMD_HIP_TRY(hipMemcpyAsync(eval, queries, Q * K * ct_bytes, hipMemcpyDeviceToDevice, stream));
        HEAMD_TRY_STATUS(heamd::poly_ntt(ring, eval, Q * K * 2, false, stream));
        heamd::PnnsExtractLayout layout{};
        layout.clients = Q;
        layout.query_ciphertexts = K;
        const heamd::DeviceContext dc = q_ctx->device_context(L);
        for (size_t k = 0; k < K; ++k) {
            const size_t first = k * query.rows_per_ciphertext;
            const size_t count = R - first < query.rows_per_ciphertext ? R - first : query.rows_per_ciphertext;
            HEAMD_HIP_TRY(heamd::launch_pnns_extract_rows<W>(eval, masks, extracted, dc, layout, static_cast<uint32_t>(k),
                                                              static_cast<uint32_t>(first), position_of.data() + first, count,
                                                              stream));
        }
        HEAMD_TRY_STATUS(heamd::poly_ntt(ring, extracted, V * 2, true, stream));
        // 3) replication over a SIMD row (:347-353), then both SIMD rows (:358-361)
        HEAMD_HIP_TRY(copies_mem.allocate(2 * V * ct_bytes));
        W* ahead = static_cast<W*>(copies_mem.get());
        W* behind = ahead + V * ct;
        const uint32_t most = query.rows[row_of[0]].rotate_count;
        uint64_t element_columns = 0, element_swap = 0;
        if (most > 0) HEAMD_TRY_STATUS(he_galois_element_rotating_columns(static_cast<int64_t>(P), n, &element_columns));
        HEAMD_TRY_STATUS(he_galois_element_swapping_rows(n, &element_swap));
        const W* running = extracted;
        size_t live = R;
        for (uint32_t step = 0; step < most; ++step) {
            while (query.rows[row_of[live - 1]].rotate_count <= step) --live;
            HEAMD_TRY_STATUS(grid.rotate(running, ahead, element_columns, 3, 0, live));
            HEAMD_TRY_STATUS(grid.add(ring, extracted, 0, ahead, 0, live));
            running = ahead;
            std::swap(ahead, behind);
        }
        HEAMD_TRY_STATUS(grid.rotate(extracted, ahead, element_swap, 2, 0, R));
        HEAMD_TRY_STATUS(grid.add(ring, extracted, 0, ahead, 0, R));
    }

    // 4) mulTranspose(vector:) of every row: the rows share the passes over the matrix
    std::vector<const W*> pairs(2 * V);
    for (size_t v = 0; v < V; ++v) {
        pairs[2 * v] = galois_keys[(v % Q) * key_stride];
        pairs[2 * v + 1] = galois_keys[(v % Q) * key_stride + 1];
    }
    Scratch results_mem(stream), single_mem(stream);
    HEAMD_HIP_TRY(results_mem.allocate(V * C * ct_bytes));
    W* results = static_cast<W*>(results_mem.get());  // the grid of [C] results
    HEAMD_TRY_STATUS(bsgs_product<W>(ctx, plan, matrix, extracted, pairs.data(), 2, V, results, false, s));
    const size_t out_ct = to_single ? 2 * n : ct;
    if (cps == 0) {  // no packing: innerProducts is every row's C results, in row order (:265)
        const W* source = results;
        if (to_single) {
            HEAMD_HIP_TRY(single_mem.allocate(V * C * out_ct * sizeof(W)));
            HEAMD_TRY_STATUS(heamd::bfv_mod_switch_down_to_single(ctx->bfv, L, 2, results,
                                                                  static_cast<W*>(single_mem.get()), V * C, stream));
            source = static_cast<const W*>(single_mem.get());
        }
        for (size_t r = 0; r < R; ++r)
            HEAMD_HIP_TRY(to_client_major(out, R, r, source, position_of[r], Q, C * out_ct, stream));
        return HE_OK;
    }

    // 5) the dense-column packing (:267-290), C = 1.  Half-chunk j holds the results of rows [j cps, (j + 1) cps); the halves of
    //    the last one's parity lie behind the others, so the one half that may be short is the last position, and the second
    //    halves of the chunks are one run.
    const size_t last_parity = (halves - 1) & 1, before = last_parity == 1 ? (halves + 1) / 2 : halves / 2;
    auto half_position = [&](size_t j) { return ((j & 1) == last_parity ? before : 0) + (j >> 1); };
    const size_t last_length = R - (halves - 1) * cps;
    Grid<W> sums{ctx, Q, ct, L, &tiled, most_positions * Q, s};
    Scratch sums_mem(stream);
    HEAMD_HIP_TRY(sums_mem.allocate(2 * halves * Q * ct_bytes));
    W* current = static_cast<W*>(sums_mem.get());
    W* other = current + halves * Q * ct;
    std::vector<uint64_t> elements(pack_step_count);
    for (size_t i = 0; i < pack_step_count; ++i)
        HEAMD_TRY_STATUS(he_galois_element_rotating_columns(pack_steps[i].step, n, &elements[i]));
    for (size_t j = 0; j < halves; ++j) {  // the accumulator is the half's last element (HeScheme.swift:118)
        const size_t length = j + 1 < halves ? cps : last_length;
        HEAMD_HIP_TRY(sums.copy(current, half_position(j), results, position_of[j * cps + length - 1], 1));
    }
    size_t live = halves;
    W* short_half = nullptr;  // where the short half's sum was when it ran out of elements
    for (size_t step = 0; step + 1 < cps && live > 0; ++step) {
        if (live == halves && last_length - 1 <= step) {
            short_half = current;
            --live;
            if (live == 0) break;
        }
        for (size_t i = 0; i < pack_step_count; ++i)
            for (uint32_t repeat = 0; repeat < pack_steps[i].count; ++repeat) {
                HEAMD_TRY_STATUS(sums.rotate(current, other, elements[i], 4 + i, 0, live));
                std::swap(current, other);
            }
        for (size_t j = 0; j < halves; ++j) {
            if (half_position(j) >= live) continue;
            const size_t length = j + 1 < halves ? cps : last_length;
            HEAMD_TRY_STATUS(sums.add(ring, current, half_position(j), results, position_of[j * cps + length - 2 - step], 1));
        }
    }
    if (short_half != nullptr && short_half != current) HEAMD_HIP_TRY(sums.copy(current, halves - 1, short_half, halves - 1, 1));
    // swapRowsAndAdd (:281-286, HeScheme.swift:143-151): the second half's sum is swapped, the first half's added to it
    const size_t seconds = halves / 2;
    const size_t second_first = half_position(1 < halves ? 1 : 0), first_first = half_position(0);
    if (seconds > 0) {
        uint64_t element_swap = 0;
        HEAMD_TRY_STATUS(he_galois_element_swapping_rows(n, &element_swap));
        HEAMD_TRY_STATUS(sums.rotate(current, other, element_swap, 2, second_first, seconds));
        HEAMD_TRY_STATUS(sums.add(ring, other, second_first, current, first_first, seconds));
    }
    // 6) the M packed ciphertexts of every client, through modSwitchDownToSingle for the response
    W* packed = out;
    if (to_single) {
        HEAMD_HIP_TRY(single_mem.allocate(Q * M * ct_bytes));
        packed = static_cast<W*>(single_mem.get());
    }
    for (size_t m = 0; m < M; ++m) {
        const bool whole = m < seconds;
        HEAMD_HIP_TRY(to_client_major(packed, M, m, whole ? other : current, (whole ? second_first : first_first) + m, Q, ct,
                                      stream));
    }
    if (to_single) {
        HEAMD_TRY_STATUS(heamd::bfv_mod_switch_down_to_single(ctx->bfv, L, 2, packed, out, Q * M, stream));
    }
    return HE_OK;
}

}  // namespace

extern "C" int he_pnns_context_create(const he_bfv_context* ctx, he_pnns_context** out) { return pnns_create(ctx, 64, out); }

extern "C" int he_pnns_context_create_u32(const he_bfv_context* ctx, he_pnns_context** out) {
    return pnns_create(ctx, 32, out);
}

extern "C" void he_pnns_context_destroy(he_pnns_context* ctx) {
    heamd::RelaxedCapture relaxed;
    delete ctx;
}

extern "C" int he_pnns_matrix_shape(const he_pnns_context* ctx, size_t row_count, size_t column_count, int packing,
                                    uint32_t baby_step, size_t* out_plaintext_count, uint32_t* out_baby_step,
                                    uint32_t* out_giant_step) {
    MatrixPlan plan;
    const int status = matrix_plan(ctx, row_count, column_count, packing, baby_step, plan);
    if (status != HE_OK) return status;
    if (out_plaintext_count != nullptr) *out_plaintext_count = plan.plaintext_count;
    if (out_baby_step != nullptr) *out_baby_step = plan.baby_step;
    if (out_giant_step != nullptr) *out_giant_step = plan.giant_step;
    return HE_OK;
}

extern "C" int he_pnns_quantize_rows_device(const float* vectors, size_t rows, size_t cols, float scaling_factor,
                                            int64_t* out, he_stream s) {
    if (rows == 0 || cols == 0) return HE_OK;
    if (vectors == nullptr || out == nullptr) return invalid_argument("null buffer");
    if (rows > (size_t(1) << 40) || cols > (size_t(1) << 40)) return invalid_argument("matrix too large");
    HEAMD_HIP_TRY(heamd::launch_pnns_quantize_rows(vectors, rows, cols, scaling_factor, out, as_stream(s)));
    return HE_OK;
}

extern "C" int he_pnns_diagonal_matrix_device(const he_pnns_context* ctx, const int64_t* signed_values, size_t rows,
                                              size_t cols, uint32_t baby_step, int reduce, uint32_t moduli_count,
                                              uint64_t* out, uint32_t* out_of_range, he_stream s) {
    return diagonal_matrix(ctx, signed_values, rows, cols, baby_step, reduce, moduli_count, out, out_of_range, s);
}

extern "C" int he_pnns_diagonal_matrix_device_u32(const he_pnns_context* ctx, const int64_t* signed_values, size_t rows,
                                                  size_t cols, uint32_t baby_step, int reduce, uint32_t moduli_count,
                                                  uint32_t* out, uint32_t* out_of_range, he_stream s) {
    return diagonal_matrix(ctx, signed_values, rows, cols, baby_step, reduce, moduli_count, out, out_of_range, s);
}

extern "C" int he_pnns_mul_transpose_device(const he_pnns_context* ctx, const uint64_t* matrix, size_t matrix_plaintext_count,
                                            size_t rows, size_t cols, uint32_t baby_step, const uint64_t* queries,
                                            size_t query_count, const uint64_t* const* galois_keys, uint64_t* out,
                                            he_stream s) {
    return mul_transpose(ctx, matrix, matrix_plaintext_count, rows, cols, baby_step, queries, query_count, galois_keys,
                                out, false, s);
}

extern "C" int he_pnns_mul_transpose_device_u32(const he_pnns_context* ctx, const uint32_t* matrix,
                                                size_t matrix_plaintext_count, size_t rows, size_t cols, uint32_t baby_step,
                                                const uint32_t* queries, size_t query_count,
                                                const uint32_t* const* galois_keys, uint32_t* out, he_stream s) {
    return mul_transpose(ctx, matrix, matrix_plaintext_count, rows, cols, baby_step, queries, query_count, galois_keys,
                                out, false, s);
}

extern "C" int he_pnns_compute_response_device(const he_pnns_context* ctx, const uint64_t* matrix,
                                               size_t matrix_plaintext_count, size_t rows, size_t cols, uint32_t baby_step,
                                               const uint64_t* queries, size_t query_count,
                                               const uint64_t* const* galois_keys, uint64_t* out, he_stream s) {
    return mul_transpose(ctx, matrix, matrix_plaintext_count, rows, cols, baby_step, queries, query_count, galois_keys,
                                out, true, s);
}

extern "C" int he_pnns_compute_response_device_u32(const he_pnns_context* ctx, const uint32_t* matrix,
                                                   size_t matrix_plaintext_count, size_t rows, size_t cols, uint32_t baby_step,
                                                   const uint32_t* queries, size_t query_count,
                                                   const uint32_t* const* galois_keys, uint32_t* out, he_stream s) {
    return mul_transpose(ctx, matrix, matrix_plaintext_count, rows, cols, baby_step, queries, query_count, galois_keys,
                                out, true, s);
}

extern "C" int he_pnns_query_matrix_shape(const he_pnns_context* ctx, size_t matrix_rows, size_t cols, size_t query_rows,
                                          size_t* out_query_ciphertexts, size_t* out_result_ciphertexts,
                                          uint32_t* out_pack_needs) {
    MatrixPlan plan;
    const int status = matrix_plan(ctx, matrix_rows, cols, HE_PNNS_PACKING_DIAGONAL, 0, plan);
    if (status != HE_OK) return status;
    QueryPlan query;
    const int planned = query_plan(ctx, matrix_rows, cols, query_rows, plan.baby_step, plan.giant_step, query);
    if (planned != HE_OK) return planned;
    if (out_query_ciphertexts != nullptr) *out_query_ciphertexts = query.query_ciphertexts;
    if (out_result_ciphertexts != nullptr) *out_result_ciphertexts = query.result_ciphertexts;
    if (out_pack_needs != nullptr) *out_pack_needs = query.needs;
    return HE_OK;
}

#define HEAMD_PNNS_MATRIX_ENTRY(NAME, WORD, TO_SINGLE)                                                                        \
    extern "C" int NAME(const he_pnns_context* ctx, const WORD* matrix, size_t matrix_plaintext_count, size_t rows, size_t cols, \
                        uint32_t baby_step, const WORD* queries, size_t query_rows, size_t query_count,                        \
                        const he_pnns_pack_step* pack_steps, size_t pack_step_count, const WORD* const* galois_keys, WORD* out, \
                        he_stream s) {                                                                                         \
        return mul_transpose_matrix(ctx, matrix, matrix_plaintext_count, rows, cols, baby_step, queries, query_rows,           \
                                    query_count, pack_steps, pack_step_count, galois_keys, out, TO_SINGLE, s);                 \
    }
HEAMD_PNNS_MATRIX_ENTRY(he_pnns_mul_transpose_matrix_device, uint64_t, false)
HEAMD_PNNS_MATRIX_ENTRY(he_pnns_mul_transpose_matrix_device_u32, uint32_t, false)
HEAMD_PNNS_MATRIX_ENTRY(he_pnns_compute_response_matrix_device, uint64_t, true)
HEAMD_PNNS_MATRIX_ENTRY(he_pnns_compute_response_matrix_device_u32, uint32_t, true)
#undef HEAMD_PNNS_MATRIX_ENTRY
