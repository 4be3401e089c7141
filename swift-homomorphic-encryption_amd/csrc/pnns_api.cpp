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
// transforms, additions and the mod-switch are the library's own entry points, batched over the queries; the one kernel of its
// own is the pass over the matrix (pnns_kernels.hip, pnns_bsgs_inner_product_kernel).
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <vector>

#include "api_internal.hpp"
#include "bfv_context.hpp"
#include "kernels.hpp"

using heamd::as_stream;
using heamd::invalid_argument;
using heamd::Scratch;

#define HEAMD_TRY_STATUS(expr)                \
    do {                                      \
        const int status_ = (expr);           \
        if (status_ != HE_OK) return status_; \
    } while (0)

// Opaque handle of include/he_amd.h
struct he_pnns_context {
    const he_bfv_context* bfv = nullptr;          // borrowed
    std::unique_ptr<heamd::PolyContext> plaintext;  // plaintextContext: [t]
    std::vector<uint32_t> encoding_matrix;        // simdEncodingMatrix: slot -> slab word
    uint32_t* slot_of_word_device = nullptr;      // its inverse, on the device
    ~he_pnns_context() {
        if (slot_of_word_device != nullptr) (void)hipFree(slot_of_word_device);
    }
};

namespace {

size_t next_power_of_two(size_t x) {
    size_t p = 1;
    while (p < x) p <<= 1;
    return p;
}
size_t dividing_ceil(size_t a, size_t b) { return (a + b - 1) / b; }

struct MatrixPlan {
    size_t plaintext_count = 0, padded_cols = 0, plaintexts_per_column = 0;
    uint32_t baby_step = 0, giant_step = 0;
};

// PlaintextMatrix.plaintextCount (PlaintextMatrix.swift:246-275) and BabyStepGiantStep.init (MatrixMultiplication.swift:33-60)
int matrix_plan(const he_pnns_context* ctx, size_t rows, size_t cols, int packing, uint32_t baby_step, MatrixPlan& plan) {
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
        std::vector<uint32_t> slot_of_word(bfv.degree());
        for (uint32_t slot = 0; slot < bfv.degree(); ++slot) slot_of_word[ctx->encoding_matrix[slot]] = slot;
        const size_t bytes = slot_of_word.size() * sizeof(uint32_t);
        HEAMD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&ctx->slot_of_word_device), bytes));
        HEAMD_HIP_TRY(hipMemcpy(ctx->slot_of_word_device, slot_of_word.data(), bytes, hipMemcpyHostToDevice));
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

int inverse_ntt(const heamd::PolyContext& ring, uint64_t* slabs, size_t count, hipStream_t stream) {
    HEAMD_HIP_TRY(heamd::launch_ntt(true, slabs, ring.device_context(), 0, 1, count, stream));
    return HE_OK;
}
int inverse_ntt(const heamd::PolyContext& ring, uint32_t* slabs, size_t count, hipStream_t stream) {
    heamd::DeviceContext32 dc{};
    const int status = ring.device_context32(1, dc);
    if (status != HE_OK) return status;
    HEAMD_HIP_TRY(heamd::launch_ntt32(true, slabs, dc, 0, 1, count, stream));
    return HE_OK;
}
int to_eval(const he_bfv_context* ctx, uint32_t L, const uint64_t* staging, uint64_t* out, size_t batch, he_stream s) {
    return he_bfv_plaintext_to_eval_device(ctx, L, staging, out, batch, s);
}
int to_eval(const he_bfv_context* ctx, uint32_t L, const uint32_t* staging, uint32_t* out, size_t batch, he_stream s) {
    return he_bfv_plaintext_to_eval_device_u32(ctx, L, staging, out, batch, s);
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
    const int ready = to_eval(ctx->bfv, moduli_count, static_cast<const W*>(nullptr), static_cast<W*>(nullptr), 0, s);
    if (ready != HE_OK) return ready;
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
        const int inverted = inverse_ntt(ring, staging, count, stream);
        if (inverted != HE_OK) return inverted;
        const int converted = to_eval(ctx->bfv, moduli_count, staging, out + first * moduli_count * n, count, s);
        if (converted != HE_OK) return converted;
    }
    return HE_OK;
}

// ---- mulTranspose(vector:using:) and computeResponse ---------------------------------------------------------------------------
// The library's entry points by word size.  rotate: `groups` runs of `group_size` ciphertexts, run g under keys[g * key_stride].
struct Ops64 {
    using Word = uint64_t;
    static int rotate(const he_bfv_context* ctx, uint32_t L, const Word* in, uint64_t element, const Word* const* keys,
                      size_t key_stride, size_t groups, size_t group_size, Word* out, he_stream s) {
        std::vector<const Word*> per_group(groups);
        for (size_t g = 0; g < groups; ++g) per_group[g] = keys[g * key_stride];
        return he_bfv_apply_galois_grouped_device(ctx, L, in, element, per_group.data(), groups, group_size, out, nullptr, 0, s);
    }
    static int forward_ntt(const he_poly_context* ring, Word* slab, size_t polys, he_stream s) {
        return he_ntt_forward_device(ring, slab, polys, s);
    }
    static int inverse_ntt(const he_poly_context* ring, Word* slab, size_t polys, he_stream s) {
        return he_ntt_inverse_device(ring, slab, polys, s);
    }
    static int add(const he_poly_context* ring, Word* lhs, const Word* rhs, size_t polys, he_stream s) {
        return he_poly_add_device(ring, lhs, rhs, polys, s);
    }
    static int to_single(const he_bfv_context* ctx, uint32_t L, const Word* in, Word* out, size_t batch, Word*, he_stream s) {
        return he_bfv_mod_switch_down_to_single_device(ctx, L, 2, in, out, batch, s);
    }
    static size_t to_single_scratch_words(uint32_t, size_t, size_t) { return 0; }
};
struct Ops32 {
    using Word = uint32_t;
    static int rotate(const he_bfv_context* ctx, uint32_t L, const Word* in, uint64_t element, const Word* const* keys,
                      size_t key_stride, size_t groups, size_t group_size, Word* out, he_stream s) {
        const size_t ct = 2 * size_t(L) * heamd::bfv_impl(ctx).degree();
        for (size_t g = 0; g < groups; ++g) {  // the 4-byte Galois entry takes one key per call
            const int status = he_bfv_apply_galois_device_u32(ctx, L, in + g * group_size * ct, element, keys[g * key_stride],
                                                              out + g * group_size * ct, group_size, nullptr, 0, s);
            if (status != HE_OK) return status;
        }
        return HE_OK;
    }
    static int forward_ntt(const he_poly_context* ring, Word* slab, size_t polys, he_stream s) {
        return he_ntt_forward_device_u32(ring, slab, polys, s);
    }
    static int inverse_ntt(const he_poly_context* ring, Word* slab, size_t polys, he_stream s) {
        return he_ntt_inverse_device_u32(ring, slab, polys, s);
    }
    static int add(const he_poly_context* ring, Word* lhs, const Word* rhs, size_t polys, he_stream s) {
        return he_poly_add_device_u32(ring, lhs, rhs, polys, s);
    }
    // the chain of he_bfv_mod_switch_down_device_u32 through two slabs of `level_words` words
    static int to_single(const he_bfv_context* ctx, uint32_t L, const Word* in, Word* out, size_t batch, Word* levels,
                         he_stream s) {
        const size_t n = heamd::bfv_impl(ctx).degree();
        if (L == 1) {
            HEAMD_HIP_TRY(hipMemcpyAsync(out, in, batch * 2 * n * sizeof(Word), hipMemcpyDeviceToDevice, as_stream(s)));
            return HE_OK;
        }
        Word* ping = levels;
        Word* pong = levels + batch * 2 * size_t(L - 1) * n;
        const Word* source = in;
        for (uint32_t level = L; level > 1; --level) {
            Word* step = level == 2 ? out : (source == ping ? pong : ping);
            const int status = he_bfv_mod_switch_down_device_u32(ctx, level, 2, source, step, batch, s);
            if (status != HE_OK) return status;
            source = step;
        }
        return HE_OK;
    }
    static size_t to_single_scratch_words(uint32_t L, size_t batch, size_t n) {
        return L > 2 ? 2 * batch * 2 * size_t(L - 1) * n : 0;
    }
};

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

template <typename Ops>
int mul_transpose(const he_pnns_context* ctx, const typename Ops::Word* matrix, size_t matrix_plaintext_count, size_t rows,
                  size_t cols, uint32_t baby_step, const typename Ops::Word* queries, size_t query_count,
                  const typename Ops::Word* const* galois_keys, typename Ops::Word* out, bool to_single, he_stream s) {
    using W = typename Ops::Word;
    if (ctx == nullptr) return invalid_argument("null context");
    if (baby_step == 0) return invalid_argument("baby_step must be the one the matrix was packed with");
    MatrixPlan plan;
    const int planned = matrix_plan(ctx, rows, cols, HE_PNNS_PACKING_DIAGONAL, baby_step, plan);
    if (planned != HE_OK) return planned;
    if (matrix_plaintext_count != plan.plaintext_count)  // PnnsError.invalidMatrixDimensions, MatrixMultiplication.swift:147-149
        return invalid_argument("the matrix does not hold nextPowerOfTwo(cols) x ceil(rows / N) plaintexts");
    const heamd::BfvContext& bfv = heamd::bfv_impl(ctx->bfv);
    if (bfv.word_bits() != 8 * sizeof(W)) return invalid_argument("context of the other word size");
    if (query_count == 0) return HE_OK;
    const uint32_t b = plan.baby_step, G = plan.giant_step, L = bfv.top_level();
    const size_t n = bfv.degree(), C = plan.plaintexts_per_column, Q = query_count;
    if (C > (size_t(1) << 24) || Q > (size_t(1) << 16)) return invalid_argument("too many result ciphertexts or queries");
    // rotatingColumns(by: -1) for the baby steps, (by: -babyStep) for the sum (MatrixMultiplication.swift:185,221-224)
    const bool need_one = b > 1, need_baby = G > 1;
    if (need_one || need_baby) {
        bool missing = galois_keys == nullptr || !bfv.has_key_switching();
        for (size_t q = 0; !missing && q < Q; ++q)
            missing = (need_one && galois_keys[2 * q] == nullptr) || (need_baby && galois_keys[2 * q + 1] == nullptr);
        if (missing) {
            heamd::set_last_error("no Galois key for a rotation mulTranspose needs");
            return HE_ERR_MISSING_GALOIS_KEY;
        }
    }
    if (matrix == nullptr || queries == nullptr || out == nullptr) return invalid_argument("null buffer");
    if (reinterpret_cast<uintptr_t>(matrix) % 16 != 0) return invalid_argument("the matrix must be 16-byte aligned");
    if (n < 16 / sizeof(W)) return invalid_argument("degree below one 16-byte access");
    const heamd::PolyContext* q_ctx = bfv.ciphertext(L);
    const int on_device = q_ctx->check_device();
    if (on_device != HE_OK) return on_device;
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
        HEAMD_TRY_STATUS(Ops::rotate(ctx->bfv, L, rot + size_t(j - 1) * Q * ct, element_one, galois_keys, 2, Q, 1,
                                     rot + size_t(j) * Q * ct, s));
    HEAMD_TRY_STATUS(Ops::forward_ntt(ring, rot, size_t(b) * Q * 2, s));

    heamd::PnnsBsgsLayout layout{};
    layout.rot_step_words = Q * ct;
    layout.log_degree = q_ctx->log_degree();
    layout.moduli_count = L;
    layout.baby_step = b;
    layout.giant_step = G;
    layout.padded_cols = static_cast<uint32_t>(plan.padded_cols);
    layout.columns = static_cast<uint32_t>(C);
    layout.out_queries = static_cast<uint32_t>(Q);
    layout.max_lazy = q_ctx->max_lazy_product_accumulation_count(L);
    layout.cadence = layout.max_lazy;
    layout.narrow_moduli = true;
    for (uint32_t i = 0; i < L; ++i) {  // as he_bfv_inner_product_plain_device: sums of the carry-counting accumulator below 2^127
        layout.narrow_moduli = layout.narrow_moduli && (q_ctx->moduli()[i] >> 56) == 0;
        const unsigned __int128 below = q_ctx->moduli()[i] - 1;
        if (below == 0) continue;
        const unsigned __int128 limit = ((static_cast<unsigned __int128>(1) << 127) - q_ctx->moduli()[i]) / (below * below);
        if (limit < layout.cadence) layout.cadence = static_cast<uint64_t>(limit);
    }
    const unsigned per_pass = heamd::pnns_bsgs_queries_per_pass(layout, sizeof(W), Q);
    const heamd::DeviceContext dc = q_ctx->device_context(L);

    const size_t group = response_group(C, Q, G, ct_bytes);
    const size_t out_ct = to_single ? 2 * n : ct;  // words of a result ciphertext in `out`
    Scratch products_mem(stream), sums_mem(stream), levels_mem(stream);
    HEAMD_HIP_TRY(products_mem.allocate(Q * G * group * ct_bytes));
    HEAMD_HIP_TRY(sums_mem.allocate(2 * Q * group * ct_bytes));
    const size_t level_words = to_single ? Ops::to_single_scratch_words(L, Q * group, n) : 0;
    if (level_words != 0) HEAMD_HIP_TRY(levels_mem.allocate(level_words * sizeof(W)));
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
        HEAMD_TRY_STATUS(Ops::inverse_ntt(ring, products, Q * G * now * 2, s));
        // 3) rotateColumnsAndSum (HeScheme.swift:113-133): the last giant step's product, then per earlier one rotate by
        //    -babyStep and add it; every step one key switch and one addition over the Q x now accumulators.  The products are
        //    giant-step major, so the last step's slab is the first accumulator where it lies.
        W* current = products + size_t(G - 1) * Q * now * ct;
        W* other = sums;
        for (uint32_t g = G - 1; g-- > 0;) {
            HEAMD_TRY_STATUS(Ops::rotate(ctx->bfv, L, current, element_baby, galois_keys + 1, 2, Q, now, other, s));
            HEAMD_TRY_STATUS(Ops::add(ring, other, products + size_t(g) * Q * now * ct, Q * now * 2, s));
            current = other;
            other = current == sums ? sums + Q * now * ct : sums;
        }
        // 4) the group's results to their places in out [Q][C]; computeResponse: through modSwitchDownToSingle (Server.swift:84)
        if (to_single && now == C) {
            HEAMD_TRY_STATUS(Ops::to_single(ctx->bfv, L, current, out, Q * C, static_cast<W*>(levels_mem.get()), s));
        } else if (to_single) {
            HEAMD_TRY_STATUS(Ops::to_single(ctx->bfv, L, current, other, Q * now, static_cast<W*>(levels_mem.get()), s));
            HEAMD_HIP_TRY(hipMemcpy2DAsync(out + first * out_ct, C * out_ct * sizeof(W), other, now * out_ct * sizeof(W),
                                           now * out_ct * sizeof(W), Q, hipMemcpyDeviceToDevice, stream));
        } else {
            HEAMD_HIP_TRY(hipMemcpy2DAsync(out + first * out_ct, C * out_ct * sizeof(W), current, now * out_ct * sizeof(W),
                                           now * out_ct * sizeof(W), Q, hipMemcpyDeviceToDevice, stream));
        }
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
    return mul_transpose<Ops64>(ctx, matrix, matrix_plaintext_count, rows, cols, baby_step, queries, query_count, galois_keys,
                                out, false, s);
}

extern "C" int he_pnns_mul_transpose_device_u32(const he_pnns_context* ctx, const uint32_t* matrix,
                                                size_t matrix_plaintext_count, size_t rows, size_t cols, uint32_t baby_step,
                                                const uint32_t* queries, size_t query_count,
                                                const uint32_t* const* galois_keys, uint32_t* out, he_stream s) {
    return mul_transpose<Ops32>(ctx, matrix, matrix_plaintext_count, rows, cols, baby_step, queries, query_count, galois_keys,
                                out, false, s);
}

extern "C" int he_pnns_compute_response_device(const he_pnns_context* ctx, const uint64_t* matrix,
                                               size_t matrix_plaintext_count, size_t rows, size_t cols, uint32_t baby_step,
                                               const uint64_t* queries, size_t query_count,
                                               const uint64_t* const* galois_keys, uint64_t* out, he_stream s) {
    return mul_transpose<Ops64>(ctx, matrix, matrix_plaintext_count, rows, cols, baby_step, queries, query_count, galois_keys,
                                out, true, s);
}

extern "C" int he_pnns_compute_response_device_u32(const he_pnns_context* ctx, const uint32_t* matrix,
                                                   size_t matrix_plaintext_count, size_t rows, size_t cols, uint32_t baby_step,
                                                   const uint32_t* queries, size_t query_count,
                                                   const uint32_t* const* galois_keys, uint32_t* out, he_stream s) {
    return mul_transpose<Ops32>(ctx, matrix, matrix_plaintext_count, rows, cols, baby_step, queries, query_count, galois_keys,
                                out, true, s);
}
