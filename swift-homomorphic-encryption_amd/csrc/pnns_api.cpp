// pnns_api.cpp -- the PNNS server database (reference Sources/PrivateNearestNeighborSearch/) behind the C ABI: the SIMD
// encoding context a he_bfv_context lacks, the plan (PlaintextMatrix.plaintextCount, BabyStepGiantStep.init) and
// Database.process for one context (ProcessedDatabase.swift:194-229).  Kernels: pnns_kernels.hip.
//
// Per group of plaintexts: the pack kernel writes the slabs Context.encodeSimd (Encoding.swift:222-234) fills through
// simdEncodingMatrix, the batched inverse NTT over [t] turns them into Coeff plaintexts in place, and
// Plaintext.convertToEvalFormat (he_bfv_plaintext_to_eval_device) takes them into the matrix.  The inverse NTT is in place, so
// one N-word staging slab per plaintext of a group is all the scratch there is.
#include <cstdlib>
#include <memory>
#include <vector>

#include "api_internal.hpp"
#include "bfv_context.hpp"
#include "kernels.hpp"

using heamd::as_stream;
using heamd::invalid_argument;
using heamd::Scratch;

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
