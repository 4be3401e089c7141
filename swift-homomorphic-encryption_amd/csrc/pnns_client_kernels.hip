// pnns_client_kernels.hip -- the PNNS client (reference Sources/PrivateNearestNeighborSearch/Client.swift:74-127) on the device,
// between the kernels that exist: Context.encodeSimd / decodeSimd (Encoding.swift:222-245) around the transforms over [t], the
// dense-row packing of a query (PlaintextMatrix.swift:341-406), the unpackings of a result (:515-590), and the last step of
// Client.decrypt(response:): CrtComposer.compose (CrtComposer.swift:76-97), remainderToCentered and the float scaling
// (Client.swift:110-117).  Every kernel takes one lane per word or value it writes, on an exact grid; the permutation of
// simdEncodingMatrix always lands on the loads, so every store is a coalesced vector store.  No LDS, no atomics.
#include "kernels.hpp"
#include "launch_grid.hpp"
#include "pnns_values.hpp"

namespace heamd {

namespace {

constexpr unsigned kClientThreads = 256;

// ---- encodeSimd up to inverseNtt, decodeSimd behind forwardNtt ----------------------------------------------------------------
// array[0, simdEncodingMatrix[index]] = values[index] (Encoding.swift:228-230) as a gather: word w takes slot slot_of_word[w].
template <typename W>
__global__ __launch_bounds__(kClientThreads) void pnns_simd_scatter_kernel(const W* __restrict__ slots,
                                                                           const uint32_t* __restrict__ slot_of_word,
                                                                           uint32_t log_degree, uint64_t t, size_t words,
                                                                           W* __restrict__ staging,
                                                                           uint32_t* __restrict__ out_of_range) {
    const size_t index = static_cast<size_t>(blockIdx.x) * kClientThreads + threadIdx.x;
    if (index >= words) return;
    const size_t n = size_t(1) << log_degree;
    const size_t word = index & (n - 1);
    const W value = slots[index - word + slot_of_word[word]];
    if (static_cast<uint64_t>(value) >= t && out_of_range != nullptr) *out_of_range = 1u;  // validDataForEncoding
    staging[index] = value;
}

// poly.data[0, simdEncodingMatrix[index]] (Encoding.swift:242-244)
template <typename W>
__global__ __launch_bounds__(kClientThreads) void pnns_simd_gather_kernel(const W* __restrict__ transformed,
                                                                          const uint32_t* __restrict__ word_of_slot,
                                                                          uint32_t log_degree, size_t words,
                                                                          W* __restrict__ out_slots) {
    const size_t index = static_cast<size_t>(blockIdx.x) * kClientThreads + threadIdx.x;
    if (index >= words) return;
    const size_t n = size_t(1) << log_degree;
    const size_t slot = index & (n - 1);
    out_slots[index] = transformed[index - slot + word_of_slot[slot]];
}

// ---- denseRowPlaintexts -------------------------------------------------------------------------------------------------------
// With P = nextPowerOfTwo(cols), h = N / 2 and rpp = N / P rows to a plaintext: P divides h, so neither of the reference's two
// paddings inside the loop (:379-381) ever fires and a full plaintext p holds row p rpp + e / P, column e mod P at slot e.
// The last plaintext, when it holds m < rpp rows (m P = len values), is padded and repeated (:388-402):
//     len <= h   padded to S = nextPowerOfTwo(len) (len mod h == 0 only for len == h, where S = h too), the S slots repeat to N:
//                slot k holds element k mod S                                                          -> base 0, period S
//     len > h    the second SIMD row's len - h values are padded to S = nextPowerOfTwo(len - h) and repeat to N; the first
//                SIMD row stays: slot k < h holds element k, slot k >= h element h + (k - h) mod S     -> base h, period S
// and element e is a value when e < len and e mod P < cols, else 0.  The host hands over (base, period) of the last plaintext;
// a full last plaintext is base 0, period N.
struct DenseRowShape {
    size_t rows, cols, count;  // count: plaintexts
    uint64_t t;
    uint32_t log_degree, log_padded_cols, tail_base, tail_period;
    int reduce;
};

template <typename W>
__global__ __launch_bounds__(kClientThreads) void pnns_dense_row_pack_kernel(const long long* __restrict__ values,
                                                                             const uint32_t* __restrict__ slot_of_word,
                                                                             const DenseRowShape shape, W* __restrict__ staging,
                                                                             uint32_t* __restrict__ out_of_range) {
    const size_t index = static_cast<size_t>(blockIdx.x) * kClientThreads + threadIdx.x;
    if (index >= (shape.count << shape.log_degree)) return;
    const size_t plaintext = index >> shape.log_degree;
    const uint32_t word = static_cast<uint32_t>(index & ((size_t(1) << shape.log_degree) - 1));
    const uint32_t slot = slot_of_word[word];
    uint32_t element = slot;
    if (plaintext + 1 == shape.count && slot >= shape.tail_base)
        element = shape.tail_base + ((slot - shape.tail_base) & (shape.tail_period - 1u));
    const size_t row = (plaintext << (shape.log_degree - shape.log_padded_cols)) + (element >> shape.log_padded_cols);
    const size_t column = element & ((1u << shape.log_padded_cols) - 1u);
    unsigned long long value = 0;
    bool outside = false;
    if (row < shape.rows && column < shape.cols)
        value = pnns_signed_to_residue(values[row * shape.cols + column], static_cast<long long>(shape.t), shape.reduce != 0,
                                       outside);
    if (outside && out_of_range != nullptr) *out_of_range = 1u;  // a plain vector store; racing lanes store the same word
    staging[index] = static_cast<W>(value);
}

// ---- unpackDenseColumn, unpackDenseRow ------------------------------------------------------------------------------------------
// Where value j of the column-major sequence (column c, row r: j = c R + r) of an R-row matrix lies (PlaintextMatrix.swift:
// 524-545, the inverse of :285-331).  R <= h: a SIMD row holds V = R (h / R) values and a plaintext 2 V; the padding behind
// them is skipped.  R > h: a column spans ceil(R / N) plaintexts of its own, from slot 0.
struct DenseColumnPlace {
    size_t plaintext;
    uint32_t slot;
};
__device__ __forceinline__ DenseColumnPlace dense_column_place(size_t j, size_t rows, uint32_t log_degree) {
    const size_t n = size_t(1) << log_degree, half = n >> 1;
    if (rows <= half) {
        const size_t per_simd_row = rows * (half / rows);
        const size_t plaintext = j / (2 * per_simd_row), within = j - plaintext * 2 * per_simd_row;
        return DenseColumnPlace{plaintext,
                                static_cast<uint32_t>(within < per_simd_row ? within : half + (within - per_simd_row))};
    }
    const size_t per_column = (rows + n - 1) >> log_degree;
    const size_t column = j / rows, row = j - column * rows;
    return DenseColumnPlace{column * per_column + (row >> log_degree), static_cast<uint32_t>(row & (n - 1))};
}

struct UnpackShape {
    size_t rows, cols;
    uint32_t log_degree, log_padded_cols;
    int dense_row;
};

// one lane per value of the row-major result; `transformed` [plaintext_count][N] is forwardNtt of the plaintexts
template <typename W>
__global__ __launch_bounds__(kClientThreads) void pnns_unpack_kernel(const W* __restrict__ transformed,
                                                                     const uint32_t* __restrict__ word_of_slot,
                                                                     const UnpackShape shape,
                                                                     unsigned long long* __restrict__ out_values) {
    const size_t index = static_cast<size_t>(blockIdx.x) * kClientThreads + threadIdx.x;
    if (index >= shape.rows * shape.cols) return;
    const size_t row = index / shape.cols, column = index - row * shape.cols;
    DenseColumnPlace place;
    if (shape.dense_row) {  // (:574-583): SIMD row s, position i of it is matrix row p rpp + s (h / P) + i, at slot s h + i P
        const uint32_t log_rows = shape.log_degree - shape.log_padded_cols;
        place.plaintext = row >> log_rows;
        place.slot = static_cast<uint32_t>(((row & ((size_t(1) << log_rows) - 1)) << shape.log_padded_cols) + column);
    } else {
        place = dense_column_place(column * shape.rows + row, shape.rows, shape.log_degree);
    }
    out_values[index] = transformed[(place.plaintext << shape.log_degree) + word_of_slot[place.slot]];
}

// ---- Client.decrypt(response:) behind decrypt and forwardNtt ----------------------------------------------------------------
// One lane per distance of the column-major run [first_element, first_element + elements) that the plaintexts
// [first_plaintext, ..) of this launch hold: its residue under every context, composed in UInt64 in row order as compose does
// (acc = addMod(acc, ((inv_i x_i) mod t_i) (q / t_i), q); 2 q <= UInt64.max, so the sum never wraps), centred and scaled.
template <typename W>
__global__ __launch_bounds__(kClientThreads) void pnns_compose_distances_kernel(const W* __restrict__ transformed,
                                                                                const uint32_t* __restrict__ word_of_slot,
                                                                                const PnnsComposeLayout layout,
                                                                                const PnnsComposeTables tables,
                                                                                float scaling_factor, float* __restrict__ out) {
#pragma clang fp contract(off)
    const size_t index = static_cast<size_t>(blockIdx.x) * kClientThreads + threadIdx.x;
    if (index >= layout.elements) return;
    const size_t j = layout.first_element + index;
    const DenseColumnPlace place = dense_column_place(j, layout.rows, layout.log_degree);
    const size_t source = ((place.plaintext - layout.first_plaintext) << layout.log_degree) + word_of_slot[place.slot];
    uint64_t composed = static_cast<uint64_t>(transformed[source]);
    if (tables.count > 1) {  // (one modulus: the composition is the identity)
        uint64_t acc = 0;
        for (uint32_t i = 0; i < tables.count; ++i) {  // wave-uniform
            const uint64_t x = static_cast<uint64_t>(transformed[i * layout.context_stride + source]);
            const uint64_t scaled = shoup_mul(x, tables.inverse[i], tables.inverse_shoup[i], tables.t[i]);
            const uint64_t sum = acc + scaled * tables.punctured[i];
            acc = sum >= tables.q ? sum - tables.q : sum;
        }
        composed = acc;
    }
    // remainderToCentered(modulus: q), then Float(signed) / (Float(scalingFactor) * Float(scalingFactor)) (Client.swift:115-116)
    const long long centred = composed > ((tables.q - 1) >> 1) ? static_cast<long long>(composed - tables.q)
                                                                : static_cast<long long>(composed);
    const float divisor = scaling_factor * scaling_factor;
    const size_t column = j / layout.rows, row = j - column * layout.rows;
    out[row * layout.cols + column] = static_cast<float>(centred) / divisor;
}

template <typename Kernel, typename... Args>
hipError_t launch_exact(Kernel kernel, size_t lanes, hipStream_t stream, Args... args) {
    if (lanes == 0) return hipSuccess;
    const size_t blocks = launch_grid::grid_blocks(lanes, kClientThreads, launch_grid::kMaxLanes);
    if (!launch_grid::launch_fits(blocks, kClientThreads)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(kClientThreads), 0, stream, args...);
    return hipGetLastError();
}

uint32_t log2_exact(size_t power_of_two) {
    uint32_t log = 0;
    while ((size_t(1) << log) < power_of_two) ++log;
    return log;
}

}  // namespace

template <typename W>
hipError_t launch_pnns_simd_scatter(const W* slots, const uint32_t* slot_of_word, uint32_t log_degree, uint64_t t, size_t batch,
                                    W* staging, uint32_t* out_of_range, hipStream_t stream) {
    return launch_exact(pnns_simd_scatter_kernel<W>, batch << log_degree, stream, slots, slot_of_word, log_degree, t,
                        batch << log_degree, staging, out_of_range);
}
template hipError_t launch_pnns_simd_scatter<uint64_t>(const uint64_t*, const uint32_t*, uint32_t, uint64_t, size_t, uint64_t*,
                                                       uint32_t*, hipStream_t);
template hipError_t launch_pnns_simd_scatter<uint32_t>(const uint32_t*, const uint32_t*, uint32_t, uint64_t, size_t, uint32_t*,
                                                       uint32_t*, hipStream_t);

template <typename W>
hipError_t launch_pnns_simd_gather(const W* transformed, const uint32_t* word_of_slot, uint32_t log_degree, size_t batch,
                                   W* out_slots, hipStream_t stream) {
    return launch_exact(pnns_simd_gather_kernel<W>, batch << log_degree, stream, transformed, word_of_slot, log_degree,
                        batch << log_degree, out_slots);
}
template hipError_t launch_pnns_simd_gather<uint64_t>(const uint64_t*, const uint32_t*, uint32_t, size_t, uint64_t*, hipStream_t);
template hipError_t launch_pnns_simd_gather<uint32_t>(const uint32_t*, const uint32_t*, uint32_t, size_t, uint32_t*, hipStream_t);

template <typename W>
hipError_t launch_pnns_dense_row_pack(const int64_t* values, const uint32_t* slot_of_word, const PnnsDenseRowLayout& layout,
                                      size_t count, W* staging, uint32_t* out_of_range, hipStream_t stream) {
    const size_t n = size_t(1) << layout.log_degree, half = n >> 1;
    if (layout.padded_cols == 0 || layout.padded_cols > half || count == 0) return hipErrorInvalidValue;
    const size_t rows_per_plaintext = n / layout.padded_cols;
    if ((count - 1) * rows_per_plaintext >= layout.rows || count * rows_per_plaintext < layout.rows) return hipErrorInvalidValue;
    DenseRowShape shape{};
    shape.rows = layout.rows;
    shape.cols = layout.cols;
    shape.count = count;
    shape.t = layout.plaintext_modulus;
    shape.log_degree = layout.log_degree;
    shape.log_padded_cols = log2_exact(layout.padded_cols);
    shape.reduce = layout.reduce ? 1 : 0;
    const size_t length = (layout.rows - (count - 1) * rows_per_plaintext) * layout.padded_cols;  // the last plaintext's values
    size_t period = 1;
    if (length <= half) {
        while (period < length) period <<= 1;
        shape.tail_base = 0;
    } else {
        while (period < length - half) period <<= 1;
        shape.tail_base = static_cast<uint32_t>(half);
    }
    if (length == n) period = n;  // full: nothing repeats
    shape.tail_period = static_cast<uint32_t>(period);
    return launch_exact(pnns_dense_row_pack_kernel<W>, count << layout.log_degree, stream,
                        reinterpret_cast<const long long*>(values), slot_of_word, shape, staging, out_of_range);
}
template hipError_t launch_pnns_dense_row_pack<uint64_t>(const int64_t*, const uint32_t*, const PnnsDenseRowLayout&, size_t,
                                                         uint64_t*, uint32_t*, hipStream_t);
template hipError_t launch_pnns_dense_row_pack<uint32_t>(const int64_t*, const uint32_t*, const PnnsDenseRowLayout&, size_t,
                                                         uint32_t*, uint32_t*, hipStream_t);

template <typename W>
hipError_t launch_pnns_unpack(const W* transformed, const uint32_t* word_of_slot, const PnnsUnpackLayout& layout,
                              uint64_t* out_values, hipStream_t stream) {
    UnpackShape shape{};
    shape.rows = layout.rows;
    shape.cols = layout.cols;
    shape.log_degree = layout.log_degree;
    shape.log_padded_cols = log2_exact(layout.padded_cols);
    shape.dense_row = layout.dense_row ? 1 : 0;
    if (layout.dense_row && shape.log_padded_cols >= layout.log_degree) return hipErrorInvalidValue;
    return launch_exact(pnns_unpack_kernel<W>, layout.rows * layout.cols, stream, transformed, word_of_slot, shape,
                        reinterpret_cast<unsigned long long*>(out_values));
}
template hipError_t launch_pnns_unpack<uint64_t>(const uint64_t*, const uint32_t*, const PnnsUnpackLayout&, uint64_t*, hipStream_t);
template hipError_t launch_pnns_unpack<uint32_t>(const uint32_t*, const uint32_t*, const PnnsUnpackLayout&, uint64_t*, hipStream_t);

template <typename W>
hipError_t launch_pnns_compose_distances(const W* transformed, const uint32_t* word_of_slot, const PnnsComposeLayout& layout,
                                         const PnnsComposeTables& tables, float scaling_factor, float* out, hipStream_t stream) {
    if (tables.count == 0 || tables.count > kPnnsMaxClientContexts) return hipErrorInvalidValue;
    return launch_exact(pnns_compose_distances_kernel<W>, layout.elements, stream, transformed, word_of_slot, layout, tables,
                        scaling_factor, out);
}
template hipError_t launch_pnns_compose_distances<uint64_t>(const uint64_t*, const uint32_t*, const PnnsComposeLayout&,
                                                            const PnnsComposeTables&, float, float*, hipStream_t);
template hipError_t launch_pnns_compose_distances<uint32_t>(const uint32_t*, const uint32_t*, const PnnsComposeLayout&,
                                                            const PnnsComposeTables&, float, float*, hipStream_t);

}  // namespace heamd
