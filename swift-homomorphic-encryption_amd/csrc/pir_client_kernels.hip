// pir_client_kernels.hip -- the MulPIR client (reference Sources/PrivateInformationRetrieval/IndexPir/MulPir.swift:179-289) on
// the device, between the kernels that exist: the selection plaintexts of PirUtil.compressBinaryInputs (PirUtil.swift:361-404)
// in front of encryption, and CoefficientPacking.coefficientsToBytes (CoefficientPacking.swift:155-216) with the entry
// extraction of MulPirClient.decrypt(response:at:using:) behind decryption.  Both take one lane per word or byte they write, on
// an exact grid, and are gathers: every store is contiguous, nothing is zeroed first.  No LDS, no atomics.
#include "pir_client_kernels.hpp"

#include "launch_grid.hpp"

namespace heamd {

namespace {

constexpr unsigned kClientThreads = 256;

// ---- compressBinaryInputs up to encryption --------------------------------------------------------------------------------------
struct SelectionShape {
    uint32_t dimensions[pir_client::kMaxDimensions];
    uint64_t suffix[pir_client::kMaxDimensions];  // prod(dimensions[k + 1 ..])
    uint64_t dimension_sum, inputs /* S I */, indices_count, entries_per_plaintext, entry_count, ciphertexts, first, last, words;
    uint32_t dimension_count, log_degree;
};

// Word x of ciphertext c of query q is input p = c N + x of generateQuery's totalInputCount = S I (MulPir.swift:204-217): index
// i = p / S of the query, dimension k whose range [prefix_k, prefix_k + d_k) holds r = p mod S.  It is one when coordinate k of
// indices[q][i] is r - prefix_k (computeCoordinates, :181-193), and a one is written as (2^ceilLog2(inputs of c))^-1 mod t.
template <typename W>
__global__ __launch_bounds__(kClientThreads) void pir_selection_plaintexts_kernel(const unsigned long long* __restrict__ indices,
                                                                                  const SelectionShape shape,
                                                                                  W* __restrict__ out,
                                                                                  uint32_t* __restrict__ out_of_range) {
    const uint64_t index = static_cast<uint64_t>(blockIdx.x) * kClientThreads + threadIdx.x;
    if (index >= shape.words) return;
    const uint64_t slot = index >> shape.log_degree;  // q C + c
    const uint64_t query = slot / shape.ciphertexts, ciphertext = slot - query * shape.ciphertexts;
    const uint64_t input = (ciphertext << shape.log_degree) + (index & ((uint64_t(1) << shape.log_degree) - 1));
    uint64_t word = 0;
    if (input < shape.inputs) {
        const uint64_t i = input / shape.dimension_sum, r = input - i * shape.dimension_sum;
        uint64_t prefix = 0, local = 0, below = 1, size = 1;
        for (uint32_t k = 0; k < shape.dimension_count; ++k) {  // wave-uniform trip count; the dimensions come as scalars
            const uint64_t d = shape.dimensions[k];
            if (r >= prefix && r < prefix + d) {
                local = r - prefix;
                below = shape.suffix[k];
                size = d;
            }
            prefix += d;
        }
        const uint64_t entry = indices[query * shape.indices_count + i];
        if (entry >= shape.entry_count) {  // PirError.invalidIndex: selects nothing
            if (out_of_range != nullptr) *out_of_range = 1u;  // a plain vector store; racing lanes store the same word
        } else {
            const uint64_t plaintext = entry / shape.entries_per_plaintext;  // plaintextIndex(entryIndex:)
            if ((plaintext / below) % size == local) word = ciphertext + 1 == shape.ciphertexts ? shape.last : shape.first;
        }
    }
    out[index] = static_cast<W>(word);
}

// ---- coefficientsToBytes and the entry of a reply -----------------------------------------------------------------------------
struct ReplyShape {
    uint64_t bits, bytes_per_plaintext, width, entry_size, encoded, entries_per_plaintext, reply_ciphertexts;
    uint64_t lanes_per_entry, out_stride, entries /* queries I */;
    uint32_t log_degree;
};

// Byte `at` of a reply's byte string.  Stream bit s of a plaintext is bit bits - 1 - (s mod bits) of coefficient s / bits,
// MSB first.  The reference does not mask a coefficient to `bits` bits (CoefficientPacking.swift:200-202): bit `bits` of a
// coefficient whose field begins inside a byte is OR-ed into the bit in front of the field, the last bit of the field before;
// one whose field begins a byte loses it.  Words are below t < 2^(bits + 1): there is no higher bit.
template <typename W>
__device__ __forceinline__ uint32_t reply_byte(const W* __restrict__ reply, const ReplyShape& shape, uint64_t at) {
    const uint64_t plaintext = at / shape.bytes_per_plaintext;
    const uint64_t first_bit = (at - plaintext * shape.bytes_per_plaintext) * 8, end_bit = first_bit + 8;
    const W* __restrict__ coefficients = reply + (plaintext << shape.log_degree);
    uint64_t k = first_bit / shape.bits, field = k * shape.bits;
    uint32_t byte = 0;
    while (field < end_bit) {  // at most 8 coefficients; N bits is a multiple of 8, so k stays below N
        const uint64_t coefficient = static_cast<uint64_t>(coefficients[k]);
        const uint64_t from = field > first_bit ? field : first_bit;
        const uint64_t field_end = field + shape.bits, to = field_end < end_bit ? field_end : end_bit;
        const uint64_t part = (coefficient >> (field_end - to)) & ((uint64_t(1) << (to - from)) - 1);
        byte |= static_cast<uint32_t>(part) << (end_bit - to);
        if (field > first_bit) byte |= static_cast<uint32_t>((coefficient >> shape.bits) & 1u) << (end_bit - field);
        ++k;
        field = field_end;
    }
    return byte;
}

// One lane per byte of out_entries (and one for an entry of no bytes, which still has a size).  The entry of reply (q, i) lies
// at position pos = indices[q][i] mod per of its byte string: `width` little-endian bytes of size, then the bytes
// (MulPir.swift:233-274).  A size above E counts as E; bytes behind the size are zero.
template <typename W>
__global__ __launch_bounds__(kClientThreads) void pir_reply_entries_kernel(const W* __restrict__ plaintexts,
                                                                           const unsigned long long* __restrict__ indices,
                                                                           const ReplyShape shape,
                                                                           uint8_t* __restrict__ out_entries,
                                                                           unsigned long long* __restrict__ out_sizes) {
    const uint64_t index = static_cast<uint64_t>(blockIdx.x) * kClientThreads + threadIdx.x;
    if (index >= shape.entries * shape.lanes_per_entry) return;
    const uint64_t entry = index / shape.lanes_per_entry, byte = index - entry * shape.lanes_per_entry;
    const W* __restrict__ reply = plaintexts + ((entry * shape.reply_ciphertexts) << shape.log_degree);
    uint64_t start = 0, size = shape.out_stride;
    if (indices != nullptr) {
        start = (indices[entry] % shape.entries_per_plaintext) * shape.encoded;
        if (shape.width != 0) {
            uint64_t encoded_size = 0;
            for (uint64_t b = 0; b < shape.width; ++b)  // wave-uniform trip count
                encoded_size |= static_cast<uint64_t>(reply_byte(reply, shape, start + b)) << (8 * b);
            size = encoded_size < shape.entry_size ? encoded_size : shape.entry_size;
            start += shape.width;
        }
    }
    if (byte < shape.out_stride)
        out_entries[entry * shape.out_stride + byte] = byte < size ? static_cast<uint8_t>(reply_byte(reply, shape, start + byte)) : 0;
    if (byte == 0 && out_sizes != nullptr) out_sizes[entry] = size;
}

template <typename Kernel, typename... Args>
hipError_t launch_exact(Kernel kernel, size_t lanes, hipStream_t stream, Args... args) {
    if (lanes == 0) return hipSuccess;
    const size_t blocks = launch_grid::grid_blocks(lanes, kClientThreads, launch_grid::kMaxLanes);
    if (!launch_grid::launch_fits(blocks, kClientThreads)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(kClientThreads), 0, stream, args...);
    return hipGetLastError();
}

}  // namespace

template <typename W>
hipError_t launch_pir_selection_plaintexts(const uint64_t* indices, const pir_client::Plan& plan, size_t queries, uint64_t first,
                                           uint64_t last, W* out, uint32_t* out_of_range, hipStream_t stream) {
    if (plan.dimension_count == 0 || plan.dimension_count > pir_client::kMaxDimensions || plan.entries_per_plaintext == 0 ||
        plan.dimension_sum == 0 || plan.query_ciphertexts == 0)
        return hipErrorInvalidValue;
    SelectionShape shape{};
    for (uint32_t k = 0; k < plan.dimension_count; ++k) {
        shape.dimensions[k] = plan.dimensions[k];
        shape.suffix[k] = plan.suffix[k];
    }
    shape.dimension_sum = plan.dimension_sum;
    shape.inputs = plan.expanded_query_count;
    shape.indices_count = plan.indices_count;
    shape.entries_per_plaintext = plan.entries_per_plaintext;
    shape.entry_count = plan.entry_count;
    shape.ciphertexts = plan.query_ciphertexts;
    shape.first = first;
    shape.last = last;
    shape.dimension_count = plan.dimension_count;
    shape.log_degree = pir_client::floor_log2(plan.degree);
    shape.words = queries * plan.query_ciphertexts * plan.degree;
    return launch_exact(pir_selection_plaintexts_kernel<W>, shape.words, stream,
                        reinterpret_cast<const unsigned long long*>(indices), shape, out, out_of_range);
}
template hipError_t launch_pir_selection_plaintexts<uint64_t>(const uint64_t*, const pir_client::Plan&, size_t, uint64_t, uint64_t,
                                                              uint64_t*, uint32_t*, hipStream_t);
template hipError_t launch_pir_selection_plaintexts<uint32_t>(const uint64_t*, const pir_client::Plan&, size_t, uint64_t, uint64_t,
                                                              uint32_t*, uint32_t*, hipStream_t);

template <typename W>
hipError_t launch_pir_reply_entries(const W* plaintexts, const uint64_t* indices, const pir_client::Plan& plan, size_t queries,
                                    uint8_t* out_entries, uint64_t* out_sizes, hipStream_t stream) {
    if (plan.bits == 0 || plan.bits > 8 * sizeof(W) - 1 || plan.bytes_per_plaintext == 0 || plan.entries_per_plaintext == 0 ||
        plan.bytes_per_plaintext * 8 != plan.degree * plan.bits)
        return hipErrorInvalidValue;
    ReplyShape shape{};
    shape.bits = plan.bits;
    shape.bytes_per_plaintext = plan.bytes_per_plaintext;
    shape.width = plan.width;
    shape.entry_size = plan.entry_size;
    shape.encoded = plan.encoded;
    shape.entries_per_plaintext = plan.entries_per_plaintext;
    shape.reply_ciphertexts = plan.reply_ciphertexts;
    shape.out_stride = indices != nullptr ? plan.entry_size : plan.reply_ciphertexts * plan.bytes_per_plaintext;
    shape.lanes_per_entry = shape.out_stride != 0 ? shape.out_stride : 1;
    shape.entries = queries * plan.indices_count;
    shape.log_degree = pir_client::floor_log2(plan.degree);
    return launch_exact(pir_reply_entries_kernel<W>, shape.entries * shape.lanes_per_entry, stream, plaintexts,
                        reinterpret_cast<const unsigned long long*>(indices), shape, out_entries,
                        reinterpret_cast<unsigned long long*>(out_sizes));
}
template hipError_t launch_pir_reply_entries<uint64_t>(const uint64_t*, const uint64_t*, const pir_client::Plan&, size_t, uint8_t*,
                                                       uint64_t*, hipStream_t);
template hipError_t launch_pir_reply_entries<uint32_t>(const uint32_t*, const uint64_t*, const pir_client::Plan&, size_t, uint8_t*,
                                                       uint64_t*, hipStream_t);

}  // namespace heamd
