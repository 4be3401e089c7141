// pir_client_plan.hpp -- the host arithmetic of the MulPIR client (reference Sources/PrivateInformationRetrieval/IndexPir/
// MulPir.swift:86-109, 150-155, 179-236, PirUtil.swift:361-404, IndexPirProtocol.swift:61-73, 109-119).  Plain C++ (no HIP
// include): a host compiler builds it, and tests/test_pir_client_reference.py holds it to its restatement in
// tests/pir_client_reference.py without a device.
//
// With N the degree, t the plaintext modulus, bits = floor(log2 t), bpp = N bits / 8 bytes per plaintext, w the entry-size
// encoding width (0: none), E the entry size, enc = w + E, S = sum(dimensions), I indices per query:
//   per  entryChunksPerPlaintext = bpp / enc when bpp >= enc, else 1
//   R    expectedResponseCiphertextCount = ceil(enc / bpp)
//   C    query ciphertexts = ceil(S I / N)
// Entry e lies in plaintext j = e / per at position e mod per; its coordinates are the digits of j in the mixed radix of the
// dimensions, most significant first; index i of a query sets input i S + prefix_k + coordinate_k for every dimension k.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "host_math.hpp"

namespace heamd {
namespace pir_client {

constexpr uint32_t kMaxDimensions = 16;  // the kernels take the dimensions by value

inline uint32_t floor_log2(uint64_t value) {
    uint32_t log = 0;
    while ((value >> (log + 1)) != 0) ++log;
    return log;
}
inline uint32_t ceil_log2(uint64_t value) {  // Int.ceilLog2; 0 for 0 and 1
    if (value <= 1) return 0;
    return floor_log2(value - 1) + 1;
}

// IndexPirConfig.entrySizeEncodingWidth (IndexPirProtocol.swift:109-119)
inline uint64_t encoding_width(uint64_t entry_size) {
    if (entry_size <= 0xffu) return 1;
    if (entry_size <= 0xffffu) return 2;
    if (entry_size <= 0xffffffffu) return 4;
    return 8;
}

struct Plan {
    uint64_t degree = 0, bits = 0, bytes_per_plaintext = 0, width = 0, entry_size = 0, encoded = 0;
    uint64_t entries_per_plaintext = 0;  // per
    uint64_t reply_ciphertexts = 0;      // R
    uint64_t dimension_sum = 0, indices_count = 0, entry_count = 0;
    uint64_t expanded_query_count = 0;    // S I
    uint64_t query_ciphertexts = 0;       // C
    uint32_t dimension_count = 0;
    uint32_t dimensions[kMaxDimensions] = {};
    uint64_t suffix[kMaxDimensions] = {};  // prod(dimensions[k + 1 ..]): coordinate_k = (j / suffix[k]) mod dimensions[k]
};

// The plan of arguments already validated (he_pir_database_shape's checks, 1 <= dimension_count <= 16, indices_count >= 1).
inline Plan plan(uint64_t degree, uint64_t t, const uint32_t* dimensions, uint32_t dimension_count, uint64_t entry_count,
                 uint64_t entry_size, bool encoding_entry_size, uint64_t indices_count) {
    Plan p;
    p.degree = degree;
    p.bits = floor_log2(t);
    p.bytes_per_plaintext = degree * p.bits / 8;
    p.width = encoding_entry_size ? encoding_width(entry_size) : 0;
    p.entry_size = entry_size;
    p.encoded = p.width + entry_size;
    p.entries_per_plaintext = p.bytes_per_plaintext >= p.encoded ? p.bytes_per_plaintext / p.encoded : 1;
    p.reply_ciphertexts = (p.encoded + p.bytes_per_plaintext - 1) / p.bytes_per_plaintext;
    p.dimension_count = dimension_count;
    for (uint32_t k = 0; k < dimension_count; ++k) {
        p.dimensions[k] = dimensions[k];
        p.dimension_sum += dimensions[k];
    }
    uint64_t suffix = 1;
    for (uint32_t k = dimension_count; k-- > 0;) {
        p.suffix[k] = suffix;
        suffix *= dimensions[k];
    }
    p.indices_count = indices_count;
    p.entry_count = entry_count;
    p.expanded_query_count = p.dimension_sum * indices_count;
    p.query_ciphertexts = (p.expanded_query_count + degree - 1) / degree;
    return p;
}

// MulPirClient.computeCoordinates(at:) for an index below entry_count; out: dimension_count coordinates
inline void coordinates(const Plan& p, uint64_t entry_index, uint64_t* out) {
    const uint64_t plaintext = entry_index / p.entries_per_plaintext;
    for (uint32_t k = 0; k < p.dimension_count; ++k) out[k] = (plaintext / p.suffix[k]) % p.dimensions[k];
}
// the position of an entry in its plaintext (computeResponseRangeInBytes: bytes [position enc, (position + 1) enc))
inline uint64_t position(const Plan& p, uint64_t entry_index) { return entry_index % p.entries_per_plaintext; }

// the inputs query ciphertext c compresses: min(N, S I - c N)
inline uint64_t input_count(const Plan& p, uint64_t ciphertext) {
    const uint64_t left = p.expanded_query_count - ciphertext * p.degree;
    return left < p.degree ? left : p.degree;
}
// compressInputsForOneCiphertext's value (PirUtil.swift:367-371): (2^ceilLog2(count))^-1 mod t; false: no such inverse
inline bool selection_value(uint64_t count, uint64_t t, uint64_t& out) {
    return inverse_mod(pow_mod(2 % t, ceil_log2(count), t), t, out);
}

// MulPir.evaluationKeyConfig(expandedQueryCount:degree:keyCompression:) (MulPir.swift:86-109): the Galois elements, in the
// reference's order.  Strategies as PirKeyCompressionStrategy: 0 noCompression, 1 hybridCompression, 2 maxCompression.
enum KeyCompression { kNoCompression = 0, kHybridCompression = 1, kMaxCompression = 2 };
inline std::vector<uint64_t> evaluation_key_elements(uint64_t degree, uint64_t expanded_query_count, int key_compression) {
    const int64_t log_degree = floor_log2(degree);
    const int64_t depth = ceil_log2(expanded_query_count < degree ? expanded_query_count : degree);
    const int64_t smallest = log_degree - depth + 1;
    int64_t largest = log_degree;
    if (key_compression != kNoCompression) {
        const int64_t half = (log_degree + 1 + 1) / 2;  // (degree.log2 + 1).dividingCeil(2)
        largest = smallest > half ? smallest : half;
    }
    std::vector<uint64_t> elements;
    for (int64_t level = smallest; level <= largest; ++level) elements.push_back((uint64_t(1) << level) + 1);
    if (key_compression == kHybridCompression) {
        const int64_t middle = (log_degree + largest + 1) / 2;
        const uint64_t extra = (uint64_t(1) << (largest > middle ? largest : middle)) + 1;
        bool found = false;
        for (uint64_t e : elements) found = found || e == extra;
        if (!found) elements.push_back(extra);
    }
    return elements;
}

}  // namespace pir_client
}  // namespace heamd
