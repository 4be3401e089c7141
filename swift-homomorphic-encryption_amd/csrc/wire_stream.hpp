// wire_stream.hpp -- the device helpers the wire-format kernels share (ciphertext_wire_kernels.hip,
// pir_database_file_kernels.hip): a row of PolyRq.serialize is ONE big-endian bit stream of N fields (CoefficientPacking.swift:
// 169-213), read and written through the aligned 8-byte words of the byte buffer that hold it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace heamd {
namespace wire_stream {

__device__ __forceinline__ uint64_t wire_byte_swap64(uint64_t v) {
    return (static_cast<uint64_t>(__builtin_bswap32(static_cast<uint32_t>(v))) << 32) |
           __builtin_bswap32(static_cast<uint32_t>(v >> 32));
}

// `bits` (8 .. 64) stream bits of a row of w-bit fields starting at stream bit `bit`, right-aligned; past the last field: zeros
template <typename W>
__device__ __forceinline__ uint64_t gather_row_bits(const W* __restrict__ row, uint32_t n, uint32_t w, uint32_t skip,
                                                    uint64_t bit, uint32_t bits) {
    uint32_t k = static_cast<uint32_t>(bit / w), offset = static_cast<uint32_t>(bit - uint64_t(k) * w);
    const uint64_t field_mask = w == 64 ? ~uint64_t(0) : ((uint64_t(1) << w) - 1);
    uint64_t out = 0;
    uint32_t needed = bits;
    while (needed > 0 && k < n) {
        const uint32_t available = w - offset;
        const uint32_t take = available < needed ? available : needed;
        const uint64_t value = (static_cast<uint64_t>(row[k]) >> skip) & field_mask;
        const uint64_t piece = (value >> (available - take)) & (take == 64 ? ~uint64_t(0) : ((uint64_t(1) << take) - 1));
        out = (take == 64 ? 0 : (out << take)) | piece;
        needed -= take;
        offset += take;
        if (offset == w) {
            offset = 0;
            ++k;
        }
    }
    return needed >= 64 ? 0 : (out << needed);  // zero padding after the last coefficient
}

// the aligned 8-byte word at `word` as a big-endian integer; bytes outside [lowest, end) read as zero and are not touched
__device__ __forceinline__ uint64_t load_stream_word(const uint8_t* word, const uint8_t* lowest, const uint8_t* end) {
    if (word >= lowest && word + 8 <= end) return wire_byte_swap64(*reinterpret_cast<const uint64_t*>(word));
    uint64_t v = 0;
    for (int b = 0; b < 8; ++b) v = (v << 8) | (word + b >= lowest && word + b < end ? word[b] : 0);
    return v;
}

// field k of a row of w-bit fields whose first byte is `row_bytes`, out of the one or two aligned words around it
__device__ __forceinline__ uint64_t load_stream_field(const uint8_t* row_bytes, uint32_t k, uint32_t w, const uint8_t* lowest,
                                                      const uint8_t* end) {
    const uint64_t bit = uint64_t(k) * w;
    const uint8_t* first = row_bytes + (bit >> 3);
    const uint8_t* word = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(first) & ~uintptr_t(7));
    const uint32_t shift = static_cast<uint32_t>(first - word) * 8 + static_cast<uint32_t>(bit & 7);  // 0 .. 63
    const uint64_t high = load_stream_word(word, lowest, end);
    // the field ends in the next word only when shift + w > 64; otherwise that word is not read
    const uint64_t low = shift + w > 64 ? load_stream_word(word + 8, lowest, end) : 0;
    const uint64_t aligned = shift == 0 ? high : ((high << shift) | (low >> (64 - shift)));
    return aligned >> (64 - w);
}

}  // namespace wire_stream
}  // namespace heamd
