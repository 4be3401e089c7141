// serialize_form.hpp -- which of the three wire-format kernel forms a serialize or deserialize call runs.
// Plain C++ (no HIP include): a host compiler builds it, and tests/test_wire_format_reference.py holds the choice to its
// restatement in tests/wire_format_reference.py without a device, so a device test can say which form its case ran.
//
//   tile  one wavefront per 128 coefficients, 16-byte accesses: whole tiles, and every row, the record, the record stride and
//         both buffers on 16-byte boundaries;
//   word  8 bytes per lane: every row, the record, the record stride and the byte buffer on 8-byte boundaries;
//   byte  everything else.
// Serialized records are tight (their stride is the record's byte count); a deserialized record may be longer than the
// polynomial needs (include/he_amd.h: the leading byte count of each record is read), so its stride counts as well.
// A tile-aligned call is word-aligned too: a launcher whose tile grid does not fit a launch takes the word form.
#pragma once

#include <cstddef>
#include <cstdint>

namespace heamd {
namespace serialize_form {

enum class Form { kByte = 0, kWord = 1, kTile = 2 };

// every row and the record itself start on an 8-byte boundary of an 8-byte aligned buffer
// (byte_offset: rows + 1 prefix sums, [rows] = bytes per polynomial)
inline bool word_aligned(uint32_t rows, const uint64_t* byte_offset, uintptr_t bytes) {
    if ((bytes & 7) != 0) return false;
    for (uint32_t r = 0; r <= rows; ++r)
        if ((byte_offset[r] & 7) != 0) return false;
    return true;
}

// whole 128-coefficient tiles, every row, the record and both buffers on 16-byte boundaries
inline bool tile_aligned(uint32_t rows, const uint32_t* width, const uint64_t* byte_offset, uintptr_t bytes, uintptr_t slab,
                         uint32_t log_degree) {
    if (log_degree < 7) return false;
    if (((bytes | slab) & 15) != 0) return false;
    for (uint32_t r = 0; r <= rows; ++r)
        if ((byte_offset[r] & 15) != 0) return false;
    for (uint32_t r = 0; r < rows; ++r)
        if (width[r] == 0 || width[r] > 64) return false;
    return true;
}

inline Form for_serialize(uint32_t rows, const uint32_t* width, const uint64_t* byte_offset, uintptr_t bytes, uintptr_t slab,
                          uint32_t log_degree) {
    if (tile_aligned(rows, width, byte_offset, bytes, slab, log_degree)) return Form::kTile;
    if (word_aligned(rows, byte_offset, bytes)) return Form::kWord;
    return Form::kByte;
}

inline Form for_deserialize(uint32_t rows, const uint32_t* width, const uint64_t* byte_offset, uintptr_t bytes, uintptr_t slab,
                            uint32_t log_degree, size_t bytes_per_poly) {
    if (tile_aligned(rows, width, byte_offset, bytes, slab, log_degree) && (bytes_per_poly & 15) == 0) return Form::kTile;
    if (word_aligned(rows, byte_offset, bytes) && (bytes_per_poly & 7) == 0) return Form::kWord;
    return Form::kByte;
}

// Slabs of 4-byte words (PolyRq<UInt32>, widths <= 30) take the word and byte forms: a 128-coefficient tile of such a slab is
// 32 lanes of 16 bytes, not the tile kernels' 64.  Neither form asks anything of the slab's address.
inline Form for_serialize_narrow(uint32_t rows, const uint64_t* byte_offset, uintptr_t bytes) {
    return word_aligned(rows, byte_offset, bytes) ? Form::kWord : Form::kByte;
}

inline Form for_deserialize_narrow(uint32_t rows, const uint64_t* byte_offset, uintptr_t bytes, size_t bytes_per_poly) {
    return word_aligned(rows, byte_offset, bytes) && (bytes_per_poly & 7) == 0 ? Form::kWord : Form::kByte;
}

}  // namespace serialize_form
}  // namespace heamd
