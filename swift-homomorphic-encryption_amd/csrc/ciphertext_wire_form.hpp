// ciphertext_wire_form.hpp -- which kernel form a ciphertext-level wire-format call runs, and its index space.
// Plain C++ (no HIP include): a host compiler builds it, and tests/test_ciphertext_wire.py holds it to its restatement in
// tests/ciphertext_wire_reference.py without a device, so a device test can say which form its case ran.
//
// A record is a 2-byte header followed by polynomials whose bytes end wherever their widths put them, at any stride: neither
// the rows nor the records keep an alignment, so the aligned forms of serialize_form.hpp do not apply.  Each direction has
// one form that holds for every address and stride, on 8- and 4-byte slabs alike:
//   chunk  (serialize)    a lane owns one ALIGNED 8-byte chunk of the records buffer and gathers the stream bits that fall
//                         into it; a chunk that lies wholly inside its record is one 8-byte store, a chunk that holds a
//                         record's first or last bytes is byte stores (never a read-modify-write: with an odd stride the
//                         neighbouring record's lanes own the other bytes of that chunk);
//   field  (deserialize)  a lane owns one coefficient and reads the one or two ALIGNED 8-byte words that hold its field; a
//                         word that reaches outside [records, records + (count - 1) stride + record bytes) is read byte by
//                         byte, its outside bytes as zero.
// `edge_free` says that the record pointer and the stride are multiples of 8: then only a record's last chunk can take byte
// stores, and no word of the byte buffer but the last reaches outside it.
#pragma once

#include <cstddef>
#include <cstdint>

namespace heamd {
namespace ciphertext_wire_form {

// values continue serialize_form::Form (0 byte, 1 word, 2 tile), which he_ciphertexts_wire_plan reports for the
// polynomial-level entries
enum class Form { kChunk = 3, kField = 4 };

constexpr uint64_t kChunkBytes = 8;

struct Plan {
    Form form;
    uint64_t items_per_record;  // chunk: aligned chunks a record can touch; field: coefficients of a ciphertext
    bool edge_free;
};

// the most aligned 8-byte chunks a record of record_bytes can overlap, whatever its address: ceil((record_bytes + 7) / 8)
constexpr uint64_t chunks_per_record(uint64_t record_bytes) { return (record_bytes + 2 * kChunkBytes - 2) / kChunkBytes; }

inline Plan for_serialize(uint64_t record_bytes, size_t record_stride, uintptr_t records) {
    return Plan{Form::kChunk, chunks_per_record(record_bytes), ((records | record_stride) & (kChunkBytes - 1)) == 0};
}

inline Plan for_deserialize(uint32_t polys, uint32_t rows, uint32_t log_degree, size_t record_stride, uintptr_t records) {
    return Plan{Form::kField, (static_cast<uint64_t>(polys) * rows) << log_degree,
                ((records | record_stride) & (kChunkBytes - 1)) == 0};
}

}  // namespace ciphertext_wire_form
}  // namespace heamd
