// pir_database.hpp -- the device side of MulPirServer.process (reference Sources/PrivateInformationRetrieval/IndexPir/
// MulPir.swift:431-556): which entry bytes feed which database slot (pir_database_kernels.hip; host plan in pir_database.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace heamd {

// The database is [chunk_count][per_chunk] slots; slot s of chunk k holds plaintext j = (s % d0) * columns + s / d0 (the
// reference's reorder for sequential access, MulPir.swift:486-495 / 545-553).
//   split mode (packed_bytes == 0): plaintext j is entry j, its bytes (prefix(j) || entry_j)[k * bytes_per_plaintext,
//                                   + bytes_per_plaintext), cut at the end of the entry
//   pack mode:                      its bytes are F[j * packed_bytes, + packed_bytes), F the entries one after the other,
//                                   each as prefix || entry || zeros up to `encoded` bytes, cut at the end of F
struct PirDatabaseLayout {
    const uint8_t* entries = nullptr;       // [entry_count][entry_stride]; bytes past an entry's own size are never read
    const uint64_t* entry_sizes = nullptr;  // [entry_count] on the device, or nullptr: every entry is entry_stride bytes
    uint64_t entry_count = 0, entry_stride = 0;
    uint64_t width = 0;                     // bytes of the little-endian size prefix (0: none)
    uint64_t encoded = 0;                   // width + entry_stride
    uint64_t bytes_per_plaintext = 0;
    uint64_t packed_bytes = 0;              // entries per plaintext * encoded (pack mode); 0: split mode
    uint64_t plaintexts = 0;                // plaintexts that have bytes: ceil(entry_count / entries per plaintext) | entry_count
    uint64_t per_chunk = 0, d0 = 0, columns = 0;
    uint32_t bits = 0;                      // floor(log2 t): bits per coefficient
    uint32_t log_degree = 0;
};

// Slots [first_slot, first_slot + slots): CoefficientPacking.bytesToCoefficients (CoefficientPacking.swift:59-136, MSB
// first, zero padded to N coefficients) into staging [slots][N]; present[first_slot + i] = 0 when slot i's bytes are all
// zero (its plaintext is nil: the staging row is then all zero too), 1 otherwise.
template <typename W>
hipError_t launch_pir_database_unpack(const PirDatabaseLayout& layout, size_t first_slot, size_t slots, W* staging,
                                      uint8_t* present, hipStream_t stream);

}  // namespace heamd
