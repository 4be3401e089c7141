// keyword_pir_client_plan.hpp -- the host arithmetic of the keyword-PIR client (reference Sources/PrivateInformationRetrieval/
// KeywordPir/KeywordPirProtocol.swift:279-392 over HashBucket.swift:51-73,118-133,200-205).  Plain C++ (no HIP include): a host
// compiler builds it, and tests/test_keyword_pir_client_reference.py holds it to its restatement in
// tests/keyword_pir_client_reference.py without a device.
//
// The index-PIR parameter of a keyword database has no size prefix and a batch of h = hashFunctionCount indices
// (KeywordPirProtocol.swift:221-228): everything about queries and replies is pir_client_plan.hpp at encoding_entry_size = false,
// indices_count = h.  What this header adds is about the bucket row of E = entry_size_in_bytes bytes a reply decodes to: the
// slot count byte, then per slot 8 bytes of keyword hash, a UInt16 value size and the value.  It is the one place where the
// longest value of a row and the form of the bucket search are written.
#pragma once

#include <cstddef>
#include <cstdint>

namespace heamd {
namespace keyword_pir_client {

constexpr uint32_t kMaxHashFunctions = 8;     // he_keyword_pir_hash_indices_device's limit
constexpr uint64_t kSlotHeaderBytes = 10;     // keyword hash and value size
constexpr uint64_t kMaxValueBytes = 0xffffu;  // HashBucketEntry's UInt16 size

// The longest value a row of E bytes can hold: one slot behind the count byte.
inline uint64_t value_capacity(uint64_t entry_size) {
    if (entry_size < 1 + kSlotHeaderBytes) return 0;
    const uint64_t room = entry_size - 1 - kSlotHeaderBytes;
    return room < kMaxValueBytes ? room : kMaxValueBytes;
}

// The bucket search walks a chain of up to 255 slots whose addresses are only known by walking.  The staged form copies the row
// into LDS first and walks it there; the direct form walks global memory.
enum FindForm { kFindStaged = 0, kFindDirect = 1 };

// The LDS budget between the two: rows of up to 32 KiB are staged.  Reason: a CU's 160 KiB then still hold four such workgroups,
// so the walk of one row overlaps the loads of the next.  A design number, not a measured optimum.
constexpr uint64_t kStagedRowLimit = 32 * 1024;
// Rows of up to 4 KiB take the staged kernel's small instantiation (one wave a workgroup; the 32 waves a CU holds fit its LDS).
constexpr uint64_t kStagedSmallRowLimit = 4 * 1024;
// A row is staged at its own offset inside a 16-byte line, so that 16-byte loads meet 16-byte LDS stores: up to 15 bytes in front.
constexpr uint64_t kStagePadding = 16;
constexpr uint64_t kStagedLdsBytes = kStagedRowLimit + kStagePadding;
constexpr uint64_t kStagedSmallLdsBytes = kStagedSmallRowLimit + kStagePadding;

inline FindForm find_form(uint64_t entry_size) { return entry_size <= kStagedRowLimit ? kFindStaged : kFindDirect; }

// One record of 16 bytes per (query, bucket) goes from the walk to the launch that resolves a query.
constexpr uint64_t kRecordBytes = 16;
constexpr uint32_t kStatusNil = 0, kStatusFound = 1, kStatusCorrupt = 2;

struct Plan {
    uint64_t value_capacity = 0;
    FindForm form = kFindStaged;
    uint64_t lds_bytes = 0;    // of the staged kernel's instantiation; 0 for the direct form
    uint64_t reply_bytes = 0;  // R bpp: what countEntriesInResponse walks per reply
};

// reply_ciphertexts (R) and bytes_per_plaintext (bpp) are pir_client_plan.hpp's for this E without a size prefix
inline Plan plan(uint64_t entry_size, uint64_t reply_ciphertexts, uint64_t bytes_per_plaintext) {
    Plan p;
    p.value_capacity = value_capacity(entry_size);
    p.form = find_form(entry_size);
    p.lds_bytes = p.form == kFindDirect ? 0 : (entry_size <= kStagedSmallRowLimit ? kStagedSmallLdsBytes : kStagedLdsBytes);
    p.reply_bytes = reply_ciphertexts * bytes_per_plaintext;
    return p;
}

}  // namespace keyword_pir_client
}  // namespace heamd
