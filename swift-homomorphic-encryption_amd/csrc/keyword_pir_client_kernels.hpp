// keyword_pir_client_kernels.hpp -- launchers of keyword_pir_client_kernels.hip (asynchronous on `stream`): what
// KeywordPirClient (reference Sources/PrivateInformationRetrieval/KeywordPir/KeywordPirProtocol.swift:279-392) does besides the
// index-PIR client and the hashing of keyword_pir.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "keyword_pir_client_plan.hpp"

namespace heamd {

// uint32 -> uint64, one lane per index: he_keyword_pir_hash_indices_device's indices as the MulPIR client reads them
hipError_t launch_keyword_client_widen_indices(const uint32_t* in, uint64_t* out, size_t count, hipStream_t stream);

// decrypt(response:at:using:) lines 352-358 over bucket bytes: buckets [queries][h][E] at any byte address, hashes [queries].
//   records     scratch, [queries][h] records of keyword_pir_client::kRecordBytes bytes, 16-byte aligned
//   out_values  [queries][value_capacity(E)] at any byte address: the value, then zeros
//   out_sizes   [queries]; out_status [queries]: keyword_pir_client::kStatusNil / Found / Corrupt
// form: kFindStaged needs E <= kStagedRowLimit (else hipErrorInvalidValue).  Two launches: the walk, then the resolve and copy.
hipError_t launch_keyword_client_find(const uint8_t* buckets, const uint64_t* hashes, uint64_t entry_size, uint32_t h, size_t queries,
                                      keyword_pir_client::FindForm form, void* records, uint8_t* out_values, uint64_t* out_sizes,
                                      uint32_t* out_status, hipStream_t stream);

// countEntriesInResponse (:376-391) over reply bytes: bytes [queries][replies_per_query][reply_bytes] at any byte address;
// out_counts [queries], the slots of every bucket the scan deserializes, summed over a query's replies.
hipError_t launch_keyword_client_count(const uint8_t* bytes, uint64_t reply_bytes, uint64_t replies_per_query, size_t queries,
                                       uint64_t* out_counts, hipStream_t stream);

}  // namespace heamd
