// pir_client_kernels.hpp -- launchers of pir_client_kernels.hip: the two kernels of the MulPIR client that are not encryption
// or decryption (reference Sources/PrivateInformationRetrieval/IndexPir/MulPir.swift:179-289, PirUtil.swift:361-404,
// Sources/HomomorphicEncryption/CoefficientPacking.swift:141-216).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pir_client_plan.hpp"

namespace heamd {

// The plaintexts of PirUtil.compressBinaryInputs for `queries` queries: out [queries][C][N] words, every word written.
//   indices       DEVICE [queries][I] entry indices; one not below entry_count sets *out_of_range (may be nullptr) to 1 and
//                 selects nothing
//   first, last   compressInputsForOneCiphertext's value of ciphertexts 0 .. C - 2 and of ciphertext C - 1
template <typename W>
hipError_t launch_pir_selection_plaintexts(const uint64_t* indices, const pir_client::Plan& plan, size_t queries, uint64_t first,
                                           uint64_t last, W* out, uint32_t* out_of_range, hipStream_t stream);

// The bytes of MulPirClient.decrypt(response:at:using:) / decryptFull behind decryption: plaintexts [queries][I][R][N] words
// below t.  The byte string of a reply is CoefficientPacking.coefficientsToBytes of its R plaintexts back to back.
//   indices      DEVICE [queries][I], or nullptr: decryptFull, out_entries [queries][I][R bpp] the whole byte string
//   out_entries  [queries][I][E]: the entry's bytes, zeros behind its size
//   out_sizes    [queries][I] (may be nullptr): min(size prefix, E); E without a prefix; R bpp for decryptFull
template <typename W>
hipError_t launch_pir_reply_entries(const W* plaintexts, const uint64_t* indices, const pir_client::Plan& plan, size_t queries,
                                    uint8_t* out_entries, uint64_t* out_sizes, hipStream_t stream);

}  // namespace heamd
