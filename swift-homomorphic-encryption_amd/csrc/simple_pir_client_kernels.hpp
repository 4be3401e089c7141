// simple_pir_client_kernels.hpp -- launchers of simple_pir_client_kernels.hip (asynchronous on `stream`), templates on the slab
// word W (uint64_t, or uint32_t with p <= 2^30 - 1).  `ctx`: SimplePirContext.extraContext, one modulus.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "device_context.hpp"
#include "simple_pir_client_plan.hpp"

namespace heamd {

// out [rows][N] 8-byte words = secrets [rows][N] (the copy the forward NTT transforms)
template <typename W>
hipError_t launch_simple_pir_client_widen(const W* secrets, uint64_t* out, size_t words, hipStream_t stream);
// staging [rows][blocks][N] = a_eval[k] * secret_eval[row] mod p, all Eval
template <typename W>
hipError_t launch_simple_pir_client_products(const W* a_eval, const uint64_t* secret_eval, uint64_t* staging, size_t rows,
                                             uint32_t blocks, const DeviceContext& ctx, hipStream_t stream);
// The last step of SimplePirContext.encryptZero for secret rows [first_row, first_row + rows) of the batch (row = query *
// chunks + chunk): queries[row][col] = (divideAndRound(staging[row - first_row][col]) + e) & mask for col < columns, with e
// coefficient chunk * columns + col of the query's error stream, drawn here from `chain` [batch][error_chunks] records.
template <typename W>
hipError_t launch_simple_pir_client_finish(const uint64_t* staging, size_t staging_row_words, const uint32_t* chain,
                                           size_t error_chunks, const simple_pir_client::ErrorSampler& sampler,
                                           const simple_pir_client::Division& division, size_t chunks, size_t columns,
                                           size_t first_row, size_t rows, W* queries, hipStream_t stream);

// codes [rows][code_words_per_row(N)]: 2 bits per secret word, 0 -> 0, 1 -> 1, p - 1 -> 2, sixteen to a word
template <typename W>
hipError_t launch_simple_pir_client_pack_codes(const W* secrets, uint32_t* codes, size_t rows, uint32_t degree, uint64_t p,
                                               hipStream_t stream);
// results [rows][column_size] = sum_n secrets[r][n] hint[j][n] mod p from the codes; hint [column_size][N], 16-byte aligned.
// rows_per_pass and fold_terms: the plan's; degree N, p and barrett64 = floor(2^64 / p): the ring's.
template <typename W>
hipError_t launch_simple_pir_client_hint_product(const uint32_t* codes, size_t rows, const W* hint, size_t column_size,
                                                 W* results, uint32_t rows_per_pass, uint64_t fold_terms, uint32_t degree,
                                                 uint64_t p, uint64_t barrett64, hipStream_t stream);

struct SimplePirClientLayout {
    uint64_t chunks, entries_per_column, database_columns, column_size, chunk_size, entry_count, entry_size_in_bytes;
    uint64_t delta, mask;
    uint32_t plaintext_bits, shift;  // shift = ciphertext_bits - plaintext_bits
};
// WithoutIndices.add(index:) for `batch` queries in place; flags[b] = 1 and query b untouched for an index >= entry_count
template <typename W>
hipError_t launch_simple_pir_client_add_indices(W* queries, const uint64_t* indices, uint32_t* flags,
                                                const SimplePirClientLayout& layout, size_t batch, hipStream_t stream);
// extractEntries of both slabs and integrate: coefficients [batch][chunks chunk_size] (zero for an index >= entry_count)
template <typename W>
hipError_t launch_simple_pir_client_integrate(const W* responses, const W* results, const uint64_t* indices, W* coefficients,
                                              uint32_t* flags, const SimplePirClientLayout& layout, size_t batch,
                                              hipStream_t stream);
// coefficientsToBytes(bitsPerCoeff: plaintext_bits) cut to entry_size_in_bytes: entries [batch][entry_size_in_bytes]
template <typename W>
hipError_t launch_simple_pir_client_entry_bytes(const W* coefficients, uint8_t* entries, const SimplePirClientLayout& layout,
                                                size_t batch, hipStream_t stream);

}  // namespace heamd
