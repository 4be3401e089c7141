// pir_client_layer.hpp -- the MulPIR client's checks and plans for the entries built on it (keyword_pir_client_api.cpp).
// Defined once, in pir_client_api.cpp; not exported.
#pragma once

#include "api_internal.hpp"
#include "pir_client_plan.hpp"

namespace heamd {
namespace pir_client {

// The IndexPirParameter and the index count of a query: he_pir_client_plan's errors
int client_plan(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count, size_t entry_count,
                size_t entry_size_in_bytes, int encoding_entry_size, size_t indices_count, Plan& plan);

// A workspace begins with the plaintexts; from `nested` to `total` lies that of he_bfv_encrypt_device / he_bfv_decrypt_device
struct QueryPlan {
    Plan client;
    uint64_t first = 0, last = 0;  // compressInputsForOneCiphertext's value of every ciphertext but the last, and of the last
    size_t nested = 0, total = 0;
};
struct ResponsePlan {
    Plan client;
    size_t replies = 0;  // ciphertexts: queries I R
    size_t out_stride = 0, nested = 0, total = 0;
};
// Every check of he_pir_generate_query_device / he_pir_decrypt_response_device in front of the null buffers, in their order: the
// word and the context, client_plan's errors, (response) moduli_count, "too many queries for one call", (query)
// HE_ERR_NOT_INVERTIBLE
int plan_query(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions, uint32_t dimension_count,
               size_t entry_count, size_t entry_size_in_bytes, int encoding_entry_size, size_t indices_count, size_t queries,
               QueryPlan& plan);
int plan_response(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions, uint32_t dimension_count,
                  size_t entry_count, size_t entry_size_in_bytes, int encoding_entry_size, size_t indices_count,
                  uint32_t moduli_count, bool full, size_t queries, ResponsePlan& plan);

}  // namespace pir_client
}  // namespace heamd
