// simple_pir_context.hpp -- the opaque he_simple_pir_context of include/he_amd.h: the plan of a SimplePIR database
// (computingParams, SimplePir+Database.swift:209-243) and SimplePirContext.extraContext on the device.  Shared by the server
// (simple_pir_api.cpp) and the client (simple_pir_client_api.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>

#include "poly_context.hpp"

namespace heamd {

struct SimplePirPlan {
    uint32_t plaintext_bits = 0, ciphertext_bits = 0, lattice_dimension = 0, word_bits = 0, element_bytes = 0;
    size_t entry_count = 0, entry_size_in_bytes = 0;
    size_t entry_size_in_scalar = 0, entries_per_column = 0, chunks_per_entry = 0, database_columns = 0, column_size = 0,
           padded_entry_size = 0, a_poly_count = 0;
    uint64_t modulus = 0;
};

// he_simple_pir_shape's checks and plan (simple_pir_api.cpp)
int simple_pir_plan(uint32_t plaintext_bits, uint32_t ciphertext_bits, uint32_t lattice_dimension, uint32_t word_bits,
                    size_t entry_count, size_t entry_size_in_bytes, SimplePirPlan& plan);

}  // namespace heamd

// Opaque handle of include/he_amd.h: the plan and SimplePirContext.extraContext on the device
struct he_simple_pir_context {
    heamd::SimplePirPlan plan;
    std::unique_ptr<heamd::PolyContext> ring;
};
