// pnns_context.hpp -- what the PNNS translation units share: the handle behind he_pnns_context and the plan of a
// PlaintextMatrix (pnns_api.cpp: the server's database and response; pnns_client_api.cpp: the client's query and distances).
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "api_internal.hpp"
#include "bfv_context.hpp"

// Opaque handle of include/he_amd.h
struct he_pnns_context {
    const he_bfv_context* bfv = nullptr;          // borrowed
    std::unique_ptr<heamd::PolyContext> plaintext;  // plaintextContext: [t]
    std::vector<uint32_t> encoding_matrix;        // simdEncodingMatrix: slot -> slab word
    uint32_t* slot_of_word_device = nullptr;      // its inverse, on the device: [N], then simdEncodingMatrix itself, [N]
    const uint32_t* word_of_slot_device() const { return slot_of_word_device + encoding_matrix.size(); }
    ~he_pnns_context() {
        if (slot_of_word_device != nullptr) (void)hipFree(slot_of_word_device);
    }
};

namespace heamd {

inline size_t next_power_of_two(size_t x) {
    size_t p = 1;
    while (p < x) p <<= 1;
    return p;
}
inline size_t dividing_ceil(size_t a, size_t b) { return (a + b - 1) / b; }

struct MatrixPlan {
    size_t plaintext_count = 0, padded_cols = 0, plaintexts_per_column = 0;
    uint32_t baby_step = 0, giant_step = 0;
};

// PlaintextMatrix.plaintextCount (PlaintextMatrix.swift:246-275) and BabyStepGiantStep.init (MatrixMultiplication.swift:33-60):
// pnns_api.cpp
int matrix_plan(const he_pnns_context* ctx, size_t rows, size_t cols, int packing, uint32_t baby_step, MatrixPlan& plan);

}  // namespace heamd
