// simple_pir_batch_plan.hpp -- which path he_simple_pir_compute_response_batch_device takes for a shape, and with what tile.
// Plain C++ (no HIP include): the API, the launcher and a host-only test program share it.
//
// The modulus is a power of two, so the product splits exactly into 7-bit limbs (each 0..127, a non-negative int8):
//   sum_c d[r][c] x[q][c] mod 2^cb = ( sum_s 2^(7s) sum_{i+j=s} sum_c d_i[r][c] x_j[q][c] ) mod 2^cb,
// of which only the shift classes s < ceil(cb / 7) survive the mask.  All limb pairs of one class share an i32 accumulator.
#pragma once

#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace heamd {
namespace simple_pir_batch {

constexpr unsigned kLimbBits = 7;
constexpr unsigned kKStep = 64;          // columns of one v_mfma_i32_16x16x64_i8
constexpr unsigned kBlockRows = 128;     // database rows of one workgroup: 4 wavefronts x 2 tiles of 16 rows
constexpr unsigned kRequestTile = 16;    // requests of one accumulator tile
// up to this many shift classes a pass carries two request tiles, above it one: what keeps the kernel's accumulators, its
// prefetched database chunks and its staged request words in registers at two wavefronts per SIMD (4-byte words stage twice
// the columns per tile)
constexpr unsigned wide_classes(uint32_t word_bits) { return word_bits == 32 ? 4 : 6; }
constexpr uint64_t kLimbProduct = 127u * 127u;  // 16129, the largest product of two limbs

struct Plan {
    uint32_t matrix_path = 0, database_limbs = 0, request_limbs = 0, requests_per_pass = 0;
    size_t fold_columns = 0, workspace_bytes = 0;
};

constexpr uint32_t classes_of(uint32_t ciphertext_bits) { return (ciphertext_bits + kLimbBits - 1) / kLimbBits; }

// 1: the stored byte is the limb; 2: lo = e & 127, hi = e >> 7; 0: not on the matrix path
constexpr uint32_t database_limbs_of(uint32_t plaintext_bits) {
    return plaintext_bits <= 7 ? 1u : (plaintext_bits >= 9 && plaintext_bits <= 14) ? 2u : 0u;
}

constexpr uint32_t requests_per_pass_of(uint32_t classes, uint32_t word_bits) {
    return classes <= wide_classes(word_bits) ? 2 * kRequestTile : kRequestTile;
}

// The largest multiple of the K step after which `limbs` limb pairs per column still fit a non-negative i32:
// fold_columns * limbs * 16129 <= INT32_MAX.  133120 columns for one limb, 66560 for two.
constexpr size_t natural_fold_columns(uint32_t limbs) {
    return static_cast<size_t>(static_cast<uint64_t>(INT32_MAX) / (kLimbProduct * limbs) / kKStep * kKStep);
}

// HEAMD_SIMPLE_PIR_FOLD_COLUMNS=<columns> lowers the cadence (the tests: many folds must give the words of one), rounded
// down to a multiple of the K step and never below one step; it never raises it.  Read at the call.
inline size_t fold_columns_in_force(uint32_t limbs) {
    size_t columns = natural_fold_columns(limbs);
    if (const char* forced = std::getenv("HEAMD_SIMPLE_PIR_FOLD_COLUMNS")) {
        const unsigned long long want = std::strtoull(forced, nullptr, 10);
        if (want != 0 && want < columns) columns = want < kKStep ? kKStep : static_cast<size_t>(want) / kKStep * kKStep;
    }
    return columns;
}

inline Plan plan_for(uint32_t plaintext_bits, uint32_t ciphertext_bits, uint32_t word_bits) {
    Plan plan;
    plan.database_limbs = database_limbs_of(plaintext_bits);
    plan.matrix_path = plan.database_limbs != 0;
    plan.request_limbs = classes_of(ciphertext_bits);
    if (plan.matrix_path) {
        plan.requests_per_pass = requests_per_pass_of(plan.request_limbs, word_bits);
        plan.fold_columns = fold_columns_in_force(plan.database_limbs);
    } else {
        plan.requests_per_pass = 8;  // the existing reply kernel's pass
        plan.fold_columns = 0;
    }
    plan.workspace_bytes = 0;  // request words are split while they are staged in LDS
    return plan;
}

}  // namespace simple_pir_batch
}  // namespace heamd
