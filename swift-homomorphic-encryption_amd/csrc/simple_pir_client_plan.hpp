// simple_pir_client_plan.hpp -- the host arithmetic of the SimplePIR client (reference Sources/PrivateInformationRetrieval/
// SimplePir/SimplePir+Client.swift:19-121, SimplePir+Precompute.swift:191-311, HomomorphicEncryption/Array2d.swift:382-429,
// 489-514) and the one routine its finishing kernel shares with the host: the rounded division of divideAndRound.  Plain C++
// (no HIP include): a host compiler builds it, and tests/c/simple_pir_client_plan_probe.cpp holds it to
// tests/simple_pir_client_reference.py without a device.
//
// With N the lattice dimension, p the NTT-friendly modulus (2^c <= p < 2^(c+1), c = ciphertext_bits), C = chunks_per_entry,
// D = database_columns, A = a_poly_count = ceil(D / N), B queries per call and R = B C secret rows:
//   query slab of one precomputed query     C D words              results slab   C column_size words
//   error stream of one query               C D coefficients of 16 (stdDev32) or 32 (stdDev64) bytes, ONE generator
//   secret x hint                           passes of G = secret_rows_per_pass rows per read of the hint
#pragma once

#include <cstddef>
#include <cstdint>

#include "workspace_layout.hpp"  // round16

#if defined(__HIPCC__)
#define HEAMD_SIMPLE_PIR_CLIENT_HD __host__ __device__
#else
#define HEAMD_SIMPLE_PIR_CLIENT_HD
#endif

namespace heamd {
namespace simple_pir_client {

// ErrorStdDev (HomomorphicEncryption/Error.swift, EncryptionParameters.swift): the cases of the C ABI
enum ErrorStdDev { kStdDev32 = 0, kStdDev64 = 1 };

constexpr uint32_t kChunkBytes = 4096;        // BufferedRng's refill
constexpr uint32_t kChainRecordBytes = 192;   // aes_ctr_drbg.hpp: 44 round-key words + the counter, per refill
constexpr uint32_t kDeviceModulusBytes = 144; // sizeof(DeviceModulus) (simple_pir_client_api.cpp asserts it)
constexpr uint32_t kHintTileRows = 64;        // hint rows of a workgroup of the product: one per lane of a wavefront
constexpr uint32_t kHintWaves = 4;            // its wavefronts: each takes a quarter of the columns
constexpr size_t kStagingWords = size_t(1) << 24;  // 8-byte words of the un-noised sample staged per block of secret rows
constexpr size_t kMaxBatch = size_t(1) << 20;

// Array2d.randomCenteredBinomialDistribution (Array2d.swift:394-405): k = ceil(2 sigma^2) trial bits a side in
// ceil(k / 64) UInt64 each, the last word of each side masked to k mod 64 bits.
//   stdDev32 (3.2): 2 * 10.24 = 20.48 -> k = 21, 1 + 1 words, mask 2^21 - 1
//   stdDev64 (6.4): 2 * 40.96 = 81.92 -> k = 82, 2 + 2 words, mask 2^18 - 1 on words 1 and 3
struct ErrorSampler {
    uint32_t k = 0, words_per_side = 0, stream_bytes = 0;  // stream_bytes = 16 words_per_side: whole AES blocks
    uint64_t last_word_mask = 0;
};
inline bool error_sampler(int std_dev, ErrorSampler& out) {
    if (std_dev != kStdDev32 && std_dev != kStdDev64) return false;
    out.k = std_dev == kStdDev32 ? 21 : 82;
    out.words_per_side = (out.k + 63) / 64;
    out.stream_bytes = 16 * out.words_per_side;
    out.last_word_mask = out.k % 64 != 0 ? (uint64_t(1) << (out.k % 64)) - 1 : ~uint64_t(0);
    return true;
}

// ---- divideAndRound(initialMod: p, newMod: 2^c) (Array2d.swift:489-514): floor((x 2^c + (p >> 1)) / p) mod 2^c ----------------
// p has c + 1 significant bits, c <= 60, x < p.  The dividend n = x 2^c + (p >> 1) is below p 2^c <= 2^(2c+1), so the quotient is
// below 2^c (the final reduction changes nothing) and Barrett's estimate with k = c + 1 applies: with
//   mu = floor(2^(2c+2) / p) < 2^(c+2),   q' = floor(floor(n / 2^c) mu / 2^(c+2)),
// q - 2 <= q' <= q (HAC 14.42: n < 2^(2k), 2^(k-1) <= p < 2^k).  The remainder n - q' p is below 3p < 2^63: it is formed in one
// word and at most two subtractions fix q' up.
struct Division {
    uint64_t p = 0, mu = 0, half = 0, mask = 0;
    uint32_t c = 0;
};
inline Division division_for(uint64_t p, uint32_t c) {
    Division d;
    d.p = p;
    d.c = c;
    d.half = p >> 1;
    d.mask = (uint64_t(1) << c) - 1;
    d.mu = static_cast<uint64_t>((static_cast<unsigned __int128>(1) << (2 * c + 2)) / p);
    return d;
}
HEAMD_SIMPLE_PIR_CLIENT_HD inline uint64_t divide_and_round(uint64_t x, const Division& d) {
    const uint32_t c = d.c;  // 1 <= c <= 60
    uint64_t lo = x << c, hi = x >> (64 - c);
    lo += d.half;
    hi += lo < d.half ? 1 : 0;
    const uint64_t top = (lo >> c) | (hi << (64 - c));  // floor(n / 2^c) < 2^(c+1)
    const unsigned __int128 product = static_cast<unsigned __int128>(top) * d.mu;
    uint64_t q = static_cast<uint64_t>(product >> (c + 2));
    uint64_t r = lo - q * d.p;  // (mod 2^64: the true remainder is below 3p)
    if (r >= d.p) {
        r -= d.p;
        ++q;
    }
    if (r >= d.p) ++q;
    return q & d.mask;
}

// ---- secret x hint -------------------------------------------------------------------------------------------------------------
// A lane adds terms of at most p (a hint word h < p for a secret +1, p - h <= p for a secret -1) into one 64-bit word; a fold
// leaves a word below p, which counts as one term.  fold_terms = floor((2^64 - 1) / p) is the largest number of such terms a
// word holds without wrapping: fold_terms p <= 2^64 - 1 < (fold_terms + 1) p.
inline uint64_t fold_terms(uint64_t p) { return ~uint64_t(0) / p; }
// 2-bit codes of one secret row: 16 to a 4-byte word
inline size_t code_words_per_row(uint32_t n) { return n < 16 ? 1 : n / 16; }
// Secret rows per read of the hint.  Registers: one 64-bit accumulator per row and lane, 32 VGPRs of a budget of 128 that keeps
// four wavefronts on a SIMD.  LDS: the codes of a pass are held a slab of kCodeSlabColumns columns at a time (N = 1024: the
// whole row, 256 bytes), so a longer row costs no more; with the partial sums a workgroup takes hint_product_lds_bytes().
constexpr uint32_t kSecretRowsPerPass = 16;
constexpr uint32_t kCodeSlabColumns = 1024;
// LDS of a workgroup of the product: the codes of a slab, and one partial sum per (secret row, hint row)
inline size_t hint_product_lds_bytes() {
    return size_t(kSecretRowsPerPass) * (kCodeSlabColumns / 16) * 4 + size_t(kSecretRowsPerPass) * kHintTileRows * 8;
}

struct Shape {
    uint32_t plaintext_bits = 0, ciphertext_bits = 0, lattice_dimension = 0, word_bits = 0;
    size_t entry_count = 0, entry_size_in_bytes = 0, entry_size_in_scalar = 0, entries_per_column = 0, chunks_per_entry = 0,
           database_columns = 0, column_size = 0, a_poly_count = 0;
    uint64_t modulus = 0;
};

struct Plan {
    size_t chunk_size = 0;                 // SimplePirParameters.chunkSize = ceil(entry_size_in_scalar / chunks_per_entry)
    size_t query_words = 0, result_words = 0;
    ErrorSampler sampler;
    size_t error_chunks = 0;               // 4096-byte refills of one query's error stream
    uint32_t secret_rows_per_pass = 0;
    uint64_t fold_terms = 0;
    size_t row_block = 0;                  // secret rows staged at a time by encrypt_zero
    size_t hint_product_lds_bytes = 0;
    size_t rows = 0;                       // B C
    // workspace of encrypt_zero: [error chain | secrets in Eval form | staged sample]
    size_t error_chain_bytes = 0, secret_eval_bytes = 0, staging_bytes = 0;
    // of secret x hint for B C rows: the codes
    size_t codes_bytes = 0;
    // of precompute in front of those: [ternary chain | secrets]
    size_t secret_chain_bytes = 0, secrets_bytes = 0;
    // of a_polynomials: [modulus table | chain | 8-byte polynomials (4-byte words only)]
    size_t a_table_bytes = 0, a_chain_bytes = 0, a_wide_bytes = 0;
    // of decrypt_responses: the decrypted coefficients [B][C chunk_size]
    size_t coefficients_bytes = 0;
    size_t encrypt_zero_bytes() const { return error_chain_bytes + secret_eval_bytes + staging_bytes; }
    size_t precompute_bytes() const { return secret_chain_bytes + secrets_bytes + encrypt_zero_bytes() + codes_bytes; }
    size_t a_polynomials_bytes() const { return a_table_bytes + a_chain_bytes + a_wide_bytes; }
};

// The codes of `rows` secret rows
inline size_t codes_bytes(uint32_t n, size_t rows) { return round16(rows * 4 * code_words_per_row(n)); }

// The plan of a shape he_simple_pir_shape accepted.  forced_row_block: HEAMD_SIMPLE_PIR_CLIENT_ROW_BLOCK (0: none); it lowers
// the block and never raises it.  false: an unknown standard deviation or a batch above kMaxBatch.
inline bool plan(const Shape& s, int std_dev, size_t batch, size_t forced_row_block, Plan& out) {
    Plan p;
    if (!error_sampler(std_dev, p.sampler) || batch > kMaxBatch) return false;
    const uint32_t n = s.lattice_dimension;
    const size_t word_bytes = s.word_bits / 8;
    p.secret_rows_per_pass = kSecretRowsPerPass;
    p.chunk_size = (s.entry_size_in_scalar + s.chunks_per_entry - 1) / s.chunks_per_entry;
    p.query_words = s.chunks_per_entry * s.database_columns;
    p.result_words = s.chunks_per_entry * s.column_size;
    p.error_chunks = (p.query_words * p.sampler.stream_bytes + kChunkBytes - 1) / kChunkBytes;
    p.fold_terms = fold_terms(s.modulus);
    p.hint_product_lds_bytes = hint_product_lds_bytes();
    p.rows = batch * s.chunks_per_entry;
    const size_t row_words = s.a_poly_count * n;
    size_t block = kStagingWords / row_words;
    if (block == 0) block = 1;
    if (forced_row_block != 0 && forced_row_block < block) block = forced_row_block;
    if (p.rows != 0 && p.rows < block) block = p.rows;
    p.row_block = block;
    p.error_chain_bytes = round16(batch * p.error_chunks * kChainRecordBytes);
    p.secret_eval_bytes = round16(block * n * 8);
    p.staging_bytes = round16(block * row_words * 8);
    p.codes_bytes = codes_bytes(n, p.rows);
    const size_t ternary_chunks = (size_t(12) * n + kChunkBytes - 1) / kChunkBytes;
    p.secret_chain_bytes = round16(p.rows * ternary_chunks * kChainRecordBytes);
    p.secrets_bytes = round16(p.rows * n * word_bytes);
    p.a_table_bytes = round16(s.a_poly_count * kDeviceModulusBytes);
    p.a_chain_bytes = round16((row_words + 255) / 256 * kChainRecordBytes);
    p.a_wide_bytes = s.word_bits == 32 ? round16(row_words * 8) : 0;
    p.coefficients_bytes = round16(batch * s.chunks_per_entry * p.chunk_size * word_bytes);
    out = p;
    return true;
}

}  // namespace simple_pir_client
}  // namespace heamd
