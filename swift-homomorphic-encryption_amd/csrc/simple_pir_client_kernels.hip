// simple_pir_client_kernels.hip -- the SimplePIR client (reference Sources/PrivateInformationRetrieval/SimplePir/
// SimplePir+Client.swift, SimplePir+Precompute.swift:116-311) on the device:
//   noiselessSample                 SimplePir+Client.swift:29-50     a_k * s per secret, between the existing transforms
//   divideAndRound + error + mask   Array2d.swift:382-429, 489-514   one finishing kernel; the error is drawn in registers
//   secretMatrix.multiply(transposing: hint, modulus: p)   SimplePir+Precompute.swift:122-188   the hint product below
//   add(index:), extractEntries, integrate, decrypt        :241-311, SimplePir+Client.swift:85-121
//
// The hint product.  The secrets are ternary, so the reference's 128-bit multiply-accumulate over n is
//   results[r][j] = (sum_{s[r][n] = +1} hint[j][n] + sum_{s[r][n] = -1} (p - hint[j][n])) mod p:
// additions of terms of at most p and one reduction.  A prepass packs the secrets to 2-bit codes.  A workgroup of four
// wavefronts owns a tile of 64 hint rows, one per lane, and answers kSecretRowsPerPass secret rows per read of the tile: every
// lane loads 16 bytes of its row at a time (wavefront w takes the 16-byte groups w, w + 4, ...), the codes of the pass sit in
// LDS a slab of kCodeSlabColumns columns at a time and reach the lanes as scalars (the code of (r, n) is the same for every hint
// row), and the wavefronts' sums meet in LDS at the end.  No atomics; a hint word is read from memory once per pass.
// Accumulator bound (simple_pir_client_plan.hpp fold_terms): a lane's 64-bit word holds floor((2^64 - 1) / p) terms of at most
// p; it is folded to below p (one term) before it would take more -- never at p < 2^30 or N <= 1024 with c <= 53, every 6 to
// 14 terms at c = 60.
//
// Every kernel runs on an exact grid, as those of encrypt_kernels.hip and pir_client_kernels.hip: a workgroup of the product owns
// one (pass, tile), a wavefront of the finishing kernel one (secret row, 4096-byte refill) -- the geometry of the samplers --, a
// lane of the others one word or byte it writes; none strides by the grid, and a batch HIP cannot launch is refused.
#include <hip/hip_runtime.h>

#include "aes_ctr_drbg.hpp"
#include "device_math.hpp"
#include "launch_grid.hpp"
#include "simple_pir_client_kernels.hpp"

namespace heamd {
namespace {

using namespace aes;
using simple_pir_client::Division;
using simple_pir_client::kCodeSlabColumns;
using simple_pir_client::kHintTileRows;
using simple_pir_client::kHintWaves;
using simple_pir_client::kSecretRowsPerPass;

constexpr unsigned kThreads = 256;

// ---- noiselessSample ------------------------------------------------------------------------------------------------------------
template <typename W>
__global__ void __launch_bounds__(kThreads)
    simple_pir_client_widen_kernel(const W* __restrict__ secrets, uint64_t* __restrict__ out, size_t words) {
    const size_t i = blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x;  // (an exact grid)
    if (i < words)
        out[i] = static_cast<uint64_t>(secrets[i]);
}

// staging [rows][blocks][N] = a_eval [blocks][N] * secret_eval [rows][N]
template <typename W>
__global__ void __launch_bounds__(kThreads)
    simple_pir_client_products_kernel(const W* __restrict__ a_eval, const uint64_t* __restrict__ secret_eval,
                                      uint64_t* __restrict__ staging, uint32_t blocks, const DeviceContext ctx, size_t words) {
    const DeviceModulus* m = ctx.moduli;
    const uint64_t p = m->p, factor = m->product_factor;
    const int shift = static_cast<int>(m->product_shift);
    const size_t row_words = static_cast<size_t>(blocks) << ctx.log_degree;
    const size_t i = blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x;  // (an exact grid)
    if (i < words) {
        const size_t row = i / row_words, k = i - row * row_words;
        const size_t n = k & ((size_t(1) << ctx.log_degree) - 1);
        staging[i] = barrett_mul(static_cast<uint64_t>(a_eval[k]), secret_eval[(row << ctx.log_degree) + n], p, factor, shift);
    }
}

// ---- divideAndRound, the error, the mask ------------------------------------------------------------------------------------------
constexpr int kSamplerWaves = 4;
constexpr unsigned kSamplerThreads = 64 * kSamplerWaves;

// UInt64(littleEndianBytes:) of the two halves of a counter block
__device__ __forceinline__ uint64_t block_word(const Block& b, int half) {
    return static_cast<uint64_t>(__builtin_bswap32(b.w[2 * half])) |
           (static_cast<uint64_t>(__builtin_bswap32(b.w[2 * half + 1])) << 32);
}

// BLOCKS counter blocks per coefficient: 1 at stdDev32 (one UInt64 a side), 2 at stdDev64 (two a side).  Wavefront (row, t)
// takes refill first_refill(row) + t of the query's stream and, of its 256 / BLOCKS coefficients, those of the row.
template <typename W, int BLOCKS>
__global__ void __launch_bounds__(kSamplerThreads)
    simple_pir_client_finish_kernel(const uint64_t* __restrict__ staging, size_t staging_row_words,
                                    const uint32_t* __restrict__ chain, size_t error_chunks, uint64_t last_word_mask,
                                    const Division division, size_t chunks, size_t columns, size_t first_row,
                                    uint32_t refills_per_row, size_t total_items, W* __restrict__ queries) {
    __shared__ uint32_t table[256 * kTableCopies];
    fill_table<kTableCopies, kSamplerThreads>(table);
    constexpr uint32_t kCoefficients = kChunkBlocks / BLOCKS;  // per refill
    const uint32_t lane = threadIdx.x & 63;
    const TableView<kTableCopies> te0{table + (lane & (kTableCopies - 1))};
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t item = static_cast<size_t>(blockIdx.x) * kSamplerWaves + wave;  // (an exact grid)
    if (item >= total_items) return;
    const size_t local_row = item / refills_per_row;
    const uint32_t t = static_cast<uint32_t>(item - local_row * refills_per_row);
    const size_t row = first_row + local_row, query = row / chunks, chunk = row - query * chunks;
    const size_t begin = chunk * columns, end = begin + columns;  // the row's coefficients of the query's stream
    const size_t refill = begin / kCoefficients + t;
    if (refill * kCoefficients >= end) return;  // (wave-uniform: the row's last refills may be fewer than refills_per_row)
    const uint32_t* record = chain + (query * error_chunks + refill) * kRecordWords;
    uint32_t rk[44];
#pragma unroll
    for (int i = 0; i < 44; ++i) rk[i] = record[i];
    const Block v{{record[44], record[45], record[46], record[47]}};
    const uint64_t* sample = staging + local_row * staging_row_words;
    W* out = queries + row * columns;
#pragma unroll
    for (uint32_t j = 0; j < kCoefficients / 64; ++j) {
        const uint32_t local = 64 * j + lane;
        const size_t coefficient = refill * kCoefficients + local;
        if (coefficient < begin || coefficient >= end) continue;
        // trialBits: BLOCKS words a side, the last of each masked; nonzeroBitCount of each side
        uint32_t positive = 0, negative = 0;
        if constexpr (BLOCKS == 1) {
            const Block b = encrypt(te0, rk, counter_add(v, 1 + local));
            positive = __popcll(block_word(b, 0) & last_word_mask);
            negative = __popcll(block_word(b, 1) & last_word_mask);
        } else {
            const Block b0 = encrypt(te0, rk, counter_add(v, 1 + 2 * local));
            const Block b1 = encrypt(te0, rk, counter_add(v, 2 + 2 * local));
            positive = __popcll(block_word(b0, 0)) + __popcll(block_word(b0, 1) & last_word_mask);
            negative = __popcll(block_word(b1, 0)) + __popcll(block_word(b1, 1) & last_word_mask);
        }
        const size_t column = coefficient - begin;
        // pos.subtractMod(neg, modulus: 2^c), then (sample + error) & mask: wrapping arithmetic under the mask
        const uint64_t word = simple_pir_client::divide_and_round(sample[column], division) + positive - negative;
        out[column] = static_cast<W>(word & division.mask);
    }
}

// ---- secret x hint ----------------------------------------------------------------------------------------------------------------
// One lane per code word: sixteen secret words.  PRECONDITION of the product: every secret word is 0, 1 or p - 1 (anything
// else is packed as 0).
template <typename W>
__global__ void __launch_bounds__(kThreads)
    simple_pir_client_pack_codes_kernel(const W* __restrict__ secrets, uint32_t* __restrict__ codes, uint32_t degree,
                                        uint32_t code_words, uint64_t p, size_t total) {
    const size_t i = blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x;  // (an exact grid)
    if (i < total) {
        const size_t row = i / code_words;
        const uint32_t first = static_cast<uint32_t>(i - row * code_words) * 16;
        const W* words = secrets + row * degree + first;
        uint32_t packed = 0;
        for (uint32_t k = 0; k < 16 && first + k < degree; ++k) {
            const uint64_t s = words[k];
            packed |= (s == 1 ? 1u : s == p - 1 ? 2u : 0u) << (2 * k);
        }
        codes[i] = packed;
    }
}

constexpr unsigned kHintThreads = 64 * kHintWaves;
constexpr uint32_t kSlabWords = kCodeSlabColumns / 16;

// the WORDS hint words at `at`: one 16-byte load where WORDS fills it, a single word otherwise
template <typename W, int WORDS>
__device__ __forceinline__ void load_hint_words(const W* at, uint64_t (&h)[WORDS]) {
    if constexpr (WORDS == 1) {
        h[0] = at[0];
    } else if constexpr (sizeof(W) == 8) {
        const U64x2 pair = *reinterpret_cast<const U64x2*>(at);
        h[0] = pair.x;
        h[1] = pair.y;
    } else {
        const uint4 quad = *reinterpret_cast<const uint4*>(at);
        h[0] = quad.x;
        h[1] = quad.y;
        h[2] = quad.z;
        h[3] = quad.w;
    }
}

// VEC: N is a multiple of the words of a 16-byte load (every N but 2 at 4-byte words); the hint is 16-byte aligned either way
template <typename W, bool VEC>
__global__ void __launch_bounds__(kHintThreads)
    simple_pir_client_hint_product_kernel(const uint32_t* __restrict__ codes, size_t rows, const W* __restrict__ hint,
                                          size_t column_size, W* __restrict__ results, uint32_t degree, uint32_t code_words,
                                          uint64_t fold_terms, uint64_t p, uint64_t barrett64, size_t tiles) {
    constexpr int G = kSecretRowsPerPass;
    constexpr int WORDS = VEC ? 16 / sizeof(W) : 1;
    __shared__ uint32_t lds_codes[G][kSlabWords];
    __shared__ uint64_t partial[G][kHintTileRows];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t item = blockIdx.x;  // (an exact grid: one workgroup per (pass, tile))
    const size_t pass = item / tiles, tile = item - pass * tiles;
    const size_t first_row = pass * G;
    const size_t j = tile * kHintTileRows + lane;
    const bool live = j < column_size;
    const W* row = hint + (live ? j : column_size - 1) * degree;  // an idle lane shadows the last row and stores nothing
    uint64_t acc[G];
#pragma unroll
    for (int r = 0; r < G; ++r) acc[r] = 0;
    uint64_t held = 0;  // acc[r] <= held * p
    for (uint32_t slab = 0; slab < degree; slab += kCodeSlabColumns) {
        const uint32_t slab_columns = degree - slab < kCodeSlabColumns ? degree - slab : kCodeSlabColumns;
        const uint32_t slab_words = (slab_columns + 15) / 16;
        __syncthreads();  // the readers of the slab before
        for (uint32_t i = threadIdx.x; i < G * kSlabWords; i += kHintThreads) {
            const uint32_t r = i / kSlabWords, w = i - r * kSlabWords;
            const size_t secret_row = first_row + r;
            lds_codes[r][w] = secret_row < rows && w < slab_words ? codes[secret_row * code_words + slab / 16 + w] : 0u;
        }
        __syncthreads();
        const uint32_t groups = slab_columns / WORDS;
        for (uint32_t g = wave; g < groups; g += kHintWaves) {
            const uint32_t column = g * WORDS;  // of the slab; a group lies in one code word
            uint64_t h[WORDS], minus[WORDS];
            load_hint_words<W, WORDS>(row + slab + column, h);
#pragma unroll
            for (int i = 0; i < WORDS; ++i) minus[i] = p - h[i];
            const uint32_t word = column / 16, shift = (column % 16) * 2;
#pragma unroll
            for (int r = 0; r < G; ++r) {
                const uint32_t code_bits = __builtin_amdgcn_readfirstlane(lds_codes[r][word]) >> shift;
#pragma unroll
                for (int i = 0; i < WORDS; ++i) {
                    const uint32_t code = (code_bits >> (2 * i)) & 3u;  // wave-uniform
                    const uint64_t term = code == 2 ? minus[i] : h[i];
                    acc[r] += code != 0 ? term : 0;
                }
            }
            held += WORDS;
            if (held + WORDS > fold_terms) {  // wave-uniform
#pragma unroll
                for (int r = 0; r < G; ++r) acc[r] = barrett_reduce64(acc[r], p, barrett64);
                held = 1;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < G; ++r) acc[r] = barrett_reduce64(acc[r], p, barrett64);
    // the four wavefronts' sums, each below p, one after the other: below 4p < 2^63
    for (uint32_t w = 0; w < kHintWaves; ++w) {
        if (wave == w) {
#pragma unroll
            for (int r = 0; r < G; ++r) partial[r][lane] = (w == 0 ? 0 : partial[r][lane]) + acc[r];
        }
        __syncthreads();
    }
    for (uint32_t r = wave; r < G; r += kHintWaves) {
        const size_t secret_row = first_row + r;
        if (live && secret_row < rows)
            results[secret_row * column_size + j] = static_cast<W>(barrett_reduce64(partial[r][lane], p, barrett64));
    }
    // the codes and the sums are the secrets': nothing of them stays in LDS
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < G * kSlabWords; i += kHintThreads) lds_codes[i / kSlabWords][i % kSlabWords] = 0;
    for (uint32_t i = threadIdx.x; i < G * kHintTileRows; i += kHintThreads) partial[i / kHintTileRows][i % kHintTileRows] = 0;
}

// ---- add(index:), integrate, decrypt ----------------------------------------------------------------------------------------------
// one lane per (query, chunk): queries[b][q][(q + index chunks) / entries_per_column] += delta, masked
template <typename W>
__global__ void __launch_bounds__(kThreads)
    simple_pir_client_add_indices_kernel(W* __restrict__ queries, const unsigned long long* __restrict__ indices,
                                         uint32_t* __restrict__ flags, const SimplePirClientLayout layout, size_t total) {
    const size_t i = blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x;  // (an exact grid)
    if (i < total) {
        const uint64_t b = i / layout.chunks, q = i - b * layout.chunks;
        const uint64_t index = indices[b];
        const bool valid = index < layout.entry_count;
        if (q == 0 && flags != nullptr) flags[b] = valid ? 0u : 1u;
        if (valid) {
            const uint64_t column = (q + index * layout.chunks) / layout.entries_per_column;
            W* word = queries + (b * layout.chunks + q) * layout.database_columns + column;
            *word = static_cast<W>((static_cast<uint64_t>(*word) + layout.delta) & layout.mask);
        }
    }
}

// one lane per extracted coefficient: ((response - result + (delta >> 1)) & mask) >> (c - plaintext_bits), wrapping in the word
template <typename W>
__global__ void __launch_bounds__(kThreads)
    simple_pir_client_integrate_kernel(const W* __restrict__ responses, const W* __restrict__ results,
                                       const unsigned long long* __restrict__ indices, W* __restrict__ coefficients,
                                       uint32_t* __restrict__ flags, const SimplePirClientLayout layout, size_t total) {
    const uint64_t per_query = layout.chunks * layout.chunk_size;
    const size_t i = blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x;  // (an exact grid)
    if (i < total) {
        const uint64_t b = i / per_query, at = i - b * per_query;
        const uint64_t q = at / layout.chunk_size, k = at - q * layout.chunk_size;
        const uint64_t index = indices[b];
        const bool valid = index < layout.entry_count;
        if (at == 0 && flags != nullptr) flags[b] = valid ? 0u : 1u;
        W value = 0;
        if (valid) {
            const uint64_t entry = q + index * layout.chunks;  // extractEntries
            const uint64_t start = (b * layout.chunks + q) * layout.column_size +
                                   (entry % layout.entries_per_column) * layout.chunk_size + k;
            const W difference = static_cast<W>(responses[start] - results[start] + static_cast<W>(layout.delta >> 1));
            value = static_cast<W>((difference & static_cast<W>(layout.mask)) >> layout.shift);
        }
        coefficients[i] = value;
    }
}

// one lane per byte: stream bit s of a query is bit bits - 1 - (s mod bits) of coefficient s / bits, MSB first
// (CoefficientPacking.swift:155-216); the coefficients are below 2^bits
template <typename W>
__global__ void __launch_bounds__(kThreads)
    simple_pir_client_entry_bytes_kernel(const W* __restrict__ coefficients, uint8_t* __restrict__ entries,
                                         const SimplePirClientLayout layout, size_t total) {
    const uint64_t per_query = layout.chunks * layout.chunk_size, bits = layout.plaintext_bits;
    const size_t i = blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x;  // (an exact grid)
    if (i < total) {
        const uint64_t b = i / layout.entry_size_in_bytes, at = i - b * layout.entry_size_in_bytes;
        const W* mine = coefficients + b * per_query;
        const uint64_t first_bit = at * 8, end_bit = first_bit + 8;
        uint64_t k = first_bit / bits, field = k * bits;
        uint32_t byte = 0;
        while (field < end_bit) {  // at most 8 coefficients, all below ceil(8 entry_size / bits) <= chunks chunk_size
            const uint64_t coefficient = static_cast<uint64_t>(mine[k]);
            const uint64_t from = field > first_bit ? field : first_bit;
            const uint64_t field_end = field + bits, to = field_end < end_bit ? field_end : end_bit;
            const uint64_t part = (coefficient >> (field_end - to)) & ((uint64_t(1) << (to - from)) - 1);
            byte |= static_cast<uint32_t>(part) << (end_bit - to);
            ++k;
            field = field_end;
        }
        entries[i] = static_cast<uint8_t>(byte);
    }
}

template <typename Kernel, typename... Args>
hipError_t launch_exact(Kernel kernel, size_t lanes, hipStream_t stream, Args... args) {
    if (lanes == 0) return hipSuccess;
    const size_t blocks = launch_grid::grid_blocks(lanes, kThreads, launch_grid::kMaxLanes);
    if (!launch_grid::launch_fits(blocks, kThreads)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, stream, args...);
    return hipGetLastError();
}

}  // namespace

template <typename W>
hipError_t launch_simple_pir_client_widen(const W* secrets, uint64_t* out, size_t words, hipStream_t stream) {
    return launch_exact(simple_pir_client_widen_kernel<W>, words, stream, secrets, out, words);
}

template <typename W>
hipError_t launch_simple_pir_client_products(const W* a_eval, const uint64_t* secret_eval, uint64_t* staging, size_t rows,
                                             uint32_t blocks, const DeviceContext& ctx, hipStream_t stream) {
    const size_t words = (rows * blocks) << ctx.log_degree;
    return launch_exact(simple_pir_client_products_kernel<W>, words, stream, a_eval, secret_eval, staging, blocks, ctx, words);
}

template <typename W>
hipError_t launch_simple_pir_client_finish(const uint64_t* staging, size_t staging_row_words, const uint32_t* chain,
                                           size_t error_chunks, const simple_pir_client::ErrorSampler& sampler,
                                           const simple_pir_client::Division& division, size_t chunks, size_t columns,
                                           size_t first_row, size_t rows, W* queries, hipStream_t stream) {
    if (rows == 0 || columns == 0) return hipSuccess;
    if (sampler.words_per_side != 1 && sampler.words_per_side != 2) return hipErrorInvalidValue;
    const size_t coefficients = kChunkBlocks / sampler.words_per_side;
    // a row of `columns` coefficients touches at most this many refills, wherever in the stream it begins
    const size_t refills_per_row = (columns + coefficients - 1) / coefficients + 1;
    if (refills_per_row > 0xffffffffull) return hipErrorInvalidValue;
    const size_t total = rows * refills_per_row;
    const size_t blocks = launch_grid::grid_blocks(total, kSamplerWaves, SIZE_MAX);
    if (!launch_grid::launch_fits(blocks, kSamplerThreads)) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>(blocks));
    if (sampler.words_per_side == 1)
        hipLaunchKernelGGL((simple_pir_client_finish_kernel<W, 1>), grid, dim3(kSamplerThreads), 0, stream, staging,
                           staging_row_words, chain, error_chunks, sampler.last_word_mask, division, chunks, columns, first_row,
                           static_cast<uint32_t>(refills_per_row), total, queries);
    else
        hipLaunchKernelGGL((simple_pir_client_finish_kernel<W, 2>), grid, dim3(kSamplerThreads), 0, stream, staging,
                           staging_row_words, chain, error_chunks, sampler.last_word_mask, division, chunks, columns, first_row,
                           static_cast<uint32_t>(refills_per_row), total, queries);
    return hipGetLastError();
}

template <typename W>
hipError_t launch_simple_pir_client_pack_codes(const W* secrets, uint32_t* codes, size_t rows, uint32_t degree, uint64_t p,
                                               hipStream_t stream) {
    const uint32_t code_words = static_cast<uint32_t>(simple_pir_client::code_words_per_row(degree));
    const size_t total = rows * code_words;
    return launch_exact(simple_pir_client_pack_codes_kernel<W>, total, stream, secrets, codes, degree, code_words, p, total);
}

template <typename W>
hipError_t launch_simple_pir_client_hint_product(const uint32_t* codes, size_t rows, const W* hint, size_t column_size,
                                                 W* results, uint32_t rows_per_pass, uint64_t fold_terms, uint32_t degree,
                                                 uint64_t p, uint64_t barrett64, hipStream_t stream) {
    if (rows == 0 || column_size == 0) return hipSuccess;
    constexpr uint32_t kVectorWords = 16 / sizeof(W);
    // the kernel is built for the plan's pass; a word must hold a fold (one term) and the terms of one more load
    if (rows_per_pass != kSecretRowsPerPass || fold_terms < kVectorWords + 1) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(hint) & 15u) != 0) return hipErrorInvalidValue;
    const uint32_t code_words = static_cast<uint32_t>(simple_pir_client::code_words_per_row(degree));
    const size_t tiles = (column_size + kHintTileRows - 1) / kHintTileRows;
    const size_t passes = (rows + rows_per_pass - 1) / rows_per_pass;
    const size_t items = tiles * passes;
    if (!launch_grid::launch_fits(items, kHintThreads)) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>(items));
    if (degree % kVectorWords == 0)
        hipLaunchKernelGGL((simple_pir_client_hint_product_kernel<W, true>), grid, dim3(kHintThreads), 0, stream, codes, rows, hint,
                           column_size, results, degree, code_words, fold_terms, p, barrett64, tiles);
    else
        hipLaunchKernelGGL((simple_pir_client_hint_product_kernel<W, false>), grid, dim3(kHintThreads), 0, stream, codes, rows, hint,
                           column_size, results, degree, code_words, fold_terms, p, barrett64, tiles);
    return hipGetLastError();
}

template <typename W>
hipError_t launch_simple_pir_client_add_indices(W* queries, const uint64_t* indices, uint32_t* flags,
                                                const SimplePirClientLayout& layout, size_t batch, hipStream_t stream) {
    const size_t total = batch * layout.chunks;
    return launch_exact(simple_pir_client_add_indices_kernel<W>, total, stream, queries,
                          reinterpret_cast<const unsigned long long*>(indices), flags, layout, total);
}

template <typename W>
hipError_t launch_simple_pir_client_integrate(const W* responses, const W* results, const uint64_t* indices, W* coefficients,
                                              uint32_t* flags, const SimplePirClientLayout& layout, size_t batch,
                                              hipStream_t stream) {
    const size_t total = batch * layout.chunks * layout.chunk_size;
    return launch_exact(simple_pir_client_integrate_kernel<W>, total, stream, responses, results,
                          reinterpret_cast<const unsigned long long*>(indices), coefficients, flags, layout, total);
}

template <typename W>
hipError_t launch_simple_pir_client_entry_bytes(const W* coefficients, uint8_t* entries, const SimplePirClientLayout& layout,
                                                size_t batch, hipStream_t stream) {
    const size_t total = batch * layout.entry_size_in_bytes;
    return launch_exact(simple_pir_client_entry_bytes_kernel<W>, total, stream, coefficients, entries, layout, total);
}

#define HEAMD_SIMPLE_PIR_CLIENT_INSTANCES(W)                                                                                   \
    template hipError_t launch_simple_pir_client_widen<W>(const W*, uint64_t*, size_t, hipStream_t);                          \
    template hipError_t launch_simple_pir_client_products<W>(const W*, const uint64_t*, uint64_t*, size_t, uint32_t,          \
                                                             const DeviceContext&, hipStream_t);                              \
    template hipError_t launch_simple_pir_client_finish<W>(const uint64_t*, size_t, const uint32_t*, size_t,                  \
                                                           const simple_pir_client::ErrorSampler&,                            \
                                                           const simple_pir_client::Division&, size_t, size_t, size_t,        \
                                                           size_t, W*, hipStream_t);                                          \
    template hipError_t launch_simple_pir_client_pack_codes<W>(const W*, uint32_t*, size_t, uint32_t, uint64_t, hipStream_t); \
    template hipError_t launch_simple_pir_client_hint_product<W>(const uint32_t*, size_t, const W*, size_t, W*, uint32_t,     \
                                                                 uint64_t, uint32_t, uint64_t, uint64_t, hipStream_t);        \
    template hipError_t launch_simple_pir_client_add_indices<W>(W*, const uint64_t*, uint32_t*, const SimplePirClientLayout&, \
                                                                size_t, hipStream_t);                                         \
    template hipError_t launch_simple_pir_client_integrate<W>(const W*, const W*, const uint64_t*, W*, uint32_t*,             \
                                                              const SimplePirClientLayout&, size_t, hipStream_t);             \
    template hipError_t launch_simple_pir_client_entry_bytes<W>(const W*, uint8_t*, const SimplePirClientLayout&, size_t,     \
                                                                hipStream_t);
HEAMD_SIMPLE_PIR_CLIENT_INSTANCES(uint64_t)
HEAMD_SIMPLE_PIR_CLIENT_INSTANCES(uint32_t)
#undef HEAMD_SIMPLE_PIR_CLIENT_INSTANCES

}  // namespace heamd
