// simple_pir_matrix_kernels.hip -- SimplePirServer.computeResponse for large request batches on the int8 matrix cores
// (v_mfma_i32_16x16x64_i8).  The arithmetic and the tile constants: simple_pir_batch_plan.hpp.
//
//   responses[q][r] = (sum_c database[r][c] * requests[q][c]) & mask
//
// The database rows are the A operand (M = 16 rows, K = 64 columns, each lane 16 contiguous K bytes: its 16-byte row load IS
// the fragment for 1-byte elements; 2-byte elements are split in registers into a low and a high limb fragment).  The request
// limbs are the B operand with N = 16 requests of one limb j.  The K sum is commutative and both fragments are loaded by the
// same rule (byte k of the lane's fragment is column 64 step + 16 (lane >> 4) + k), so nothing here depends on the
// instruction's operand lane map beyond "lane & 15 is the row / the column"; the result map (col = lane & 15,
// row = 4 (lane >> 4) + reg) is type-independent on gfx950.  A lane therefore holds the same request in every class
// accumulator, the recombination sum_s acc_s << 7s stays in its registers, and it stores 4 consecutive rows of one request.
//
// A workgroup of four wavefronts owns kBlockRows = 128 rows (two 16-row tiles per wavefront) and walks the columns in tiles
// of KS K-steps.  Per tile it loads the requests' words, issues the NEXT tile's database loads (so the database stream stays
// in flight across the staging), splits the words into limbs and writes them to LDS as a [n][k] byte image
// (n = (request tile * classes + limb) * 16 + request, row stride padded by 16 bytes), and then every wavefront multiplies its
// two row tiles with every staged fragment.  The i32 accumulators are folded into word accumulators every `fold_steps`
// K-steps: a limb product is at most 127^2, so fold_columns * database_limbs * 16129 <= INT32_MAX keeps them non-negative.
#include <climits>

#include "device_math.hpp"
#include "kernels.hpp"
#include "launch_grid.hpp"
#include "simple_pir_batch_plan.hpp"

namespace heamd {

namespace {

using namespace simple_pir_batch;

constexpr unsigned kMatrixThreads = 256, kWaveRowTiles = 2;
static_assert(kBlockRows == (kMatrixThreads / 64) * kWaveRowTiles * 16, "rows of a workgroup");
static_assert(natural_fold_columns(1) * kLimbProduct <= INT32_MAX && natural_fold_columns(2) * 2 * kLimbProduct <= INT32_MAX,
              "the i32 accumulators stay non-negative between folds");

typedef int Frag __attribute__((ext_vector_type(4)));  // 16 int8 of an operand, or 4 i32 of a result

// K-steps per column tile: the tile's database bytes per lane (and the staged request words per thread) stay the same
template <typename W, unsigned LIMBS>
constexpr unsigned tile_steps() {
    return (sizeof(W) == 4 ? 4 : 2) / LIMBS;
}

// the 16 elements a lane takes of row `row` at `column`: LIMBS chunks of 16 bytes, zeros outside the database
template <unsigned LIMBS>
__device__ __forceinline__ void load_row_chunks(const uint8_t* __restrict__ database, size_t rows, size_t columns, size_t row,
                                                size_t column, bool aligned, Frag (&raw)[LIMBS]) {
    constexpr unsigned kPerChunk = 16 / LIMBS;  // elements per 16 bytes
#pragma unroll
    for (unsigned h = 0; h < LIMBS; ++h) {
        raw[h] = Frag{0, 0, 0, 0};
        const size_t first = column + h * kPerChunk;
        if (row < rows && first < columns) {
            const uint8_t* source = database + (row * columns + first) * LIMBS;
            if (aligned) {
                raw[h] = __builtin_nontemporal_load(reinterpret_cast<const Frag*>(source));
            } else if constexpr (LIMBS == 1) {
#pragma unroll
                for (unsigned e = 0; e < 16; ++e)
                    if (first + e < columns) raw[h][e >> 2] |= static_cast<int>(static_cast<uint32_t>(source[e]) << (8 * (e & 3)));
            } else {
                const uint16_t* wide = reinterpret_cast<const uint16_t*>(source);
#pragma unroll
                for (unsigned e = 0; e < 8; ++e)
                    if (first + e < columns) raw[h][e >> 1] |= static_cast<int>(static_cast<uint32_t>(wide[e]) << (16 * (e & 1)));
            }
        }
    }
}

// 16 two-byte elements (below 2^14) -> the fragment of their low 7 bits and the fragment of the bits above
__device__ __forceinline__ void split_limbs(const Frag (&raw)[2], Frag& lo, Frag& hi) {
#pragma unroll
    for (unsigned w = 0; w < 4; ++w) {
        const uint32_t a = static_cast<uint32_t>(raw[w >> 1][2 * (w & 1)]), b = static_cast<uint32_t>(raw[w >> 1][2 * (w & 1) + 1]);
        // bytes 0 and 2 of each masked word: elements 4w .. 4w + 3 in order
        lo[w] = static_cast<int>(__builtin_amdgcn_perm(b & 0x007f007fu, a & 0x007f007fu, 0x06040200u));
        hi[w] = static_cast<int>(__builtin_amdgcn_perm((b >> 7) & 0x007f007fu, (a >> 7) & 0x007f007fu, 0x06040200u));
    }
}

template <typename W, unsigned LIMBS, unsigned C, unsigned NT>
__global__ __launch_bounds__(kMatrixThreads, 2) void simple_pir_matrix_response_kernel(
    const uint8_t* __restrict__ database, size_t rows, size_t columns, const W* __restrict__ requests, unsigned live_queries,
    W* __restrict__ responses, W mask, unsigned fold_steps) {
    constexpr unsigned KS = tile_steps<W, LIMBS>();
    constexpr unsigned kTileColumns = KS * kKStep;
    constexpr unsigned kStride = kTileColumns + 16;             // bytes of an image row: 16-byte reads of 16 rows hit 64 banks
    constexpr unsigned kImageRows = NT * C * kRequestTile;
    constexpr unsigned kQueries = NT * kRequestTile;
    constexpr unsigned kItems = kQueries * (kTileColumns / 4) / kMatrixThreads;  // 4 columns of one request per item
    static_assert(kQueries * (kTileColumns / 4) % kMatrixThreads == 0, "whole items per thread");
    static_assert(kImageRows * kStride <= 64 * 1024, "static LDS");
    __shared__ __attribute__((aligned(16))) uint8_t image[kImageRows * kStride];

    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned lane_n = lane & 15, lane_k = lane >> 4;
    const size_t first_row = static_cast<size_t>(blockIdx.x) * kBlockRows + wave * (kWaveRowTiles * 16);
    // 16-byte loads need 16-byte rows; anything else takes the element-wise loads (wave-uniform choices)
    const bool aligned = (columns * LIMBS) % 16 == 0 && (reinterpret_cast<uintptr_t>(database) & 15u) == 0;
    const bool requests_aligned = columns % 4 == 0 && (reinterpret_cast<uintptr_t>(requests) & 15u) == 0;

    Frag acc[kWaveRowTiles][NT][C];
    W folded[kWaveRowTiles][NT][4];
#pragma unroll
    for (unsigned m = 0; m < kWaveRowTiles; ++m)
#pragma unroll
        for (unsigned t = 0; t < NT; ++t) {
#pragma unroll
            for (unsigned s = 0; s < C; ++s) acc[m][t][s] = Frag{0, 0, 0, 0};
#pragma unroll
            for (unsigned i = 0; i < 4; ++i) folded[m][t][i] = 0;
        }
    auto fold = [&]() {
#pragma unroll
        for (unsigned m = 0; m < kWaveRowTiles; ++m)
#pragma unroll
            for (unsigned t = 0; t < NT; ++t)
#pragma unroll
                for (unsigned i = 0; i < 4; ++i) {
                    W sum = 0;
#pragma unroll
                    for (unsigned s = 0; s < C; ++s) {
                        sum += static_cast<W>(static_cast<uint32_t>(acc[m][t][s][i])) << (kLimbBits * s);
                        acc[m][t][s][i] = 0;
                    }
                    folded[m][t][i] += sum;
                }
    };

    Frag next[kWaveRowTiles][KS][LIMBS];
    auto load_tile = [&](size_t tile) {
#pragma unroll
        for (unsigned m = 0; m < kWaveRowTiles; ++m)
#pragma unroll
            for (unsigned ks = 0; ks < KS; ++ks)
                load_row_chunks<LIMBS>(database, rows, columns, first_row + m * 16 + lane_n,
                                       tile + ks * kKStep + lane_k * 16, aligned, next[m][ks]);
    };
    load_tile(0);

    unsigned since_fold = 0;
    for (size_t tile = 0; tile < columns; tile += kTileColumns) {
        // this tile's request words, 4 columns of one request per item
        W words[kItems][4];
#pragma unroll
        for (unsigned it = 0; it < kItems; ++it) {
            const unsigned item = threadIdx.x + it * kMatrixThreads;
            const unsigned q = item / (kTileColumns / 4), c4 = item % (kTileColumns / 4);
            const size_t column = tile + 4 * c4;
#pragma unroll
            for (unsigned e = 0; e < 4; ++e) words[it][e] = 0;
            if (q < live_queries && column < columns) {
                const W* source = requests + static_cast<size_t>(q) * columns + column;
                if (requests_aligned) {
                    if constexpr (sizeof(W) == 4) {
                        const Frag v = *reinterpret_cast<const Frag*>(source);
#pragma unroll
                        for (unsigned e = 0; e < 4; ++e) words[it][e] = static_cast<W>(static_cast<uint32_t>(v[e]));
                    } else {
                        const Frag v0 = *reinterpret_cast<const Frag*>(source), v1 = *reinterpret_cast<const Frag*>(source + 2);
                        words[it][0] = static_cast<W>(static_cast<uint32_t>(v0[0]) | (static_cast<uint64_t>(static_cast<uint32_t>(v0[1])) << 32));
                        words[it][1] = static_cast<W>(static_cast<uint32_t>(v0[2]) | (static_cast<uint64_t>(static_cast<uint32_t>(v0[3])) << 32));
                        words[it][2] = static_cast<W>(static_cast<uint32_t>(v1[0]) | (static_cast<uint64_t>(static_cast<uint32_t>(v1[1])) << 32));
                        words[it][3] = static_cast<W>(static_cast<uint32_t>(v1[2]) | (static_cast<uint64_t>(static_cast<uint32_t>(v1[3])) << 32));
                    }
                } else {
#pragma unroll
                    for (unsigned e = 0; e < 4; ++e)
                        if (column + e < columns) words[it][e] = source[e];
                }
            }
        }
        // this tile's database chunks move to `now`; the next tile's loads go out before anything waits
        Frag now[kWaveRowTiles][KS][LIMBS];
#pragma unroll
        for (unsigned m = 0; m < kWaveRowTiles; ++m)
#pragma unroll
            for (unsigned ks = 0; ks < KS; ++ks)
#pragma unroll
                for (unsigned h = 0; h < LIMBS; ++h) now[m][ks][h] = next[m][ks][h];
        if (tile + kTileColumns < columns) load_tile(tile + kTileColumns);

        __syncthreads();  // the previous tile's readers are done
#pragma unroll
        for (unsigned it = 0; it < kItems; ++it) {
            const unsigned item = threadIdx.x + it * kMatrixThreads;
            const unsigned q = item / (kTileColumns / 4), c4 = item % (kTileColumns / 4);
            const unsigned t = q / kRequestTile, n = q % kRequestTile;
#pragma unroll
            for (unsigned j = 0; j < C; ++j) {
                uint32_t packed = 0;
#pragma unroll
                for (unsigned e = 0; e < 4; ++e)
                    packed |= (static_cast<uint32_t>(words[it][e] >> (kLimbBits * j)) & 127u) << (8 * e);
                *reinterpret_cast<uint32_t*>(image + ((t * C + j) * kRequestTile + n) * kStride + 4 * c4) = packed;
            }
        }
        __syncthreads();

#pragma unroll
        for (unsigned ks = 0; ks < KS; ++ks) {
            Frag a[kWaveRowTiles][LIMBS];
#pragma unroll
            for (unsigned m = 0; m < kWaveRowTiles; ++m) {
                if constexpr (LIMBS == 1) a[m][0] = now[m][ks][0];
                else split_limbs(now[m][ks], a[m][0], a[m][1]);
            }
#pragma unroll
            for (unsigned t = 0; t < NT; ++t)
#pragma unroll
                for (unsigned j = 0; j < C; ++j) {
                    const Frag b = *reinterpret_cast<const Frag*>(image + ((t * C + j) * kRequestTile + lane_n) * kStride +
                                                                  ks * kKStep + lane_k * 16);
#pragma unroll
                    for (unsigned m = 0; m < kWaveRowTiles; ++m) {
                        acc[m][t][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[m][0], b, acc[m][t][j], 0, 0, 0);
                        if constexpr (LIMBS == 2) {
                            if (j + 1 < C) acc[m][t][j + 1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[m][1], b, acc[m][t][j + 1], 0, 0, 0);
                        }
                    }
                }
            if (++since_fold == fold_steps) {
                fold();
                since_fold = 0;
            }
        }
    }
    fold();

    // the lane holds rows 4 lane_k .. 4 lane_k + 3 of each of its row tiles for request lane_n of each request tile
#pragma unroll
    for (unsigned m = 0; m < kWaveRowTiles; ++m)
#pragma unroll
        for (unsigned t = 0; t < NT; ++t) {
            const unsigned q = t * kRequestTile + lane_n;
#pragma unroll
            for (unsigned i = 0; i < 4; ++i) {
                const size_t r = first_row + m * 16 + 4 * lane_k + i;
                if (q < live_queries && r < rows) responses[static_cast<size_t>(q) * rows + r] = folded[m][t][i] & mask;
            }
        }
}

template <typename W, unsigned LIMBS, unsigned C, unsigned NT>
hipError_t matrix_pass(const void* database, size_t rows, size_t columns, const W* requests, unsigned live, W* responses,
                       W mask, unsigned fold_steps, hipStream_t stream) {
    const size_t blocks = (rows + kBlockRows - 1) / kBlockRows;
    if (!launch_grid::launch_fits(blocks, kMatrixThreads)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((simple_pir_matrix_response_kernel<W, LIMBS, C, NT>), dim3(static_cast<unsigned>(blocks)),
                       dim3(kMatrixThreads), 0, stream, static_cast<const uint8_t*>(database), rows, columns, requests, live,
                       responses, mask, fold_steps);
    return hipGetLastError();
}

template <typename W, unsigned LIMBS, unsigned C>
hipError_t matrix_classes(const void* database, size_t rows, size_t columns, const W* requests, size_t query_count,
                          W* responses, W mask, unsigned fold_steps, hipStream_t stream) {
    constexpr unsigned kPass = requests_per_pass_of(C, 8 * sizeof(W));
    // passes of kPass requests; a last pass of at most 16 takes the one-tile kernel (its spare slots multiply zeros)
    for (size_t q = 0; q < query_count;) {
        const size_t left = query_count - q;
        const unsigned live = static_cast<unsigned>(left < kPass ? left : kPass);
        hipError_t status;
        if constexpr (kPass == 2 * kRequestTile) {
            if (live > kRequestTile)
                status = matrix_pass<W, LIMBS, C, 2>(database, rows, columns, requests + q * columns, live, responses + q * rows, mask, fold_steps, stream);
            else
                status = matrix_pass<W, LIMBS, C, 1>(database, rows, columns, requests + q * columns, live, responses + q * rows, mask, fold_steps, stream);
        } else {
            status = matrix_pass<W, LIMBS, C, 1>(database, rows, columns, requests + q * columns, live, responses + q * rows, mask, fold_steps, stream);
        }
        if (status != hipSuccess) return status;
        q += live;
    }
    return hipSuccess;
}

template <typename W, unsigned LIMBS>
hipError_t matrix_limbs(const void* database, size_t rows, size_t columns, const W* requests, size_t query_count, W* responses,
                        uint32_t ciphertext_bits, size_t fold_columns, hipStream_t stream) {
    const W mask = ciphertext_bits >= 8 * sizeof(W) ? ~W(0) : static_cast<W>((W(1) << ciphertext_bits) - 1);
    const size_t natural = natural_fold_columns(LIMBS);
    const size_t cadence = fold_columns == 0 || fold_columns > natural ? natural : fold_columns;  // never above the bound
    const unsigned fold_steps = static_cast<unsigned>(cadence / kKStep ? cadence / kKStep : 1);
#define HEAMD_MATRIX_CLASSES(C) \
    case C: return matrix_classes<W, LIMBS, C>(database, rows, columns, requests, query_count, responses, mask, fold_steps, stream);
    switch (classes_of(ciphertext_bits)) {
        HEAMD_MATRIX_CLASSES(1)
        HEAMD_MATRIX_CLASSES(2)
        HEAMD_MATRIX_CLASSES(3)
        HEAMD_MATRIX_CLASSES(4)
        HEAMD_MATRIX_CLASSES(5)
        default: break;
    }
    if constexpr (sizeof(W) == 8) {
        switch (classes_of(ciphertext_bits)) {
            HEAMD_MATRIX_CLASSES(6)
            HEAMD_MATRIX_CLASSES(7)
            HEAMD_MATRIX_CLASSES(8)
            HEAMD_MATRIX_CLASSES(9)
            HEAMD_MATRIX_CLASSES(10)
            default: break;
        }
    }
#undef HEAMD_MATRIX_CLASSES
    return hipErrorInvalidValue;
}

}  // namespace

template <typename W>
hipError_t launch_simple_pir_matrix_response(const void* database, uint32_t database_limbs, size_t rows, size_t columns,
                                             const W* requests, size_t query_count, W* responses, uint32_t ciphertext_bits,
                                             size_t fold_columns, hipStream_t stream) {
    if (rows == 0 || query_count == 0) return hipSuccess;
    if (ciphertext_bits == 0 || ciphertext_bits > 8 * sizeof(W)) return hipErrorInvalidValue;
    switch (database_limbs) {
        case 1: return matrix_limbs<W, 1>(database, rows, columns, requests, query_count, responses, ciphertext_bits, fold_columns, stream);
        case 2: return matrix_limbs<W, 2>(database, rows, columns, requests, query_count, responses, ciphertext_bits, fold_columns, stream);
        default: return hipErrorInvalidValue;
    }
}
template hipError_t launch_simple_pir_matrix_response<uint64_t>(const void*, uint32_t, size_t, size_t, const uint64_t*, size_t,
                                                                uint64_t*, uint32_t, size_t, hipStream_t);
template hipError_t launch_simple_pir_matrix_response<uint32_t>(const void*, uint32_t, size_t, size_t, const uint32_t*, size_t,
                                                                uint32_t*, uint32_t, size_t, hipStream_t);

}  // namespace heamd
