// pnns_kernels.hip -- the PNNS server database (reference Sources/PrivateNearestNeighborSearch/) on the device:
// Array2d<Float>.normalizedScaledAndRounded (Util.swift:74-89) and the diagonal packing of PlaintextMatrix.diagonalPlaintexts
// (PlaintextMatrix.swift:417-483) up to the slab Context.encodeSimd (Encoding.swift:222-234) hands to inverseNtt.  The
// inverse NTT over [t] and Plaintext.convertToEvalFormat that follow are the existing kernels (pnns_api.cpp).
#include "kernels.hpp"

namespace heamd {

namespace {

// ---- normalizedScaledAndRounded -------------------------------------------------------------------------------------------
// A row belongs to a group of 16 lanes.  The lanes load 16 consecutive floats together (64 contiguous bytes) and square
// them; the ordered sum then takes the 16 squares one at a time from their lanes, so every lane of the group runs the same
// left-to-right float32 accumulation from 0 the reference's reduce(0, +) runs.  A lane past the row's end contributes +0,
// which leaves a non-negative partial sum as it is.  The squares are formed in another lane than the one that adds them and
// the quotient has no addition, so there is nothing the compiler could contract into a fused multiply-add; the pragma says
// so for whatever is added later.  sqrtf and `/` are the correctly rounded forms (hipcc's default for float32); the
// __fsqrt_rn / __fmul_rn family of this toolchain is the native square root and the bare, contractible operators.
constexpr unsigned kQuantizeThreads = 256;
constexpr unsigned kQuantizeLanesPerRow = 16;
constexpr size_t kQuantizeGridCap = size_t(1) << 20;

__global__ __launch_bounds__(kQuantizeThreads) void pnns_quantize_rows_kernel(const float* __restrict__ vectors, size_t rows,
                                                                              size_t cols, float scaling_factor,
                                                                              long long* __restrict__ out) {
#pragma clang fp contract(off)
    const unsigned lane = threadIdx.x % kQuantizeLanesPerRow;
    const size_t rows_per_block = kQuantizeThreads / kQuantizeLanesPerRow;
    const size_t blocks = (rows + rows_per_block - 1) / rows_per_block;
    for (size_t block = blockIdx.x; block < blocks; block += gridDim.x) {  // every lane of a block runs the same trips
        const size_t row = block * rows_per_block + threadIdx.x / kQuantizeLanesPerRow;
        const bool live = row < rows;
        const float* source = vectors + (live ? row : 0) * cols;
        float sum = 0.0f;
        for (size_t base = 0; base < cols; base += kQuantizeLanesPerRow) {
            const size_t column = base + lane;
            const float v = live && column < cols ? source[column] : 0.0f;
            const float square = v * v;
            for (unsigned k = 0; k < kQuantizeLanesPerRow; ++k) sum = sum + __shfl(square, k, kQuantizeLanesPerRow);
        }
        const float norm = sqrtf(sum);
        if (!live) continue;
        long long* target = out + row * cols;
        for (size_t column = lane; column < cols; column += kQuantizeLanesPerRow) {
            long long rounded = 0;
            if (norm != 0.0f) rounded = static_cast<long long>(roundf((source[column] * scaling_factor) / norm));
            target[column] = rounded;
        }
    }
}

// ---- diagonal packing -----------------------------------------------------------------------------------------------------
// With P = nextPowerOfTwo(cols), h = N / 2, b the baby step and data the [rows][cols] matrix, plaintext (diagonal r, chunk c)
// -- index r * plaintextsPerColumn + c -- is encodeSimd of the chunk the reference rotates (PlaintextMatrix.swift:465-478):
//     before rotation  chunk[j] = data[c N + j][(c N + j + r) mod P]   if that column < cols and that row < rows, else 0
//     rotationStep     s = r - r mod b;  rotate(toStartAt: h - s) of each half puts old element (k - s) mod h at place k
//     SIMD slot k      = chunk[(k & h) | ((k - s) & (h - 1))]
//     slab word        encodingMatrix[k] holds slot k                                            (Encoding.swift:228-230)
// so word w of the slab, with k = slot_of_word[w] the inverse of encodingMatrix, is
//     data[R][(R + r) mod P],   R = c N + ((k & h) | ((k - s) & (h - 1))).
// R depends on r only through s, which is one value for the b diagonals of a giant step, and the column grows with r: a run
// of D consecutive diagonals of one giant step reads D consecutive elements (mod P) of row R for word w.
//
// A workgroup therefore owns kPackWords consecutive words of the slabs of kPackDiagonals consecutive diagonals of one giant
// step and one chunk: it reads, for each of its words, the kPackDiagonals-element segment of the word's source row (16 lanes
// read the 128 contiguous bytes of a segment together; every element of the matrix is read from memory exactly once over the
// whole build), parks the converted values in LDS diagonal-major and stores them 16 bytes per lane, kPackWords contiguous
// words per diagonal.  The permutation of encodingMatrix lands on the loads, where it picks whole row segments, and never on
// the stores.  An N-word slab of every diagonal of a run does not fit LDS next to a tile of source rows (N = 8192: 64 KiB per
// diagonal), which is why the permutation is not done slab by slab.
constexpr unsigned kPackThreads = 256;
constexpr unsigned kPackWords = 256;      // slab words per workgroup
constexpr unsigned kPackDiagonals = 16;   // diagonals per run

struct PackShape {
    size_t rows, cols;
    size_t padded_cols;            // P
    size_t plaintexts_per_column;  // ceil(rows / N)
    size_t first, count;           // the plaintexts of this launch: staging slab p - first for first <= p < first + count
    uint64_t t;
    uint32_t log_degree, baby_step, runs_per_giant_step, first_run;
    int reduce;
};

template <typename W>
__global__ __launch_bounds__(kPackThreads) void pnns_diagonal_pack_kernel(const long long* __restrict__ values,
                                                                          const uint32_t* __restrict__ slot_of_word,
                                                                          const PackShape shape, W* __restrict__ staging,
                                                                          uint32_t* __restrict__ out_of_range) {
    constexpr unsigned kVector = 16 / sizeof(W);     // words of a 16-byte store
    constexpr unsigned kPitch = kPackWords + kVector;  // 8-byte words: the 16 diagonals of a store group fall on distinct bank
                                                       // pairs but for d and d + 8 (two-way, free on a store)
    __shared__ __attribute__((aligned(16))) W tile[kPackDiagonals * kPitch];
    const size_t n = size_t(1) << shape.log_degree;
    const uint32_t half = static_cast<uint32_t>(n >> 1);
    const size_t tiles = (n + kPackWords - 1) / kPackWords;
    const size_t chunk = blockIdx.x / tiles;
    const uint32_t first_word = static_cast<uint32_t>(blockIdx.x % tiles) * kPackWords;
    const uint32_t run = shape.first_run + blockIdx.y;
    const uint32_t giant = run / shape.runs_per_giant_step;
    const size_t step = size_t(giant) * shape.baby_step;  // s: the rotation of every diagonal of this run
    const size_t first_diagonal = step + size_t(run % shape.runs_per_giant_step) * kPackDiagonals;
    size_t last_diagonal = step + shape.baby_step;        // one past the run's last
    if (last_diagonal > shape.padded_cols) last_diagonal = shape.padded_cols;
    if (last_diagonal > first_diagonal + kPackDiagonals) last_diagonal = first_diagonal + kPackDiagonals;
    const long long t = static_cast<long long>(shape.t);
    const long long most = (t - 1) >> 1, least = -(t >> 1);
    const size_t end = shape.first + shape.count;

    const unsigned d = threadIdx.x % kPackDiagonals;
    const size_t diagonal = first_diagonal + d;
    const size_t plaintext = diagonal * shape.plaintexts_per_column + chunk;
    const bool wanted = diagonal < last_diagonal && plaintext >= shape.first && plaintext < end;
    bool outside = false;
    for (unsigned i = threadIdx.x / kPackDiagonals; i < kPackWords; i += kPackThreads / kPackDiagonals) {
        const uint32_t word = first_word + i;
        unsigned long long value = 0;
        if (wanted && word < n) {
            const uint32_t slot = slot_of_word[word];
            const uint32_t source = (slot & half) | ((slot - static_cast<uint32_t>(step)) & (half - 1));
            const size_t row = chunk * n + source;
            const size_t column = (row + diagonal) & (shape.padded_cols - 1);
            if (row < shape.rows && column < shape.cols) {
                long long v = values[row * shape.cols + column];
                if (shape.reduce) {  // Modulus.reduce(SignedScalar): the remainder in [0, t)
                    v %= t;
                    if (v < 0) v += t;
                } else {             // centeredToRemainder
                    outside |= v > most || v < least;
                    if (v < 0) v += t;
                }
                value = static_cast<unsigned long long>(v);
            }
        }
        tile[d * kPitch + i] = static_cast<W>(value);
    }
    if (outside && out_of_range != nullptr) *out_of_range = 1u;  // a plain vector store; racing lanes store the same word
    __syncthreads();
    constexpr unsigned kLanesPerDiagonal = kPackWords / kVector;
    const unsigned offset = (threadIdx.x % kLanesPerDiagonal) * kVector;
    for (unsigned e = threadIdx.x / kLanesPerDiagonal; e < kPackDiagonals; e += kPackThreads / kLanesPerDiagonal) {
        const size_t p = (first_diagonal + e) * shape.plaintexts_per_column + chunk;
        if (first_diagonal + e >= last_diagonal || p < shape.first || p >= end) continue;
        W* slab = staging + (p - shape.first) * n + first_word;
        if (first_word + offset + kVector <= n) {
            *reinterpret_cast<uint4*>(slab + offset) = *reinterpret_cast<const uint4*>(&tile[e * kPitch + offset]);
        } else {
            for (unsigned k = 0; k < kVector; ++k)
                if (first_word + offset + k < n) slab[offset + k] = tile[e * kPitch + offset + k];
        }
    }
}

}  // namespace

hipError_t launch_pnns_quantize_rows(const float* vectors, size_t rows, size_t cols, float scaling_factor, int64_t* out,
                                     hipStream_t stream) {
    if (rows == 0 || cols == 0) return hipSuccess;
    const size_t rows_per_block = kQuantizeThreads / kQuantizeLanesPerRow;
    const size_t blocks = (rows + rows_per_block - 1) / rows_per_block;
    const unsigned grid = static_cast<unsigned>(blocks < kQuantizeGridCap ? blocks : kQuantizeGridCap);
    hipLaunchKernelGGL(pnns_quantize_rows_kernel, dim3(grid), dim3(kQuantizeThreads), 0, stream, vectors, rows, cols,
                       scaling_factor, reinterpret_cast<long long*>(out));
    return hipGetLastError();
}

template <typename W>
hipError_t launch_pnns_diagonal_pack(const int64_t* values, const uint32_t* slot_of_word, const PnnsMatrixLayout& layout,
                                     size_t first, size_t count, W* staging, uint32_t* out_of_range, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    const size_t n = size_t(1) << layout.log_degree;
    PackShape shape{};
    shape.rows = layout.rows;
    shape.cols = layout.cols;
    shape.padded_cols = layout.padded_cols;
    shape.plaintexts_per_column = layout.plaintexts_per_column;
    shape.first = first;
    shape.count = count;
    shape.t = layout.plaintext_modulus;
    shape.log_degree = layout.log_degree;
    shape.baby_step = layout.baby_step;
    shape.reduce = layout.reduce;
    // runs of diagonals in diagonal order: those that meet the diagonals [first / ppc, (first + count - 1) / ppc] are launched
    const size_t per_giant = (size_t(layout.baby_step) + kPackDiagonals - 1) / kPackDiagonals;
    shape.runs_per_giant_step = static_cast<uint32_t>(per_giant);
    auto run_of = [&](size_t diagonal) {
        const size_t giant = diagonal / layout.baby_step;
        return giant * per_giant + (diagonal - giant * layout.baby_step) / kPackDiagonals;
    };
    const size_t first_run = run_of(first / layout.plaintexts_per_column);
    const size_t last_run = run_of((first + count - 1) / layout.plaintexts_per_column);
    shape.first_run = static_cast<uint32_t>(first_run);
    const size_t tiles = (n + kPackWords - 1) / kPackWords;
    const size_t blocks = tiles * layout.plaintexts_per_column;
    if (blocks >= (size_t(1) << 31) || last_run - first_run >= 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pnns_diagonal_pack_kernel<W>, dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(last_run - first_run + 1)),
                       dim3(kPackThreads), 0, stream, reinterpret_cast<const long long*>(values), slot_of_word, shape, staging,
                       out_of_range);
    return hipGetLastError();
}
template hipError_t launch_pnns_diagonal_pack<uint64_t>(const int64_t*, const uint32_t*, const PnnsMatrixLayout&, size_t, size_t,
                                                        uint64_t*, uint32_t*, hipStream_t);
template hipError_t launch_pnns_diagonal_pack<uint32_t>(const int64_t*, const uint32_t*, const PnnsMatrixLayout&, size_t, size_t,
                                                        uint32_t*, uint32_t*, hipStream_t);

}  // namespace heamd
