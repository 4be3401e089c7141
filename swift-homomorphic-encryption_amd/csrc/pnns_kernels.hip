// pnns_kernels.hip -- the PNNS server database (reference Sources/PrivateNearestNeighborSearch/) on the device:
// Array2d<Float>.normalizedScaledAndRounded (Util.swift:74-89) and the diagonal packing of PlaintextMatrix.diagonalPlaintexts
// (PlaintextMatrix.swift:417-483) up to the slab Context.encodeSimd (Encoding.swift:222-234) hands to inverseNtt.  The
// inverse NTT over [t] and Plaintext.convertToEvalFormat that follow are the existing kernels (pnns_api.cpp).
// And the server's response: the baby-step giant-step inner products of PlaintextMatrix.mulTranspose(vector:using:)
// (MatrixMultiplication.swift:195-212) for all giant steps and up to four queries in one pass over the matrix.
// And CiphertextMatrix.extractDenseRow (CiphertextMatrix.swift:252-370) for query matrices of several rows: the masks, and the
// product of every query ciphertext with the masks of all the rows packed in it.
#include "kernels.hpp"
#include "launch_grid.hpp"
#include "pnns_values.hpp"

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
                value = pnns_signed_to_residue(values[row * shape.cols + column], t, shape.reduce != 0, outside);
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

// ---- mulTranspose(vector:): the inner products of every giant step ----------------------------------------------------------
// With b the baby step, G the giant step, P = nextPowerOfTwo(cols), C = ceil(rows / N) and rot[j] the query rotated j times
// (Eval), MatrixMultiplication.swift:195-212 computes, per giant step g and result c,
//     w[g][c] = sum_{j < min(b, P - g b)} rot[j] * matrix[(g b + j) C + c]           (Bfv.innerProduct, Bfv.swift:476-505)
// Every plaintext of the matrix belongs to exactly one (g, c), and rot depends on neither: a workgroup owns 64 lanes' worth of
// (modulus, coefficient) columns -- 16 bytes per lane, contiguous along N -- keeps the b x QN x 2 rotated ciphertext rows of
// those columns in LDS for its whole life, and its wavefronts walk the (g, c) items, each streaming its item's plaintexts
// once from HBM, kBsgsDepth 16-byte loads ahead across item boundaries.  The last giant step's shorter sum is the item's own
// loop bound.  QN queries share every plaintext word.  Sums are lazy and folded on `cadence` (at most the reference's
// maxLazyProductAccumulationCount; the canonical result does not depend on it).
// FAST: N >= 64 lanes x 16 bytes, so a wavefront's columns lie in one residue row (wave-uniform modulus: the carry-counting
// sums of device_math.hpp) and the LDS tile is used.  !FAST (tiny degrees, or a baby step whose tile does not fit LDS): one
// query, the rotated rows straight from memory, per-lane modulus, 128-bit sums.
// Four queries of 8-byte words keep 16 carry-counting sums per lane: more registers than a lane of a 512-lane workgroup has,
// so that form runs four wavefronts (twice the registers each) and keeps twice the loads in flight per wavefront instead.
template <typename W, int QN>
constexpr unsigned kBsgsThreads = (sizeof(W) == 8 && QN == 4) ? 256 : 512;
template <typename W, int QN>
constexpr unsigned kBsgsDepth = (sizeof(W) == 8 && QN == 4) ? 8 : 4;

struct BsgsShape {
    size_t plaintext_words;  // L N: words of a plaintext, of a ciphertext polynomial
    size_t rot_step_words;   // from rot[j] to rot[j + 1]
    uint32_t baby_step, giant_step, padded_cols;
    uint32_t columns, first_column, group_columns;  // C; this launch covers results [first_column, first_column + group_columns)
    uint32_t out_queries;                           // queries of the whole call: out is [giant_step][out_queries][group_columns]
    uint64_t cadence;
};

template <typename W, bool FAST, bool NARROW, int R>
struct BsgsSums;
template <bool NARROW, int R>
struct BsgsSums<uint64_t, true, NARROW, R> {
    using Sum = ProductSum;
    static __device__ __forceinline__ Sum zero() { return product_sum_zero(); }
    static __device__ __forceinline__ void add_all(Sum (&s)[R], const uint64_t (&x)[R], uint64_t y) {
        product_sum_add_all<R, NARROW>(s, x, y);
    }
    static __device__ __forceinline__ uint64_t reduce(const Sum& s, const DeviceModulus& m) { return reduce_product_sum(s, m); }
    static __device__ __forceinline__ Sum from_residue(uint64_t r) {
        Sum s = product_sum_zero();
        s.t = r;
        return s;
    }
};
template <bool NARROW, int R>
struct BsgsSums<uint64_t, false, NARROW, R> {
    using Sum = U128;
    static __device__ __forceinline__ Sum zero() { return U128{0, 0}; }
    static __device__ __forceinline__ void add_all(Sum (&s)[R], const uint64_t (&x)[R], uint64_t y) {
#pragma unroll
        for (int r = 0; r < R; ++r) mac128(s[r], x[r], y);
    }
    static __device__ __forceinline__ uint64_t reduce(const Sum& s, const DeviceModulus& m) {
        return barrett_reduce128(s, m.p, m.barrett128_lo, m.barrett128_hi);
    }
    static __device__ __forceinline__ Sum from_residue(uint64_t r) { return U128{r, 0}; }
};
template <bool FAST, bool NARROW, int R>
struct BsgsSums<uint32_t, FAST, NARROW, R> {  // products below 2^60: 64-bit sums, folded at least every 15 terms
    using Sum = uint64_t;
    static __device__ __forceinline__ Sum zero() { return 0; }
    static __device__ __forceinline__ void add_all(Sum (&s)[R], const uint64_t (&x)[R], uint64_t y) {
#pragma unroll
        for (int r = 0; r < R; ++r) s[r] = mad32(lo32(x[r]), lo32(y), s[r]);
    }
    static __device__ __forceinline__ uint64_t reduce(const Sum& s, const DeviceModulus& m) {
        if constexpr (FAST) return barrett_reduce64_uniform(s, m.p, m.barrett64);
        else return barrett_reduce64(s, m.p, m.barrett64);
    }
    static __device__ __forceinline__ Sum from_residue(uint64_t r) { return r; }
};

// the 16 bytes of a lane as words
template <typename W>
__device__ __forceinline__ void bsgs_words(const uint4& v, uint64_t (&out)[16 / sizeof(W)]) {
    if constexpr (sizeof(W) == 8) {
        out[0] = pack64(v.x, v.y);
        out[1] = pack64(v.z, v.w);
    } else {
        out[0] = v.x;
        out[1] = v.y;
        out[2] = v.z;
        out[3] = v.w;
    }
}

// where a wavefront is in its sequence of (item, j) steps; every field is wave-uniform
struct BsgsCursor {
    uint32_t item, giant, column, j, count;
    bool done;
};

template <typename W, int QN, bool NARROW, bool FAST>
__global__ __launch_bounds__((kBsgsThreads<W, QN>)) void pnns_bsgs_inner_product_kernel(const W* __restrict__ rot,
                                                                                      const W* __restrict__ matrix,
                                                                                      W* __restrict__ out,
                                                                                      const DeviceContext ctx,
                                                                                      const BsgsShape shape) {
    constexpr unsigned kVector = 16 / sizeof(W), kThreads = kBsgsThreads<W, QN>, kWaves = kThreads / 64;
    constexpr unsigned kDepth = kBsgsDepth<W, QN>;
    constexpr int R = 2 * QN;  // rotated ciphertext rows per step: (query, polynomial)
    static_assert(FAST || QN == 1, "the general form answers one query per launch");
    using Sums = BsgsSums<W, FAST, NARROW, R>;
    extern __shared__ __attribute__((aligned(16))) uint4 bsgs_tile[];  // FAST: [baby_step][R][64 lanes]
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t words = shape.plaintext_words;
    const size_t block_word = static_cast<size_t>(blockIdx.x) * 64u * kVector;
    const size_t word = block_word + static_cast<size_t>(lane) * kVector;  // words is a multiple of kVector
    if constexpr (FAST) {  // every lane is inside the polynomial: words is a multiple of 64 kVector
        const uint32_t rows = shape.baby_step * R;
        for (uint32_t i = threadIdx.x; i < rows * 64u; i += kThreads) {
            const uint32_t row = i >> 6, j = row / R, r = row - j * R;
            bsgs_tile[i] = *reinterpret_cast<const uint4*>(rot + j * shape.rot_step_words + r * words + block_word +
                                                           static_cast<size_t>(i & 63u) * kVector);
        }
        __syncthreads();
    } else {
        if (word >= words) return;  // no barrier below
    }
    const DeviceModulus m = ctx.moduli[(FAST ? block_word : word) >> ctx.log_degree];
    const uint32_t total = shape.giant_step * shape.group_columns;
    const uint32_t stride = gridDim.y * kWaves;
    auto enter = [&](BsgsCursor& at) {  // at.item < total
        at.giant = at.item / shape.group_columns;
        at.column = at.item - at.giant * shape.group_columns;
        at.j = 0;
        const uint32_t left = shape.padded_cols - at.giant * shape.baby_step;
        at.count = left < shape.baby_step ? left : shape.baby_step;
    };
    auto advance = [&](BsgsCursor& at) {  // past the last step the cursor stays on it, done
        if (at.done) return;
        if (at.j + 1 < at.count) {
            ++at.j;
        } else if (at.item + stride < total) {
            at.item += stride;
            enter(at);
        } else {
            at.done = true;
        }
    };
    BsgsCursor fetch{};
    fetch.item = blockIdx.y * kWaves + wave;
    if (fetch.item >= total) return;  // after the barrier
    enter(fetch);
    BsgsCursor use = fetch;
    const W* lane_matrix = matrix + word;
    auto load = [&](const BsgsCursor& at) {  // the matrix is read once: streamed past the caches
        const size_t plaintext =
            (static_cast<size_t>(at.giant) * shape.baby_step + at.j) * shape.columns + shape.first_column + at.column;
        typedef uint32_t Words4 __attribute__((ext_vector_type(4)));
        const Words4 v = __builtin_nontemporal_load(reinterpret_cast<const Words4*>(lane_matrix + plaintext * words));
        return uint4{v.x, v.y, v.z, v.w};
    };
    // a wavefront's loads end with its steps: past the last one nothing is fetched (the branch is wave-uniform)
    uint4 ring[kDepth];
#pragma unroll
    for (unsigned d = 0; d < kDepth; ++d) {
        ring[d] = uint4{0, 0, 0, 0};
        if (!fetch.done) ring[d] = load(fetch);
        advance(fetch);
    }
    typename Sums::Sum acc[kVector][R];
#pragma unroll
    for (unsigned v = 0; v < kVector; ++v)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[v][r] = Sums::zero();
    uint64_t since_reduce = 0;
    while (!use.done) {
#pragma unroll
        for (unsigned d = 0; d < kDepth; ++d) {
            if (use.done) break;
            uint64_t y[kVector];
            bsgs_words<W>(ring[d], y);
            if (!fetch.done) ring[d] = load(fetch);
            advance(fetch);
            uint64_t x[kVector][R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                uint4 operand;
                if constexpr (FAST) operand = bsgs_tile[(use.j * R + r) * 64u + lane];
                else operand = *reinterpret_cast<const uint4*>(rot + use.j * shape.rot_step_words + r * words + word);
                uint64_t parts[kVector];
                bsgs_words<W>(operand, parts);
#pragma unroll
                for (unsigned v = 0; v < kVector; ++v) x[v][r] = parts[v];
            }
#pragma unroll
            for (unsigned v = 0; v < kVector; ++v) Sums::add_all(acc[v], x[v], y[v]);
            ++since_reduce;
            if (use.j + 1 == use.count) {  // the item's sum is complete: out[giant][query][column][polynomial]
                since_reduce = 0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    W folded[kVector];
#pragma unroll
                    for (unsigned v = 0; v < kVector; ++v) {
                        folded[v] = static_cast<W>(Sums::reduce(acc[v][r], m));
                        acc[v][r] = Sums::zero();
                    }
                    const size_t polynomial =
                        ((static_cast<size_t>(use.giant) * shape.out_queries + (r >> 1)) * shape.group_columns + use.column) * 2 +
                        (r & 1);
                    uint4 packed;
                    if constexpr (sizeof(W) == 8) {
                        packed = uint4{lo32(folded[0]), hi32(folded[0]), lo32(folded[1]), hi32(folded[1])};
                    } else {
                        packed = uint4{folded[0], folded[1], folded[2], folded[3]};
                    }
                    *reinterpret_cast<uint4*>(out + polynomial * words + word) = packed;
                }
            } else if (since_reduce >= shape.cadence) {
                since_reduce = 0;
#pragma unroll
                for (unsigned v = 0; v < kVector; ++v)
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[v][r] = Sums::from_residue(Sums::reduce(acc[v][r], m));
            }
            advance(use);
        }
    }
}

}  // namespace

hipError_t launch_pnns_quantize_rows(const float* vectors, size_t rows, size_t cols, float scaling_factor, int64_t* out,
                                     hipStream_t stream) {
    if (rows == 0 || cols == 0) return hipSuccess;
    const size_t rows_per_block = kQuantizeThreads / kQuantizeLanesPerRow;
    const size_t blocks = (rows + rows_per_block - 1) / rows_per_block;
    const unsigned grid = launch_grid::grid_for_blocks(blocks, kQuantizeThreads, kQuantizeGridCap);
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
    if (!launch_grid::launch_fits(blocks, kPackThreads) || last_run - first_run >= 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pnns_diagonal_pack_kernel<W>, dim3(static_cast<unsigned>(blocks), static_cast<unsigned>(last_run - first_run + 1)),
                       dim3(kPackThreads), 0, stream, reinterpret_cast<const long long*>(values), slot_of_word, shape, staging,
                       out_of_range);
    return hipGetLastError();
}
template hipError_t launch_pnns_diagonal_pack<uint64_t>(const int64_t*, const uint32_t*, const PnnsMatrixLayout&, size_t, size_t,
                                                        uint64_t*, uint32_t*, hipStream_t);
template hipError_t launch_pnns_diagonal_pack<uint32_t>(const int64_t*, const uint32_t*, const PnnsMatrixLayout&, size_t, size_t,
                                                        uint32_t*, uint32_t*, hipStream_t);

namespace {
template <typename W, int QN, bool NARROW, bool FAST>
hipError_t launch_bsgs(const W* rot, const W* matrix, W* out, const DeviceContext& ctx, const BsgsShape& shape,
                       size_t tile_bytes, hipStream_t stream) {
    constexpr unsigned kVector = 16 / sizeof(W), kThreads = kBsgsThreads<W, QN>, kWaves = kThreads / 64;
    auto kernel = pnns_bsgs_inner_product_kernel<W, QN, NARROW, FAST>;
    const size_t word_blocks = (shape.plaintext_words + 64 * kVector - 1) / (64 * kVector);
    const size_t items = static_cast<size_t>(shape.giant_step) * shape.group_columns;
    // workgroups over the (g, c) items of one word block: what the tile leaves room for on a compute unit (160 KiB of LDS,
    // 2048 lanes), a few rounds of it across the chip, and no more than the items can feed
    size_t resident = FAST ? (size_t(160) << 10) / tile_bytes : 4;
    if (resident > 2048 / kThreads) resident = 2048 / kThreads;
    if (resident == 0) resident = 1;
    size_t splits = (256 * resident * 2 + word_blocks - 1) / word_blocks;
    const size_t useful = (items + kWaves - 1) / kWaves;
    if (splits > useful) splits = useful;
    if (splits == 0) splits = 1;
    if (!launch_grid::launch_fits(word_blocks, kThreads) || splits > 65535) return hipErrorInvalidValue;
    if (FAST && tile_bytes > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(tile_bytes));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(word_blocks), static_cast<unsigned>(splits)), dim3(kThreads),
                       FAST ? tile_bytes : 0, stream, rot, matrix, out, ctx, shape);
    return hipGetLastError();
}
}  // namespace

unsigned pnns_bsgs_queries_per_pass(const PnnsBsgsLayout& layout, size_t word_bytes, size_t queries) {
    const size_t vector = 16 / word_bytes;
    const size_t words = static_cast<size_t>(layout.moduli_count) << layout.log_degree;
    if (queries == 0 || words % (64 * vector) != 0 || (size_t(1) << layout.log_degree) < 64 * vector) return 1;  // general form
    size_t per_pass = queries < 4 ? queries : 4;
    while (per_pass > 0 && size_t(layout.baby_step) * 2 * per_pass * 1024 > kPnnsBsgsTileLimit) --per_pass;
    return per_pass == 0 ? 1 : static_cast<unsigned>(per_pass);
}

template <typename W>
hipError_t launch_pnns_bsgs_inner_product(const W* rot, const W* matrix, W* out, const DeviceContext& ctx,
                                          const PnnsBsgsLayout& layout, unsigned queries, hipStream_t stream) {
    if (layout.group_columns == 0 || queries == 0) return hipSuccess;
    constexpr size_t kVector = 16 / sizeof(W);
    BsgsShape shape{};
    shape.plaintext_words = static_cast<size_t>(layout.moduli_count) << layout.log_degree;
    shape.rot_step_words = layout.rot_step_words;
    shape.baby_step = layout.baby_step;
    shape.giant_step = layout.giant_step;
    shape.padded_cols = layout.padded_cols;
    shape.columns = layout.columns;
    shape.first_column = layout.first_column;
    shape.group_columns = layout.group_columns;
    shape.out_queries = layout.out_queries;
    if (shape.plaintext_words % kVector != 0 || ctx.moduli_count != layout.moduli_count) return hipErrorInvalidValue;
    if (static_cast<size_t>(layout.giant_step) * layout.group_columns > INT32_MAX) return hipErrorInvalidValue;  // (no launch guard: the kernel counts its (g, c) items in 32 bits)
    const size_t tile_bytes = size_t(layout.baby_step) * 2 * queries * 1024;
    const bool fast = shape.plaintext_words % (64 * kVector) == 0 && (size_t(1) << layout.log_degree) >= 64 * kVector &&
                      tile_bytes <= kPnnsBsgsTileLimit;
    uint64_t cadence = layout.cadence < layout.max_lazy ? layout.cadence : layout.max_lazy;
    if (sizeof(W) == 4) {
        if (cadence > 15) cadence = 15;  // 15 x 2^60 + a folded residue stays below 2^64
    } else if (!fast) {
        cadence = layout.max_lazy;  // the 128-bit accumulator wraps where the reference's does
    }
    const bool narrow = sizeof(W) == 8 && fast && layout.narrow_moduli;
    if (narrow && cadence > kNarrowProductSumCadence) cadence = kNarrowProductSumCadence;
    shape.cadence = cadence == 0 ? 1 : cadence;
    if (!fast) {
        if (queries != 1) return hipErrorInvalidValue;
        return launch_bsgs<W, 1, false, false>(rot, matrix, out, ctx, shape, 0, stream);
    }
#define HEAMD_BSGS_CASE(QN)                                                                                       \
    case QN:                                                                                                      \
        return narrow ? launch_bsgs<W, QN, sizeof(W) == 8, true>(rot, matrix, out, ctx, shape, tile_bytes, stream) \
                      : launch_bsgs<W, QN, false, true>(rot, matrix, out, ctx, shape, tile_bytes, stream)
    switch (queries) {
        HEAMD_BSGS_CASE(1);
        HEAMD_BSGS_CASE(2);
        HEAMD_BSGS_CASE(3);
        HEAMD_BSGS_CASE(4);
        default: return hipErrorInvalidValue;
    }
#undef HEAMD_BSGS_CASE
}
template hipError_t launch_pnns_bsgs_inner_product<uint64_t>(const uint64_t*, const uint64_t*, uint64_t*, const DeviceContext&,
                                                             const PnnsBsgsLayout&, unsigned, hipStream_t);
template hipError_t launch_pnns_bsgs_inner_product<uint32_t>(const uint32_t*, const uint32_t*, uint32_t*, const DeviceContext&,
                                                             const PnnsBsgsLayout&, unsigned, hipStream_t);

// ---- extractDenseRow: the masks and the masked rows -----------------------------------------------------------------------
namespace {
constexpr unsigned kRowThreads = 256;

struct RowMaskBatch {
    PnnsRowMask rows[kPnnsRowsPerLaunch];
    uint32_t padded_cols, log_degree;
};

// Word w of the slab holds SIMD slot slot_of_word[w] (Encoding.swift:228-230): the stores are contiguous, the pattern is
// evaluated at the slot.  blockIdx.y: the row of this launch.
template <typename W>
__global__ __launch_bounds__(kRowThreads) void pnns_row_mask_kernel(const uint32_t* __restrict__ slot_of_word,
                                                                    const RowMaskBatch batch, W* __restrict__ staging) {
    const size_t n = size_t(1) << batch.log_degree;
    const size_t word = static_cast<size_t>(blockIdx.x) * kRowThreads + threadIdx.x;
    if (word >= n) return;
    const PnnsRowMask row = batch.rows[blockIdx.y];
    const uint64_t slot = slot_of_word[word];
    uint64_t end = row.lower + static_cast<uint64_t>(row.copies) * row.period;  // mask.prefix(degree)
    if (end > n) end = n;
    const bool one = slot >= row.lower && slot < end && ((slot - row.lower) & (row.period - 1u)) < batch.padded_cols;
    staging[static_cast<size_t>(blockIdx.y) * n + word] = one ? W(1) : W(0);
}

struct ExtractBatch {
    uint32_t positions[kPnnsRowsPerLaunch];  // where in `out` each row goes
    uint32_t count, first_row;               // the rows of this launch: masks first_row + i
    uint32_t ciphertext, query_ciphertexts;
    size_t poly_words;                       // L N
};

// A lane owns 16 bytes of one polynomial of one client's query ciphertext (blockIdx.y: polynomial, blockIdx.z: client): it
// reads them once and, per row packed in the ciphertext, multiplies them with the same 16 bytes of the row's mask and stores
// the product into the row's own ciphertext.  The masks are re-read by every client and both polynomials (cached); queries
// and rows are touched once (streamed).  UNIFORM: N >= 64 lanes x 16 bytes, so a wavefront lies in one residue row and the
// modulus is wave-uniform.  The product is he_bfv_mul_plain_device's (device_math.hpp barrett_mul).
template <typename W, bool UNIFORM>
__global__ __launch_bounds__(kRowThreads) void pnns_extract_rows_kernel(const W* __restrict__ queries,
                                                                        const W* __restrict__ masks, W* __restrict__ out,
                                                                        const DeviceContext ctx, const ExtractBatch batch) {
    constexpr unsigned kVector = 16 / sizeof(W);
    typedef uint32_t Words4 __attribute__((ext_vector_type(4)));
    const size_t word = (static_cast<size_t>(blockIdx.x) * kRowThreads + threadIdx.x) * kVector;
    if (word >= batch.poly_words) return;  // poly_words is a multiple of kVector
    uint32_t row_of_modulus = static_cast<uint32_t>(word >> ctx.log_degree);
    if constexpr (UNIFORM) row_of_modulus = __builtin_amdgcn_readfirstlane(row_of_modulus);
    const DeviceModulus* modulus = ctx.moduli + row_of_modulus;
    const uint64_t p = modulus->p, factor = modulus->product_factor;
    const int shift = static_cast<int>(modulus->product_shift);
    const size_t client = blockIdx.z, polynomial = blockIdx.y;
    const size_t source = ((client * batch.query_ciphertexts + batch.ciphertext) * 2 + polynomial) * batch.poly_words + word;
    const Words4 loaded = __builtin_nontemporal_load(reinterpret_cast<const Words4*>(queries + source));
    uint64_t x[kVector];
    bsgs_words<W>(uint4{loaded.x, loaded.y, loaded.z, loaded.w}, x);
    for (uint32_t i = 0; i < batch.count; ++i) {  // wave-uniform
        const uint4 mask = *reinterpret_cast<const uint4*>(masks + static_cast<size_t>(batch.first_row + i) * batch.poly_words + word);
        uint64_t y[kVector];
        bsgs_words<W>(mask, y);
        uint64_t product[kVector];
#pragma unroll
        for (unsigned v = 0; v < kVector; ++v) product[v] = barrett_mul(x[v], y[v], p, factor, shift);
        Words4 packed;
        if constexpr (sizeof(W) == 8) {
            packed = Words4{lo32(product[0]), hi32(product[0]), lo32(product[1]), hi32(product[1])};
        } else {
            packed = Words4{lo32(product[0]), lo32(product[1]), lo32(product[2]), lo32(product[3])};
        }
        const size_t target = static_cast<size_t>(batch.positions[i]) * gridDim.z + client;  // position-major over clients
        __builtin_nontemporal_store(packed, reinterpret_cast<Words4*>(out + (target * 2 + polynomial) * batch.poly_words + word));
    }
}
}  // namespace

template <typename W>
hipError_t launch_pnns_row_masks(const uint32_t* slot_of_word, const PnnsRowMask* rows, size_t count, uint32_t padded_cols,
                                 uint32_t log_degree, W* staging, hipStream_t stream) {
    const size_t n = size_t(1) << log_degree;
    const unsigned blocks = static_cast<unsigned>((n + kRowThreads - 1) / kRowThreads);
    for (size_t first = 0; first < count; first += kPnnsRowsPerLaunch) {
        const unsigned now = static_cast<unsigned>(count - first < kPnnsRowsPerLaunch ? count - first : kPnnsRowsPerLaunch);
        RowMaskBatch batch{};
        for (unsigned i = 0; i < now; ++i) batch.rows[i] = rows[first + i];
        batch.padded_cols = padded_cols;
        batch.log_degree = log_degree;
        hipLaunchKernelGGL(pnns_row_mask_kernel<W>, dim3(blocks, now), dim3(kRowThreads), 0, stream, slot_of_word, batch,
                           staging + first * n);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
template hipError_t launch_pnns_row_masks<uint64_t>(const uint32_t*, const PnnsRowMask*, size_t, uint32_t, uint32_t, uint64_t*,
                                                    hipStream_t);
template hipError_t launch_pnns_row_masks<uint32_t>(const uint32_t*, const PnnsRowMask*, size_t, uint32_t, uint32_t, uint32_t*,
                                                    hipStream_t);

template <typename W>
hipError_t launch_pnns_extract_rows(const W* queries, const W* masks, W* out, const DeviceContext& ctx,
                                    const PnnsExtractLayout& layout, uint32_t ciphertext, uint32_t first_row,
                                    const uint32_t* positions, size_t count, hipStream_t stream) {
    constexpr size_t kVector = 16 / sizeof(W);
    if (count == 0 || layout.clients == 0) return hipSuccess;
    const size_t n = size_t(1) << ctx.log_degree;
    const size_t poly_words = static_cast<size_t>(ctx.moduli_count) * n;
    const size_t blocks = (poly_words / kVector + kRowThreads - 1) / kRowThreads;
    if (poly_words % kVector != 0 || !launch_grid::launch_fits(blocks, kRowThreads) || layout.clients > 65535) return hipErrorInvalidValue;
    const bool uniform = n >= 64 * kVector;
    for (size_t first = 0; first < count; first += kPnnsRowsPerLaunch) {
        const unsigned now = static_cast<unsigned>(count - first < kPnnsRowsPerLaunch ? count - first : kPnnsRowsPerLaunch);
        ExtractBatch batch{};
        for (unsigned i = 0; i < now; ++i) batch.positions[i] = positions[first + i];
        batch.count = now;
        batch.first_row = first_row + static_cast<uint32_t>(first);
        batch.ciphertext = ciphertext;
        batch.query_ciphertexts = static_cast<uint32_t>(layout.query_ciphertexts);
        batch.poly_words = poly_words;
        const dim3 grid(static_cast<unsigned>(blocks), 2, static_cast<unsigned>(layout.clients));
        if (uniform) {
            hipLaunchKernelGGL((pnns_extract_rows_kernel<W, true>), grid, dim3(kRowThreads), 0, stream, queries, masks, out, ctx,
                               batch);
        } else {
            hipLaunchKernelGGL((pnns_extract_rows_kernel<W, false>), grid, dim3(kRowThreads), 0, stream, queries, masks, out, ctx,
                               batch);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
template hipError_t launch_pnns_extract_rows<uint64_t>(const uint64_t*, const uint64_t*, uint64_t*, const DeviceContext&,
                                                       const PnnsExtractLayout&, uint32_t, uint32_t, const uint32_t*, size_t,
                                                       hipStream_t);
template hipError_t launch_pnns_extract_rows<uint32_t>(const uint32_t*, const uint32_t*, uint32_t*, const DeviceContext&,
                                                       const PnnsExtractLayout&, uint32_t, uint32_t, const uint32_t*, size_t,
                                                       hipStream_t);

}  // namespace heamd
