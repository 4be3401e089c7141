// encrypt_kernels.hip -- secret keys, encryptions of zero and key-switch keys made where they are used (reference Sources/
// HomomorphicEncryption/):
//   randomizeTernary                       PolyRq/PolyRq+Randomize.swift:87-104    12 stream bytes per coefficient, mod 3
//   randomizeCenteredBinomialDistribution  PolyRq/PolyRq+Randomize.swift:120-167   16 stream bytes per coefficient, two popcounts
//   Bfv.encryptZero                        Bfv/Bfv+Encrypt.swift:150-181           [-(a s + e), a]
//   Bfv._generateKeySwitchKey              Bfv/Bfv+Keys.swift:69-103               + (q_ks mod q_j) currentKey on row j
// Every random polynomial is a function of a caller-supplied 32-byte seed through NistAes128Ctr(seed:): the byte stream is
// the one seeded_kernels.hip draws `a` from (aes_ctr_drbg.hpp: launch_seeded_chain records the round keys and counter of every
// 4096-byte chunk), and a sampler here gives the words the reference's sampler gives on that generator.
//
// Both samplers take one wavefront per (seed, chunk) and 4 counter blocks per lane, block 64 j + lane in trip j, so that
// the lanes of a wavefront store consecutive coefficients.  The binomial sampler has the geometry of the uniform one: a
// block is a coefficient.  A ternary record is 12 bytes, so the records of a chunk (341 or 342 of them; the pattern repeats
// every 3 chunks = 1024 coefficients) do not line up with its blocks and the last one may end in the first block of the next
// chunk, which lies under other round keys: the wavefront writes its chunk's bytes and that one block to LDS and reads its
// records from there.  2^32 = 1 (mod 3), so a record's 96-bit value mod 3 is the sum of its three 32-bit words mod 3.
//
// Every kernel runs on an exact grid: a wavefront of a sampler owns one (seed, chunk), a lane of the element-wise kernels one
// word, and none strides by the grid; a batch HIP cannot launch is refused, not covered in part.  All stores are ordinary
// vector stores.
#include <hip/hip_runtime.h>

#include "aes_ctr_drbg.hpp"
#include "device_math.hpp"
#include "encrypt_kernels.hpp"
#include "galois_index.hpp"
#include "launch_grid.hpp"

namespace heamd {
namespace {

using namespace aes;

constexpr int kWaves = 4;
constexpr unsigned kSamplerThreads = 64 * kWaves;
constexpr unsigned kThreads = 256;            // the element-wise kernels

// the round keys and the counter of one chunk: wave-uniform, scalar loads
struct ChunkKeys {
    uint32_t rk[44];
    Block v;
};
__device__ __forceinline__ void load_chunk_keys(const uint32_t* record, ChunkKeys& keys) {
#pragma unroll
    for (int i = 0; i < 44; ++i) keys.rk[i] = record[i];
    keys.v = Block{{record[44], record[45], record[46], record[47]}};
}

// The centred binomial draws of the lane's 4 coefficients of a chunk, coefficient 256 chunk + 64 j + lane in e[j]:
// popcount of the low 21 bits of the block's first UInt64 minus that of its second (k = ceil(2 * 3.2 * 3.2) = 21 trial bits a
// side, PolyRq+Randomize.swift:131-160); UInt64(littleEndianBytes:) puts stream bytes 0..3 and 8..11 in the low halves.
constexpr uint32_t kBinomialMask = (1u << 21) - 1;
template <typename Table>
__device__ __forceinline__ void draw_binomial(const Table& te0, const uint32_t* record, uint32_t lane, int32_t (&e)[4]) {
    ChunkKeys keys;
    load_chunk_keys(record, keys);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const Block stream = encrypt(te0, keys.rk, counter_add(keys.v, 1 + 64 * j + lane));
        e[j] = __popc(__builtin_bswap32(stream.w[0]) & kBinomialMask) - __popc(__builtin_bswap32(stream.w[2]) & kBinomialMask);
    }
}
// pos.subtractMod(neg, modulus: p), |e| <= 21 < p
__device__ __forceinline__ uint64_t centred_word(int32_t e, uint64_t p) {
    return e >= 0 ? static_cast<uint64_t>(e) : p - static_cast<uint64_t>(-e);
}

// out [batch][L][N] = randomizeCenteredBinomialDistribution over the stream of every seed
template <typename W>
__global__ void __launch_bounds__(kSamplerThreads)
    sample_binomial_kernel(const uint32_t* __restrict__ chain, W* __restrict__ out, size_t poly_stride, const DeviceContext ctx,
                           uint32_t chunks, size_t total_chunks) {
    __shared__ uint32_t table[256 * kTableCopies];
    fill_table<kTableCopies, kSamplerThreads>(table);
    const uint32_t lane = threadIdx.x & 63;
    const TableView<kTableCopies> te0{table + (lane & (kTableCopies - 1))};
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t item = static_cast<size_t>(blockIdx.x) * kWaves + wave;  // (an exact grid: sampler_grid)
    if (item < total_chunks) {
        const size_t seed_index = item / chunks;
        const uint32_t chunk = static_cast<uint32_t>(item - seed_index * chunks);
        int32_t e[4];
        draw_binomial(te0, chain + item * kRecordWords, lane, e);
        W* poly = out + seed_index * poly_stride;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t k = chunk * kChunkBlocks + 64 * j + lane;
            if (k < ctx.degree)
                for (uint32_t i = 0; i < ctx.moduli_count; ++i)
                    poly[(static_cast<size_t>(i) << ctx.log_degree) + k] = static_cast<W>(centred_word(e[j], ctx.moduli[i].p));
        }
    }
}

// cts [batch][2][m][N] Coeff: polynomial 0 = -(polynomial 0 + e), e drawn here
template <typename W>
__global__ void __launch_bounds__(kSamplerThreads)
    encrypt_finish_coeff_kernel(W* __restrict__ cts, const uint32_t* __restrict__ chain, const DeviceContext ctx, uint32_t chunks,
                                size_t total_chunks) {
    __shared__ uint32_t table[256 * kTableCopies];
    fill_table<kTableCopies, kSamplerThreads>(table);
    const uint32_t lane = threadIdx.x & 63;
    const TableView<kTableCopies> te0{table + (lane & (kTableCopies - 1))};
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t ct_words = (static_cast<size_t>(2) * ctx.moduli_count) << ctx.log_degree;
    const size_t item = static_cast<size_t>(blockIdx.x) * kWaves + wave;  // (an exact grid: sampler_grid)
    if (item < total_chunks) {
        const size_t seed_index = item / chunks;
        const uint32_t chunk = static_cast<uint32_t>(item - seed_index * chunks);
        int32_t e[4];
        draw_binomial(te0, chain + item * kRecordWords, lane, e);
        W* c0 = cts + seed_index * ct_words;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t k = chunk * kChunkBlocks + 64 * j + lane;
            if (k < ctx.degree)
                for (uint32_t i = 0; i < ctx.moduli_count; ++i) {
                    const uint64_t p = ctx.moduli[i].p;
                    W* word = c0 + (static_cast<size_t>(i) << ctx.log_degree) + k;
                    *word = static_cast<W>(neg_mod(add_mod(*word, centred_word(e[j], p), p), p));
                }
        }
    }
}

// out [batch][L][N] = randomizeTernary over the stream of every seed.  Chunk c owns the records that begin in it:
// coefficients [ceil(4096 c / 12), ceil(4096 (c + 1) / 12)), at most 342.
constexpr uint32_t kChunkWords = kChunkBytes / 4;
__device__ __forceinline__ uint32_t first_ternary_coefficient(uint32_t chunk) { return (kChunkWords * chunk + 2) / 3; }
template <typename W>
__global__ void __launch_bounds__(kSamplerThreads)
    sample_ternary_kernel(const uint32_t* __restrict__ chain, W* __restrict__ out, size_t poly_stride, const DeviceContext ctx,
                          uint32_t chunks, size_t total_chunks) {
    __shared__ uint32_t table[256 * kTableCopies];
    __shared__ uint32_t bytes[kWaves][kChunkWords + 4];  // the chunk's stream as little-endian words + the next chunk's first block
    fill_table<kTableCopies, kSamplerThreads>(table);
    const uint32_t lane = threadIdx.x & 63;
    const TableView<kTableCopies> te0{table + (lane & (kTableCopies - 1))};
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t* mine = bytes[wave];
    const size_t item = static_cast<size_t>(blockIdx.x) * kWaves + wave;  // (an exact grid: sampler_grid)
    const bool active = item < total_chunks;  // wave-uniform; an idle wave of the last workgroup still meets the barrier
    const size_t seed_index = active ? item / chunks : 0;
    const uint32_t chunk = active ? static_cast<uint32_t>(item - seed_index * chunks) : 0;
    if (active) {
        ChunkKeys keys;
        load_chunk_keys(chain + item * kRecordWords, keys);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const Block stream = encrypt(te0, keys.rk, counter_add(keys.v, 1 + 64 * j + lane));
#pragma unroll
            for (int c = 0; c < 4; ++c) mine[4 * (64 * j + lane) + c] = __builtin_bswap32(stream.w[c]);
        }
        if (chunk + 1 < chunks) {  // every lane forms the same block: one wave instruction costs what one lane's would
            load_chunk_keys(chain + (item + 1) * kRecordWords, keys);
            const Block stream = encrypt(te0, keys.rk, counter_add(keys.v, 1));
            if (lane < 4)
                mine[kChunkWords + lane] =
                    __builtin_bswap32(lane == 0 ? stream.w[0] : lane == 1 ? stream.w[1] : lane == 2 ? stream.w[2] : stream.w[3]);
        }
    }
    __syncthreads();
    if (active) {
        const uint32_t begin = first_ternary_coefficient(chunk);
        const uint32_t next = first_ternary_coefficient(chunk + 1);
        const uint32_t end = next < ctx.degree ? next : ctx.degree;
        W* poly = out + seed_index * poly_stride;
        for (uint32_t k = begin + lane; k < end; k += 64) {
            // u64 = words 0, 1, u32 = word 2 of the record; (u64 << 32 | u32) mod 3    PolyRq+Randomize.swift:95-99
            const uint32_t* record = mine + (3 * k - kChunkWords * chunk);
            const uint32_t value =
                static_cast<uint32_t>((static_cast<uint64_t>(record[0]) + record[1] + record[2]) % 3u);
            for (uint32_t i = 0; i < ctx.moduli_count; ++i) {
                const uint64_t p = ctx.moduli[i].p;  // val.subtractMod(1, modulus: p)
                poly[(static_cast<size_t>(i) << ctx.log_degree) + k] = static_cast<W>(value == 0 ? p - 1 : value - 1);
            }
        }
    }
}

// ---- element-wise steps: lane i = word k of ciphertext (or key) c, over [count][m][N] ------------------------------------

template <typename W>
__global__ void __launch_bounds__(kThreads)
    encrypt_mul_secret_kernel(W* __restrict__ cts, const W* __restrict__ secret_key, const DeviceContext ctx, size_t poly_words,
                              size_t total) {
    const size_t i = blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x;  // (launch_grid::exact_grid)
    if (i >= total) return;
    const size_t c = i / poly_words, k = i - c * poly_words;
    const DeviceModulus* m = ctx.moduli + (k >> ctx.log_degree);
    W* ct = cts + 2 * c * poly_words + k;
    ct[0] = static_cast<W>(barrett_mul(ct[poly_words], secret_key[k], m->p, m->product_factor, static_cast<int>(m->product_shift)));
}

template <typename W, bool KEY_SWITCH>
__global__ void __launch_bounds__(kThreads)
    encrypt_finish_eval_kernel(W* __restrict__ cts, const W* __restrict__ error_eval, const W* __restrict__ secret_key,
                               const W* __restrict__ current_keys, uint32_t per_key, const KeySwitchFactors factors,
                               const DeviceContext ctx, size_t poly_words, size_t total) {
    const size_t i = blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x;  // (launch_grid::exact_grid)
    if (i >= total) return;
    const size_t c = i / poly_words, k = i - c * poly_words;
    const uint32_t row = static_cast<uint32_t>(k >> ctx.log_degree);
    const DeviceModulus* m = ctx.moduli + row;
    const uint64_t p = m->p;
    W* ct = cts + 2 * c * poly_words + k;
    const uint64_t product = barrett_mul(ct[poly_words], secret_key[k], p, m->product_factor, static_cast<int>(m->product_shift));
    uint64_t c0 = neg_mod(add_mod(product, error_eval[i], p), p);
    if constexpr (KEY_SWITCH) {
        const size_t key = c / per_key;
        if (row == static_cast<uint32_t>(c - key * per_key)) {
            const U64x2 factor = factors.factor[row];
            c0 = add_mod(c0, shoup_mul(current_keys[key * poly_words + k], factor.x, factor.y, p), p);
        }
    }
    ct[0] = static_cast<W>(c0);
}

template <typename W>
__global__ void __launch_bounds__(kThreads)
    secret_key_square_kernel(const W* __restrict__ secret_key, W* __restrict__ out, const DeviceContext ctx, size_t total) {
    const size_t k = blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x;  // (launch_grid::exact_grid)
    if (k >= total) return;
    const DeviceModulus* m = ctx.moduli + (k >> ctx.log_degree);
    const uint64_t s = secret_key[k];
    out[k] = static_cast<W>(barrett_mul(s, s, m->p, m->product_factor, static_cast<int>(m->product_shift)));
}

// The rotated secret keys of `count` Galois elements in one launch: out [count][m][N], key e = f(x) -> f(x^elements[e]) of
// the Eval rows of secret_key (galois_index.hpp).  The elements travel in the kernel arguments.
template <typename W>
__global__ void __launch_bounds__(kThreads)
    secret_key_galois_kernel(const W* __restrict__ secret_key, W* __restrict__ out, uint32_t logn, size_t key_words,
                             const GaloisElementTable elements, size_t total) {
    const size_t idx = blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x;  // (launch_grid::exact_grid)
    if (idx >= total) return;
    const size_t key = idx / key_words, k = idx - key * key_words;
    const size_t row = k >> logn;
    const uint32_t i = static_cast<uint32_t>(k) & ((1u << logn) - 1);
    out[idx] = secret_key[(row << logn) + galois_eval_source(i, logn, elements.element[key])];
}

bool exact_grid_fits(size_t total, dim3& grid) {
    if (!launch_grid::launch_fits(launch_grid::grid_blocks(total, kThreads, SIZE_MAX), kThreads)) return false;
    grid = dim3(launch_grid::exact_grid(total, kThreads));
    return true;
}
// one wavefront per (seed, chunk), kWaves of them to a workgroup; false when HIP cannot launch that many
bool sampler_grid(size_t total_chunks, dim3& grid) {
    const size_t blocks = launch_grid::grid_blocks(total_chunks, kWaves, SIZE_MAX);
    if (!launch_grid::launch_fits(blocks, kSamplerThreads)) return false;
    grid = dim3(static_cast<unsigned>(blocks));
    return true;
}

}  // namespace

template <typename W>
hipError_t launch_sample_ternary(const uint32_t* chain, W* out, size_t poly_stride, const DeviceContext& ctx, size_t batch,
                                 hipStream_t stream) {
    if (batch == 0) return hipSuccess;
    const uint32_t chunks = ternary_chunks(ctx.degree);
    const size_t total_chunks = batch * chunks;
    dim3 grid;
    if (!sampler_grid(total_chunks, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_ternary_kernel<W>, grid, dim3(kSamplerThreads), 0, stream, chain, out, poly_stride, ctx, chunks,
                       total_chunks);
    return hipGetLastError();
}

template <typename W>
hipError_t launch_sample_centered_binomial(const uint32_t* chain, W* out, size_t poly_stride, const DeviceContext& ctx,
                                           size_t batch, hipStream_t stream) {
    if (batch == 0) return hipSuccess;
    const uint32_t chunks = binomial_chunks(ctx.degree);
    const size_t total_chunks = batch * chunks;
    dim3 grid;
    if (!sampler_grid(total_chunks, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_binomial_kernel<W>, grid, dim3(kSamplerThreads), 0, stream, chain, out, poly_stride, ctx, chunks,
                       total_chunks);
    return hipGetLastError();
}

template <typename W>
hipError_t launch_encrypt_mul_secret(W* cts, const W* secret_key, const DeviceContext& ctx, size_t batch, hipStream_t stream) {
    if (batch == 0) return hipSuccess;
    const size_t poly_words = static_cast<size_t>(ctx.moduli_count) << ctx.log_degree;
    dim3 grid;
    if (!exact_grid_fits(batch * poly_words, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(encrypt_mul_secret_kernel<W>, grid, dim3(kThreads), 0, stream, cts, secret_key, ctx, poly_words,
                       batch * poly_words);
    return hipGetLastError();
}

template <typename W>
hipError_t launch_encrypt_finish_coeff(W* cts, const uint32_t* error_chain, const DeviceContext& ctx, size_t batch,
                                       hipStream_t stream) {
    if (batch == 0) return hipSuccess;
    const uint32_t chunks = binomial_chunks(ctx.degree);
    const size_t total_chunks = batch * chunks;
    dim3 grid;
    if (!sampler_grid(total_chunks, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(encrypt_finish_coeff_kernel<W>, grid, dim3(kSamplerThreads), 0, stream, cts, error_chain, ctx, chunks,
                       total_chunks);
    return hipGetLastError();
}

template <typename W>
hipError_t launch_encrypt_finish_eval(W* cts, const W* error_eval, const W* secret_key, const W* current_keys,
                                      uint32_t per_key, const KeySwitchFactors& factors, const DeviceContext& ctx, size_t count,
                                      hipStream_t stream) {
    if (count == 0) return hipSuccess;
    if (current_keys != nullptr && (per_key == 0 || per_key > kMaxKeySwitchCiphertexts)) return hipErrorInvalidValue;
    const size_t poly_words = static_cast<size_t>(ctx.moduli_count) << ctx.log_degree;
    dim3 grid;
    if (!exact_grid_fits(count * poly_words, grid)) return hipErrorInvalidValue;
    if (current_keys != nullptr)
        hipLaunchKernelGGL((encrypt_finish_eval_kernel<W, true>), grid, dim3(kThreads), 0, stream, cts, error_eval, secret_key,
                           current_keys, per_key, factors, ctx, poly_words, count * poly_words);
    else
        hipLaunchKernelGGL((encrypt_finish_eval_kernel<W, false>), grid, dim3(kThreads), 0, stream, cts, error_eval, secret_key,
                           current_keys, per_key, factors, ctx, poly_words, count * poly_words);
    return hipGetLastError();
}

template <typename W>
hipError_t launch_secret_key_square(const W* secret_key, W* out, const DeviceContext& ctx, hipStream_t stream) {
    const size_t total = static_cast<size_t>(ctx.moduli_count) << ctx.log_degree;
    dim3 grid;
    if (!exact_grid_fits(total, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(secret_key_square_kernel<W>, grid, dim3(kThreads), 0, stream, secret_key, out, ctx, total);
    return hipGetLastError();
}

template <typename W>
hipError_t launch_secret_key_galois(const W* secret_key, W* out, const DeviceContext& ctx, const uint64_t* elements, size_t count,
                                    hipStream_t stream) {
    const size_t key_words = static_cast<size_t>(ctx.moduli_count) << ctx.log_degree;
    for (size_t first = 0; first < count; first += kGaloisElementsPerLaunch) {
        const size_t now = count - first < kGaloisElementsPerLaunch ? count - first : kGaloisElementsPerLaunch;
        GaloisElementTable table{};
        for (size_t e = 0; e < now; ++e) table.element[e] = static_cast<uint32_t>(elements[first + e]);
        dim3 grid;
        if (!exact_grid_fits(now * key_words, grid)) return hipErrorInvalidValue;
        hipLaunchKernelGGL(secret_key_galois_kernel<W>, grid, dim3(kThreads), 0, stream, secret_key, out + first * key_words,
                           ctx.log_degree, key_words, table, now * key_words);
        const hipError_t status = hipGetLastError();
        if (status != hipSuccess) return status;
    }
    return hipSuccess;
}

#define HEAMD_ENCRYPT_INSTANCES(W)                                                                                            \
    template hipError_t launch_sample_ternary<W>(const uint32_t*, W*, size_t, const DeviceContext&, size_t, hipStream_t);     \
    template hipError_t launch_sample_centered_binomial<W>(const uint32_t*, W*, size_t, const DeviceContext&, size_t,         \
                                                           hipStream_t);                                                      \
    template hipError_t launch_encrypt_mul_secret<W>(W*, const W*, const DeviceContext&, size_t, hipStream_t);                \
    template hipError_t launch_encrypt_finish_coeff<W>(W*, const uint32_t*, const DeviceContext&, size_t, hipStream_t);       \
    template hipError_t launch_encrypt_finish_eval<W>(W*, const W*, const W*, const W*, uint32_t, const KeySwitchFactors&,    \
                                                      const DeviceContext&, size_t, hipStream_t);                             \
    template hipError_t launch_secret_key_square<W>(const W*, W*, const DeviceContext&, hipStream_t);                         \
    template hipError_t launch_secret_key_galois<W>(const W*, W*, const DeviceContext&, const uint64_t*, size_t, hipStream_t);
HEAMD_ENCRYPT_INSTANCES(uint64_t)
HEAMD_ENCRYPT_INSTANCES(uint32_t)
#undef HEAMD_ENCRYPT_INSTANCES

}  // namespace heamd
