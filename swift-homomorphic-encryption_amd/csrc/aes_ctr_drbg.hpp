// aes_ctr_drbg.hpp -- the device side of NistAes128Ctr (Random/NistAes128Ctr.swift, Random/BufferedRng.swift,
// Random/NistCtrDrbg.swift:23-96) shared by the translation units that turn its byte stream into polynomials:
// seeded_kernels.hip (the uniform polynomial `a`) and encrypt_kernels.hip (the ternary and centred binomial samplers).
// AES (FIPS-197) uses one T-table (the other three are byte rotations of it), held in LDS `COPIES` times interleaved so
// that lane l reads copy l mod COPIES: the data-dependent lookups of a wavefront then spread over the banks instead of
// colliding on the 256 words of a single copy.
// The stream of a seed is a chain of 4096-byte generate() calls, each followed by a re-key; launch_seeded_chain
// (seeded_kernels.hip) walks that chain and records, per chunk, the round keys and the counter: kRecordWords words.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace heamd {

// chain [batch][chunks][kRecordWords]: record (b, c) holds the 44 round-key words and the 4 counter words under which
// bytes [4096 c, 4096 c + 4096) of seed b's stream are AES-CTR blocks 1..256.  Asynchronous on `stream`.
hipError_t launch_seeded_chain(const uint8_t* seeds, uint32_t* chain, size_t batch, uint32_t chunks, hipStream_t stream);

namespace aes {

// Te0[x] = (2 S[x], S[x], S[x], 3 S[x]) as a big-endian word, FIPS-197 5.1.1 / 5.1.3: built at compile time, so the
// library has no table upload (nothing to synchronise inside a stream capture) and no mutable device state.
struct AesTable {
    uint32_t te0[256];
};
constexpr uint32_t gf256_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    while (b) {
        if (b & 1) r ^= a;
        a = ((a << 1) ^ ((a & 0x80) ? 0x1b : 0)) & 0xff;
        b >>= 1;
    }
    return r;
}
constexpr AesTable make_aes_table() {
    AesTable t{};
    for (uint32_t x = 0; x < 256; ++x) {
        // the inverse in GF(2^8) is x^254 (0 -> 0)
        uint32_t inverse = 1, power = x;
        for (int bit = 1; bit < 8; ++bit) {
            power = gf256_mul(power, power);  // x^(2^bit)
            inverse = gf256_mul(inverse, power);
        }
        uint32_t s = inverse;
        for (int k = 1; k <= 4; ++k) s ^= ((inverse << k) | (inverse >> (8 - k))) & 0xff;
        s ^= 0x63;
        t.te0[x] = (gf256_mul(s, 2) << 24) | (s << 16) | (s << 8) | gf256_mul(s, 3);
    }
    return t;
}
__device__ constexpr AesTable g_aes_table = make_aes_table();
static_assert(g_aes_table.te0[0] == 0xc66363a5u && g_aes_table.te0[1] == 0xf87c7c84u, "FIPS-197 S-box: S[0] = 0x63, S[1] = 0x7c");

__device__ __forceinline__ uint32_t rotr32(uint32_t x, int k) { return (x >> k) | (x << (32 - k)); }
// a lane's view of the interleaved LDS table: entry x of its copy
template <int COPIES>
struct TableView {
    const uint32_t* base;  // &table[lane % COPIES]
    __device__ __forceinline__ uint32_t operator[](uint32_t x) const { return base[x * COPIES]; }
};

template <typename Table>
__device__ __forceinline__ uint32_t sbox(const Table& te0, uint32_t x) { return (te0[x] >> 8) & 0xffu; }
template <typename Table>
__device__ __forceinline__ uint32_t sub_word(const Table& te0, uint32_t w) {
    return (sbox(te0, w >> 24) << 24) | (sbox(te0, (w >> 16) & 0xff) << 16) | (sbox(te0, (w >> 8) & 0xff) << 8) |
           sbox(te0, w & 0xff);
}

struct Block {
    uint32_t w[4];  // big-endian column words
};

template <typename Table>
__device__ __forceinline__ void expand_key(const Table& te0, const Block& key, uint32_t (&rk)[44]) {
    // FIPS-197 5.2
#pragma unroll
    for (int i = 0; i < 4; ++i) rk[i] = key.w[i];
    uint32_t rcon = 0x01000000u;
#pragma unroll
    for (int i = 4; i < 44; ++i) {
        uint32_t t = rk[i - 1];
        if (i % 4 == 0) {
            t = sub_word(te0, (t << 8) | (t >> 24)) ^ rcon;
            rcon = (rcon << 1) ^ ((rcon & 0x80000000u) ? 0x1b000000u : 0u);
        }
        rk[i] = rk[i - 4] ^ t;
    }
}

template <typename Table, typename RoundKeys>
__device__ __forceinline__ Block encrypt(const Table& te0, const RoundKeys& rk, Block in) {
    uint32_t s0 = in.w[0] ^ rk[0], s1 = in.w[1] ^ rk[1], s2 = in.w[2] ^ rk[2], s3 = in.w[3] ^ rk[3];
#pragma unroll
    for (int r = 1; r < 10; ++r) {
        const uint32_t t0 = te0[s0 >> 24] ^ rotr32(te0[(s1 >> 16) & 0xff], 8) ^ rotr32(te0[(s2 >> 8) & 0xff], 16) ^
                            rotr32(te0[s3 & 0xff], 24) ^ rk[4 * r];
        const uint32_t t1 = te0[s1 >> 24] ^ rotr32(te0[(s2 >> 16) & 0xff], 8) ^ rotr32(te0[(s3 >> 8) & 0xff], 16) ^
                            rotr32(te0[s0 & 0xff], 24) ^ rk[4 * r + 1];
        const uint32_t t2 = te0[s2 >> 24] ^ rotr32(te0[(s3 >> 16) & 0xff], 8) ^ rotr32(te0[(s0 >> 8) & 0xff], 16) ^
                            rotr32(te0[s1 & 0xff], 24) ^ rk[4 * r + 2];
        const uint32_t t3 = te0[s3 >> 24] ^ rotr32(te0[(s0 >> 16) & 0xff], 8) ^ rotr32(te0[(s1 >> 8) & 0xff], 16) ^
                            rotr32(te0[s2 & 0xff], 24) ^ rk[4 * r + 3];
        s0 = t0, s1 = t1, s2 = t2, s3 = t3;
    }
    Block out;
    out.w[0] = ((sbox(te0, s0 >> 24) << 24) | (sbox(te0, (s1 >> 16) & 0xff) << 16) | (sbox(te0, (s2 >> 8) & 0xff) << 8) |
                sbox(te0, s3 & 0xff)) ^ rk[40];
    out.w[1] = ((sbox(te0, s1 >> 24) << 24) | (sbox(te0, (s2 >> 16) & 0xff) << 16) | (sbox(te0, (s3 >> 8) & 0xff) << 8) |
                sbox(te0, s0 & 0xff)) ^ rk[41];
    out.w[2] = ((sbox(te0, s2 >> 24) << 24) | (sbox(te0, (s3 >> 16) & 0xff) << 16) | (sbox(te0, (s0 >> 8) & 0xff) << 8) |
                sbox(te0, s1 & 0xff)) ^ rk[42];
    out.w[3] = ((sbox(te0, s3 >> 24) << 24) | (sbox(te0, (s0 >> 16) & 0xff) << 16) | (sbox(te0, (s1 >> 8) & 0xff) << 8) |
                sbox(te0, s2 & 0xff)) ^ rk[43];
    return out;
}

// 128-bit big-endian counter + small amount
__device__ __forceinline__ Block counter_add(Block v, uint32_t amount) {
    uint64_t sum = static_cast<uint64_t>(v.w[3]) + amount;
    v.w[3] = static_cast<uint32_t>(sum);
    sum = static_cast<uint64_t>(v.w[2]) + (sum >> 32);
    v.w[2] = static_cast<uint32_t>(sum);
    sum = static_cast<uint64_t>(v.w[1]) + (sum >> 32);
    v.w[1] = static_cast<uint32_t>(sum);
    v.w[0] += static_cast<uint32_t>(sum >> 32);
    return v;
}

__device__ __forceinline__ uint32_t load_be32(const uint8_t* p) {
    return (static_cast<uint32_t>(p[0]) << 24) | (static_cast<uint32_t>(p[1]) << 16) | (static_cast<uint32_t>(p[2]) << 8) |
           p[3];
}

constexpr uint32_t kChunkBlocks = 256;  // BufferedRng's 4096-byte refill = 256 counter blocks
constexpr uint32_t kChunkBytes = 16 * kChunkBlocks;
constexpr uint32_t kRecordWords = 48;   // per chunk: 44 round-key words + the 4 counter words

template <int COPIES, int THREADS>
__device__ __forceinline__ void fill_table(uint32_t* table) {
    for (uint32_t i = threadIdx.x; i < 256u * COPIES; i += THREADS) table[i] = g_aes_table.te0[i / COPIES];
    __syncthreads();
}

constexpr int kTableCopies = 16;  // interleaved copies of the AES T-table in LDS (profiles/r02n_wire_format_table_copies.txt)

}  // namespace aes
}  // namespace heamd
