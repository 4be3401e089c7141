// keyword_pir_kernels.hip -- the data-parallel parts of KeywordPirServer.process (reference Sources/PrivateInformationRetrieval/
// KeywordPir/KeywordPirProtocol.swift:191-247): HashKeyword.hash and .hashIndices (HashBucket.swift:221-269),
// ShardingFunction.shardIndex (KeywordDatabase.swift:56-62,103-111) and HashBucket.serialize (HashBucket.swift:90-103,177-187).
//
// SHA-256 (FIPS 180-4) runs one message per lane.  The message schedule is a rolling window of 16 words and the 64 rounds are
// unrolled, so every index into the window and into the round constants is a constant and the window stays in registers
// (tests/test_keyword_pir_scratch.py holds the object to that).
#include <hip/hip_runtime.h>

#include "keyword_pir.hpp"
#include "launch_grid.hpp"

namespace heamd {
namespace {

__device__ __forceinline__ uint32_t rotr(uint32_t x, uint32_t n) { return (x >> n) | (x << (32 - n)); }

constexpr uint32_t kInitialState[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                                       0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
constexpr uint32_t kRound[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
    0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
    0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
    0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
    0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
    0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

// One block: `w` is the 16 message words on entry and the rolling window of the schedule afterwards.
__device__ __forceinline__ void sha256_block(uint32_t (&state)[8], uint32_t (&w)[16]) {
    uint32_t a = state[0], b = state[1], c = state[2], d = state[3], e = state[4], f = state[5], g = state[6], h = state[7];
#pragma unroll
    for (int t = 0; t < 64; ++t) {
        if (t >= 16) {
            const uint32_t w15 = w[(t - 15) & 15], w2 = w[(t - 2) & 15];
            w[t & 15] += (rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3)) + w[(t - 7) & 15] +
                         (rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10));
        }
        const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + kRound[t] + w[t & 15];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
    }
    state[0] += a, state[1] += b, state[2] += c, state[3] += d, state[4] += e, state[5] += f, state[6] += g, state[7] += h;
}

// the first 8 digest bytes read as a little-endian UInt64 (`buffer.load(as: UInt64.self)`): the digest is big-endian words
__device__ __forceinline__ uint64_t truncated_digest(const uint32_t (&state)[8]) {
    return uint64_t(__builtin_bswap32(state[0])) | (uint64_t(__builtin_bswap32(state[1])) << 32);
}

// Word `at / 4` of the padded message (at: a multiple of 4): message bytes, then 0x80, then zeros; the bit count in the last
// 8 bytes is the caller's.  Only bytes [message, message + length) are read.
__device__ __forceinline__ uint32_t padded_word(const uint8_t* message, uint64_t length, uint64_t at) {
    if (at + 4 <= length) {
        uint32_t word;
        __builtin_memcpy(&word, message + at, 4);  // any address
        return __builtin_bswap32(word);
    }
    uint32_t word = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint64_t p = at + k;
        const uint32_t byte = p < length ? message[p] : (p == length ? 0x80u : 0u);
        word |= byte << (24 - 8 * k);
    }
    return word;
}

__global__ void __launch_bounds__(256)
    keyword_hash_kernel(const uint8_t* __restrict__ blob, const uint64_t* __restrict__ offsets, size_t count,
                        uint64_t* __restrict__ hashes) {
    const size_t idx = blockIdx.x * size_t(256) + threadIdx.x;  // one keyword per lane (launch_grid::exact_grid)
    if (idx >= count) return;
    const uint64_t begin = offsets[idx], length = offsets[idx + 1] - begin;
    const uint8_t* message = blob + begin;
    const uint64_t blocks = (length + 9 + 63) / 64;  // 0x80 and the 8-byte bit count behind the message
    uint32_t state[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) state[i] = kInitialState[i];
    for (uint64_t block = 0; block < blocks; ++block) {
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = padded_word(message, length, block * 64 + 4 * i);
        if (block + 1 == blocks) {
            w[14] = static_cast<uint32_t>(length >> 29);
            w[15] = static_cast<uint32_t>(length << 3);
        }
        sha256_block(state, w);
    }
    hashes[idx] = truncated_digest(state);
}

// HashKeyword.indexFromHash (HashBucket.swift:244-257): SHA-256 of the hash's 8 big-endian bytes and the counter byte
__device__ __forceinline__ uint64_t index_from_hash(uint64_t hash, uint64_t bucket_count, uint32_t counter) {
    uint32_t state[8], w[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) state[i] = kInitialState[i];
#pragma unroll
    for (int i = 3; i < 15; ++i) w[i] = 0;
    w[0] = static_cast<uint32_t>(hash >> 32);
    w[1] = static_cast<uint32_t>(hash);
    w[2] = (counter << 24) | 0x00800000u;
    w[15] = 72;  // 9 bytes
    sha256_block(state, w);
    return truncated_digest(state) % bucket_count;
}

constexpr uint32_t kMaxRetries = 10;  // HashKeyword.maxRetries (HashBucket.swift:212)

// One loop with one hash in it: (i, counter) is the candidate being derived and its retry.  The candidates stay in registers:
// every index into the array is a constant of an unrolled loop, the running position a predicate.
__global__ void __launch_bounds__(256)
    keyword_hash_indices_kernel(const uint64_t* __restrict__ hashes, size_t count, uint64_t bucket_count, uint32_t h,
                                uint32_t* __restrict__ indices) {
    const size_t idx = blockIdx.x * size_t(256) + threadIdx.x;  // one keyword per lane (launch_grid::exact_grid)
    if (idx >= count) return;
    const uint64_t hash = hashes[idx];
    uint32_t candidates[kKeywordPirMaxHashFunctions];
#pragma unroll
    for (uint32_t j = 0; j < kKeywordPirMaxHashFunctions; ++j) candidates[j] = 0;
    uint32_t i = 0, counter = 0;
    while (i < h) {
        const uint32_t index = static_cast<uint32_t>(index_from_hash(hash, bucket_count, counter));
        bool seen = false;
#pragma unroll
        for (uint32_t j = 0; j < kKeywordPirMaxHashFunctions; ++j) seen |= j < i && candidates[j] == index;
        if (seen && counter < kMaxRetries) {  // after the tenth retry a repeated index is kept (:227-231)
            ++counter;
            continue;
        }
#pragma unroll
        for (uint32_t j = 0; j < kKeywordPirMaxHashFunctions; ++j)
            if (j == i) candidates[j] = index;
        indices[idx * h + i] = index;
        ++i;
        counter = 0;
    }
}

__global__ void __launch_bounds__(256)
    keyword_shard_index_kernel(const uint64_t* __restrict__ hashes, size_t count, uint64_t shard_count,
                               uint64_t other_shard_count, uint32_t* __restrict__ out) {
    const size_t idx = blockIdx.x * size_t(256) + threadIdx.x;  // one keyword per lane (launch_grid::exact_grid)
    if (idx >= count) return;
    uint64_t shard = hashes[idx];
    if (other_shard_count != 0) shard %= other_shard_count;  // doubleMod (KeywordDatabase.swift:107-109)
    out[idx] = static_cast<uint32_t>(shard % shard_count);
}

__global__ void __launch_bounds__(256)
    hash_bucket_slot_starts_kernel(const HashBucketTable table, uint32_t* __restrict__ slot_starts,
                                   uint32_t* __restrict__ mismatch) {
    const size_t bucket = blockIdx.x * size_t(256) + threadIdx.x;  // one bucket per lane (launch_grid::exact_grid)
    if (bucket >= table.bucket_count) return;
    const uint32_t first = table.bucket_offsets[bucket], last = table.bucket_offsets[bucket + 1];
    uint64_t start = 1;  // the slot count byte
    for (uint32_t slot = first; slot < last; ++slot) {
        const uint32_t entry = table.slot_entries[slot];
        slot_starts[slot] = static_cast<uint32_t>(start < 0xffffffffu ? start : 0xffffffffu);
        start += 10 + (table.value_offsets[entry + 1] - table.value_offsets[entry]);  // hash, UInt16 size, value
    }
    if (mismatch != nullptr) {
        const uint32_t flags = (start > table.entry_size ? 1u : 0u) | (last - first > 255 ? 2u : 0u);
        if (flags != 0) atomicOr(mismatch, flags);
    }
}

// The slot a lane is reading from: its record is bytes [start, end) of the bucket's row (for the last slot, `end` is the end
// of the row: the padding behind the record reads as zero).
struct SlotCursor {
    bool valid = false;
    uint64_t start = 0, end = 0, value_begin = 0, value_size = 0, hash = 0;
};

// byte `r` of bucket `bucket`'s row: the slot count, the records, zeros
__device__ __forceinline__ uint32_t bucket_byte(const HashBucketTable& table, const uint32_t* __restrict__ slot_starts,
                                                uint64_t bucket, uint64_t r, SlotCursor& cursor) {
    const uint32_t first = table.bucket_offsets[bucket], last = table.bucket_offsets[bucket + 1];
    if (r == 0) return (last - first) & 0xffu;
    if (first == last) return 0;
    if (!cursor.valid || r < cursor.start || r >= cursor.end) {
        uint32_t lo = first, hi = last;  // the last slot whose record starts at or before r (slot_starts[first] = 1 <= r)
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (slot_starts[mid] <= r) lo = mid; else hi = mid;
        }
        const uint32_t entry = table.slot_entries[lo];
        cursor.valid = true;
        cursor.start = slot_starts[lo];
        cursor.value_begin = table.value_offsets[entry];
        cursor.value_size = table.value_offsets[entry + 1] - cursor.value_begin;
        cursor.end = lo + 1 == last ? table.entry_size : cursor.start + 10 + cursor.value_size;
        cursor.hash = table.hashes[entry];
    }
    const uint64_t rel = r - cursor.start;
    if (rel < 8) return static_cast<uint32_t>(cursor.hash >> (8 * rel)) & 0xffu;
    if (rel < 10) return static_cast<uint32_t>(cursor.value_size >> (8 * (rel - 8))) & 0xffu;
    if (rel < 10 + cursor.value_size) return table.values[cursor.value_begin + (rel - 10)];
    return 0;
}

// A lane owns one aligned 8-byte chunk of the output: it gathers the chunk's bytes and issues one 8-byte store, byte stores only
// where the chunk crosses the first or last byte of [out, out + total).
__global__ void __launch_bounds__(256)
    hash_bucket_serialize_kernel(const HashBucketTable table, const uint32_t* __restrict__ slot_starts,
                                 uint8_t* __restrict__ out, uint64_t total, uint64_t first_chunk, uint64_t chunks) {
    const uint64_t head = reinterpret_cast<uintptr_t>(out) & 7;  // chunk c holds output bytes [8 c - head, 8 c - head + 8)
    const uint64_t entry_size = table.entry_size;
    const uint64_t chunk = first_chunk + blockIdx.x * uint64_t(256) + threadIdx.x;  // (launch_grid::exact_grid)
    if (chunk < chunks) {
        const uint32_t lo = chunk == 0 ? static_cast<uint32_t>(head) : 0;
        const uint64_t position = 8 * chunk + lo - head;  // the first output byte of the chunk
        const uint64_t left = total - position;
        const uint32_t hi = left < 8 - lo ? lo + static_cast<uint32_t>(left) : 8;
        uint64_t bucket = position / entry_size, r = position - bucket * entry_size;
        SlotCursor cursor;
        const bool whole = lo == 0 && hi == 8;
        uint64_t word = 0;
        bool gathered = false;
        if (whole && r != 0 && r + 8 <= entry_size) {
            (void)bucket_byte(table, slot_starts, bucket, r, cursor);
            if (cursor.valid) {
                const uint64_t value_start = cursor.start + 10, value_end = value_start + cursor.value_size;
                if (r >= value_start && r + 8 <= value_end) {  // inside one value: eight bytes from any address
                    __builtin_memcpy(&word, table.values + cursor.value_begin + (r - value_start), 8);
                    gathered = true;
                } else if (r >= value_end && r + 8 <= cursor.end) {  // inside the padding
                    gathered = true;
                }
            } else {
                gathered = true;  // an empty bucket: zeros behind its count byte
            }
        }
        if (!gathered) {
            for (uint32_t k = lo; k < hi; ++k) {
                word |= uint64_t(bucket_byte(table, slot_starts, bucket, r, cursor)) << (8 * k);
                if (++r == entry_size) r = 0, ++bucket, cursor.valid = false;
            }
        }
        // 8-byte aligned; its bytes [lo, hi) lie in the output
        uint8_t* at = reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(out) & ~uintptr_t(7)) + 8 * chunk);
        if (whole) {
            *reinterpret_cast<uint64_t*>(at) = word;
        } else {
            for (uint32_t k = lo; k < hi; ++k) at[k] = static_cast<uint8_t>(word >> (8 * k));
        }
    }
}

}  // namespace

hipError_t launch_keyword_hash(const uint8_t* blob, const uint64_t* offsets, size_t count, uint64_t* hashes, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(keyword_hash_kernel, dim3(launch_grid::exact_grid(count, 256)), dim3(256), 0, stream, blob, offsets, count,
                       hashes);
    return hipGetLastError();
}

hipError_t launch_keyword_hash_indices(const uint64_t* hashes, size_t count, uint64_t bucket_count, uint32_t h,
                                       uint32_t* indices, hipStream_t stream) {
    if (h == 0 || h > kKeywordPirMaxHashFunctions) return hipErrorInvalidValue;
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(keyword_hash_indices_kernel, dim3(launch_grid::exact_grid(count, 256)), dim3(256), 0, stream, hashes,
                       count, bucket_count, h, indices);
    return hipGetLastError();
}

hipError_t launch_keyword_shard_indices(const uint64_t* hashes, size_t count, uint64_t shard_count, uint64_t other_shard_count,
                                        uint32_t* out, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(keyword_shard_index_kernel, dim3(launch_grid::exact_grid(count, 256)), dim3(256), 0, stream, hashes, count,
                       shard_count, other_shard_count, out);
    return hipGetLastError();
}

hipError_t launch_hash_bucket_slot_starts(const HashBucketTable& table, uint32_t* slot_starts, uint32_t* mismatch,
                                          hipStream_t stream) {
    if (table.bucket_count == 0) return hipSuccess;
    hipLaunchKernelGGL(hash_bucket_slot_starts_kernel, dim3(launch_grid::exact_grid(table.bucket_count, 256)), dim3(256), 0,
                       stream, table, slot_starts, mismatch);
    return hipGetLastError();
}

hipError_t launch_hash_bucket_serialize(const HashBucketTable& table, const uint32_t* slot_starts, uint8_t* out,
                                        hipStream_t stream) {
    const uint64_t total = table.bucket_count * table.entry_size;
    if (total == 0) return hipSuccess;
    const uint64_t head = reinterpret_cast<uintptr_t>(out) & 7;
    const uint64_t chunks = (head + total + 7) / 8;
    const uint64_t most = launch_grid::max_blocks(256) * 256;  // chunks of one launch: 32 GiB of rows
    for (uint64_t first = 0; first < chunks; first += most) {
        const uint64_t now = chunks - first < most ? chunks - first : most;
        hipLaunchKernelGGL(hash_bucket_serialize_kernel, dim3(launch_grid::exact_grid(now, 256)), dim3(256), 0, stream, table,
                           slot_starts, out, total, first, chunks);
        const hipError_t status = hipGetLastError();
        if (status != hipSuccess) return status;
    }
    return hipSuccess;
}

}  // namespace heamd
