// keyword_pir_client_kernels.hip -- KeywordPirClient.decrypt(response:at:using:) behind the index-PIR client (reference Sources/
// PrivateInformationRetrieval/KeywordPir/KeywordPirProtocol.swift:343-359): HashBucket.init(deserialize:) and find(hash:)
// (HashBucket.swift:51-73,118-133,200-205) over the h bucket rows of a query, and countEntriesInResponse (:376-391).
//
// A bucket is a chain: the slot count byte, then per slot 8 bytes of hash, a UInt16 size and `size` bytes of value, so slot k + 1
// is found only by reading slot k.  The search is two launches.  The walk takes one (query, bucket) row and leaves a 16-byte
// record -- corrupt, or where a matching value lies -- in scratch: the staged form copies the row into LDS with 16-byte loads
// (the up to 15 bytes in front of the first and behind the last whole line one byte a lane) and one lane walks it there, the
// direct form walks global memory with one lane a row.  The resolve launch takes each query's records in bucket order and writes
// the value and the zeros behind it, its lanes spread over the 16-byte lines of out_values.  No atomics.
#include "keyword_pir_client_kernels.hpp"

#include "launch_grid.hpp"

namespace heamd {

namespace {

using keyword_pir_client::kSlotHeaderBytes;
using keyword_pir_client::kStatusCorrupt;
using keyword_pir_client::kStatusFound;
using keyword_pir_client::kStatusNil;

constexpr unsigned kClientThreads = 256;

__global__ __launch_bounds__(kClientThreads) void keyword_client_widen_kernel(const uint32_t* __restrict__ in,
                                                                              unsigned long long* __restrict__ out, uint64_t count) {
    const uint64_t index = static_cast<uint64_t>(blockIdx.x) * kClientThreads + threadIdx.x;  // (launch_grid::exact_grid)
    if (index < count) out[index] = in[index];
}

// HashBucket.init(deserialize:) of b[0, length), length >= 1, and with kSearch find(hash:) on the way: the first slot whose hash
// is `hash`.  A bucket that does not deserialize is corrupt whatever its earlier slots hold.  Only b[0, length) is read.
struct BucketWalk {
    uint32_t status = kStatusNil, slots = 0;
    uint64_t value_offset = 0, value_size = 0;
    uint64_t end = 0;  // serializedSize(): where the bytes behind the last slot begin
};
template <bool kSearch>
__device__ __forceinline__ BucketWalk walk_bucket(const uint8_t* b, uint64_t length, uint64_t hash) {
    BucketWalk walk;
    walk.slots = b[0];
    uint64_t offset = 1;
    for (uint32_t slot = 0; slot < walk.slots; ++slot) {
        if (length < offset + kSlotHeaderBytes) {
            walk.status = kStatusCorrupt;
            return walk;
        }
        uint64_t slot_hash;
        uint16_t size;
        __builtin_memcpy(&slot_hash, b + offset, 8);  // any address; the device is little-endian, as the format
        __builtin_memcpy(&size, b + offset + 8, 2);
        offset += kSlotHeaderBytes;
        if (offset + size > length) {
            walk.status = kStatusCorrupt;
            return walk;
        }
        if (kSearch && walk.status == kStatusNil && slot_hash == hash) {
            walk.status = kStatusFound;
            walk.value_offset = offset;
            walk.value_size = size;
        }
        offset += size;
    }
    walk.end = offset;
    return walk;
}

__device__ __forceinline__ uint4 record_of(const BucketWalk& walk) {
    const bool found = walk.status == kStatusFound;
    return make_uint4(walk.status, found ? static_cast<uint32_t>(walk.value_size) : 0u,
                      found ? static_cast<uint32_t>(walk.value_offset) : 0u,
                      found ? static_cast<uint32_t>(walk.value_offset >> 32) : 0u);
}

// One workgroup per (query, bucket).  Row byte r is staged at line[head + r], head the row's offset inside its 16-byte line of
// global memory: a whole line of the row is one 16-byte load and one 16-byte LDS store, both aligned.
template <uint32_t kLdsBytes, uint32_t kThreads>
__global__ __launch_bounds__(kThreads) void keyword_find_staged_kernel(const uint8_t* __restrict__ buckets,
                                                                       const unsigned long long* __restrict__ hashes,
                                                                       uint64_t entry_size, uint32_t h, uint64_t rows,
                                                                       uint4* __restrict__ records) {
    __shared__ __attribute__((aligned(16))) uint8_t line[kLdsBytes];
    const uint64_t row = blockIdx.x;  // the grid is the rows (launch_fits)
    if (row >= rows || entry_size + 15 > kLdsBytes) return;
    const uint8_t* __restrict__ bytes = buckets + row * entry_size;
    const uint32_t head = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(bytes) & 15u);
    uint64_t front = (16u - head) & 15u;  // the row's bytes in front of its first whole line
    if (front > entry_size) front = entry_size;
    const uint64_t whole = (entry_size - front) / 16, tail = front + 16 * whole;
#pragma unroll 4
    for (uint64_t i = threadIdx.x; i < whole; i += kThreads)
        *reinterpret_cast<uint4*>(line + head + front + 16 * i) = *reinterpret_cast<const uint4*>(bytes + front + 16 * i);
    if (threadIdx.x < front) line[head + threadIdx.x] = bytes[threadIdx.x];
    if (threadIdx.x < entry_size - tail) line[head + tail + threadIdx.x] = bytes[tail + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) records[row] = record_of(walk_bucket<true>(line + head, entry_size, hashes[row / h]));
}

// One lane per (query, bucket), the chain walked in global memory: rows beyond the staged form's LDS budget.
__global__ __launch_bounds__(kClientThreads) void keyword_find_direct_kernel(const uint8_t* __restrict__ buckets,
                                                                             const unsigned long long* __restrict__ hashes,
                                                                             uint64_t entry_size, uint32_t h, uint64_t rows,
                                                                             uint4* __restrict__ records) {
    const uint64_t row = static_cast<uint64_t>(blockIdx.x) * kClientThreads + threadIdx.x;  // (launch_grid::exact_grid)
    if (row >= rows) return;
    records[row] = record_of(walk_bucket<true>(buckets + row * entry_size, entry_size, hashes[row / h]));
}

// Lane (q, c) owns 16-byte line c of the span of out_values[q]: the lines are those of memory, so a whole line is one aligned
// 16-byte store, fed by one 16-byte load from wherever the value lies; a line that the row covers in part, at either end, is
// written byte by byte.  Every lane of a query reads its h records (the same 16 h bytes) and takes the first that is not nil.
__global__ __launch_bounds__(kClientThreads) void keyword_find_resolve_kernel(const uint8_t* __restrict__ buckets,
                                                                              const uint4* __restrict__ records,
                                                                              uint64_t entry_size, uint32_t h, uint64_t capacity,
                                                                              uint64_t lines_per_query, uint64_t lanes,
                                                                              uint8_t* __restrict__ out_values,
                                                                              unsigned long long* __restrict__ out_sizes,
                                                                              uint32_t* __restrict__ out_status) {
    const uint64_t index = static_cast<uint64_t>(blockIdx.x) * kClientThreads + threadIdx.x;  // (launch_grid::exact_grid)
    if (index >= lanes) return;
    const uint64_t query = index / lines_per_query, line = index - query * lines_per_query;
    uint32_t status = kStatusNil;
    uint64_t size = 0, source = 0;  // the value: buckets[source, source + size)
    for (uint32_t bucket = 0; bucket < h; ++bucket) {  // wave-uniform trip count
        const uint4 record = records[query * h + bucket];
        if (record.x == kStatusNil) continue;
        status = record.x;
        if (status == kStatusFound) {
            size = record.y;
            source = (query * h + bucket) * entry_size + (static_cast<uint64_t>(record.w) << 32 | record.z);
        }
        break;
    }
    if (line == 0) {
        out_sizes[query] = size;
        out_status[query] = status;
    }
    if (capacity == 0) return;
    uint8_t* __restrict__ row = out_values + query * capacity;
    const uint64_t head = reinterpret_cast<uintptr_t>(row) & 15u;  // line c is row bytes [16 c - head, 16 c - head + 16)
    const uint64_t begin = line == 0 ? 0 : 16 * line - head;
    uint64_t end = 16 * line - head + 16;
    if (end > capacity) end = capacity;
    if (begin >= end) return;
    const uint8_t* __restrict__ value = buckets + source;  // read below `size` only
    if (end - begin == 16) {
        uint4 word = make_uint4(0, 0, 0, 0);
        if (begin + 16 <= size) {
            __builtin_memcpy(&word, value + begin, 16);  // any address
        } else if (begin < size) {  // the value ends inside this line
            uint64_t lo = 0, hi = 0;
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) {
                if (begin + k < size) lo |= static_cast<uint64_t>(value[begin + k]) << (8 * k);
                if (begin + 8 + k < size) hi |= static_cast<uint64_t>(value[begin + 8 + k]) << (8 * k);
            }
            word = make_uint4(static_cast<uint32_t>(lo), static_cast<uint32_t>(lo >> 32), static_cast<uint32_t>(hi),
                              static_cast<uint32_t>(hi >> 32));
        }
        *reinterpret_cast<uint4*>(row + begin) = word;
    } else {
        for (uint64_t at = begin; at < end; ++at) row[at] = at < size ? value[at] : uint8_t(0);
    }
}

// One wave per query, a lane per reply (replies beyond 64 in further trips): the scan of countEntriesInResponse.  A zero byte
// is an empty bucket of one byte, so eight zero bytes are eight of them: padding is stepped over eight bytes at a time where
// eight are left and all are zero.
constexpr unsigned kCountThreads = 64;
__global__ __launch_bounds__(kCountThreads) void keyword_count_kernel(const uint8_t* __restrict__ bytes, uint64_t reply_bytes,
                                                                      uint64_t replies, uint64_t queries,
                                                                      unsigned long long* __restrict__ out_counts) {
    const uint64_t query = blockIdx.x;  // the grid is the queries (launch_fits)
    if (query >= queries) return;
    unsigned long long total = 0;
    for (uint64_t reply = threadIdx.x; reply < replies; reply += kCountThreads) {
        const uint8_t* __restrict__ b = bytes + (query * replies + reply) * reply_bytes;
        uint64_t offset = 0;
        while (offset < reply_bytes) {
            if (b[offset] == 0) {
                uint64_t eight = 1;
                if (offset + 8 <= reply_bytes) __builtin_memcpy(&eight, b + offset, 8);
                offset += eight == 0 ? 8 : 1;
                continue;
            }
            const BucketWalk walk = walk_bucket<false>(b + offset, reply_bytes - offset, 0);
            if (walk.status == kStatusCorrupt) break;  // `try?` fails: the scan ends, this bucket's slots do not count
            total += walk.slots;
            offset += walk.end;
        }
    }
    for (int delta = kCountThreads / 2; delta > 0; delta >>= 1) total += __shfl_down(total, delta);
    if (threadIdx.x == 0) out_counts[query] = total;
}

}  // namespace

hipError_t launch_keyword_client_widen_indices(const uint32_t* in, uint64_t* out, size_t count, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(keyword_client_widen_kernel, dim3(launch_grid::exact_grid(count, kClientThreads)), dim3(kClientThreads), 0,
                       stream, in, reinterpret_cast<unsigned long long*>(out), static_cast<uint64_t>(count));
    return hipGetLastError();
}

hipError_t launch_keyword_client_find(const uint8_t* buckets, const uint64_t* hashes, uint64_t entry_size, uint32_t h, size_t queries,
                                      keyword_pir_client::FindForm form, void* records, uint8_t* out_values, uint64_t* out_sizes,
                                      uint32_t* out_status, hipStream_t stream) {
    namespace plan = keyword_pir_client;
    if (entry_size == 0 || h == 0 || h > plan::kMaxHashFunctions) return hipErrorInvalidValue;
    if (form == plan::kFindStaged && entry_size > plan::kStagedRowLimit) return hipErrorInvalidValue;
    if (queries == 0) return hipSuccess;
    const uint64_t rows = static_cast<uint64_t>(queries) * h;
    const uint64_t capacity = plan::value_capacity(entry_size);
    const uint64_t lines_per_query = capacity == 0 ? 1 : (capacity + 15) / 16 + 1;  // a row's span begins anywhere inside a line
    if (lines_per_query > launch_grid::kMaxLanes / queries) return hipErrorInvalidValue;
    const uint64_t lanes = queries * lines_per_query;
    const auto* keys = reinterpret_cast<const unsigned long long*>(hashes);
    uint4* out_records = static_cast<uint4*>(records);
    if (form == plan::kFindDirect) {
        if (rows > launch_grid::kMaxLanes) return hipErrorInvalidValue;
        hipLaunchKernelGGL(keyword_find_direct_kernel, dim3(launch_grid::exact_grid(rows, kClientThreads)), dim3(kClientThreads),
                           0, stream, buckets, keys, entry_size, h, rows, out_records);
    } else if (entry_size <= plan::kStagedSmallRowLimit) {
        if (!launch_grid::launch_fits(rows, 64)) return hipErrorInvalidValue;
        hipLaunchKernelGGL((keyword_find_staged_kernel<plan::kStagedSmallLdsBytes, 64>), dim3(static_cast<unsigned>(rows)),
                           dim3(64), 0, stream, buckets, keys, entry_size, h, rows, out_records);
    } else {
        if (!launch_grid::launch_fits(rows, 256)) return hipErrorInvalidValue;
        hipLaunchKernelGGL((keyword_find_staged_kernel<plan::kStagedLdsBytes, 256>), dim3(static_cast<unsigned>(rows)), dim3(256),
                           0, stream, buckets, keys, entry_size, h, rows, out_records);
    }
    hipError_t status = hipGetLastError();
    if (status != hipSuccess) return status;
    hipLaunchKernelGGL(keyword_find_resolve_kernel, dim3(launch_grid::exact_grid(lanes, kClientThreads)), dim3(kClientThreads), 0,
                       stream, buckets, static_cast<const uint4*>(out_records), entry_size, h, capacity, lines_per_query, lanes,
                       out_values, reinterpret_cast<unsigned long long*>(out_sizes), out_status);
    return hipGetLastError();
}

hipError_t launch_keyword_client_count(const uint8_t* bytes, uint64_t reply_bytes, uint64_t replies_per_query, size_t queries,
                                       uint64_t* out_counts, hipStream_t stream) {
    if (queries == 0) return hipSuccess;
    if (!launch_grid::launch_fits(queries, kCountThreads)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keyword_count_kernel, dim3(static_cast<unsigned>(queries)), dim3(kCountThreads), 0, stream, bytes,
                       reply_bytes, replies_per_query, static_cast<uint64_t>(queries),
                       reinterpret_cast<unsigned long long*>(out_counts));
    return hipGetLastError();
}

}  // namespace heamd
