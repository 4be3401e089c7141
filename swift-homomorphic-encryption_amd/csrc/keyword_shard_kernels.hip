// keyword_shard_kernels.hip -- KeywordDatabase.init(rows:sharding:shardingFunction:) (reference Sources/
// PrivateInformationRetrieval/KeywordPir/KeywordDatabase.swift:406-437) as a stable multi-way partition: the order of the rows
// by shard index (least-significant-digit passes of 8 bits over the 4-byte order array), the shard starts, the new offsets
// (an exclusive scan of the row lengths in the new order) and the gather of a byte blob into that order.
//
// Every kernel runs on an exact grid (launch_grid::exact_grid): a lane owns a fixed number of items and none strides by the
// grid.  No kernel waits for another workgroup: every scan is a reduce, a scan of the sums and an apply, launched one after
// the other.  No atomic decides a position: ranks come from wave-wide matching and per-wave counts in LDS.
#include <hip/hip_runtime.h>

#include "keyword_shard.hpp"
#include "launch_grid.hpp"

namespace heamd {
namespace {

constexpr unsigned kThreads = 256;
constexpr unsigned kWaves = kThreads / 64;
constexpr unsigned kRounds = kShardSortTile / kThreads;  // a lane takes one row in each round
constexpr unsigned kPerLane = kScanTile / kThreads;

// ---- exclusive scan ------------------------------------------------------------------------------------------------------
// The exclusive scan of one value per lane over the workgroup; total: the sum over the workgroup.  wave_totals: LDS [kWaves].
template <typename T>
__device__ __forceinline__ T block_exclusive_scan(T value, T* wave_totals, T& total) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inclusive = value;
#pragma unroll
    for (unsigned distance = 1; distance < 64; distance <<= 1) {
        const T up = __shfl_up(inclusive, distance, 64);
        if (lane >= distance) inclusive += up;
    }
    if (lane == 63) wave_totals[wave] = inclusive;
    __syncthreads();
    T before = 0;
    total = 0;
#pragma unroll
    for (unsigned w = 0; w < kWaves; ++w) {
        const T of_wave = wave_totals[w];
        if (w < wave) before += of_wave;
        total += of_wave;
    }
    return before + inclusive - value;
}

template <typename T>
__global__ void __launch_bounds__(kThreads) scan_reduce_kernel(const T* __restrict__ data, size_t n, T* __restrict__ sums) {
    __shared__ T wave_totals[kWaves];
    const size_t first = blockIdx.x * size_t(kScanTile) + threadIdx.x * kPerLane;  // (launch_grid::exact_grid)
    T sum = 0;
#pragma unroll
    for (unsigned k = 0; k < kPerLane; ++k)
        if (first + k < n) sum += data[first + k];
    T total;
    (void)block_exclusive_scan(sum, wave_totals, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// prefixes: what lies before each workgroup's tile (nullptr: one workgroup, nothing)
template <typename T>
__global__ void __launch_bounds__(kThreads) scan_apply_kernel(T* __restrict__ data, size_t n, const T* __restrict__ prefixes) {
    __shared__ T wave_totals[kWaves];
    const size_t first = blockIdx.x * size_t(kScanTile) + threadIdx.x * kPerLane;  // (launch_grid::exact_grid)
    T values[kPerLane];
    T sum = 0;
#pragma unroll
    for (unsigned k = 0; k < kPerLane; ++k) {
        values[k] = first + k < n ? data[first + k] : T(0);
        sum += values[k];
    }
    T total;
    T running = block_exclusive_scan(sum, wave_totals, total) + (prefixes != nullptr ? prefixes[blockIdx.x] : T(0));
#pragma unroll
    for (unsigned k = 0; k < kPerLane; ++k) {
        if (first + k < n) data[first + k] = running;
        running += values[k];
    }
}

template <typename T>
hipError_t exclusive_scan(T* data, size_t n, T* scratch, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const size_t blocks = launch_grid::grid_blocks(n, kScanTile, SIZE_MAX);
    if (!launch_grid::launch_fits(blocks, kThreads)) return hipErrorInvalidConfiguration;
    const dim3 grid(launch_grid::exact_grid(blocks * kThreads, kThreads));
    if (blocks > 1) {
        hipLaunchKernelGGL(scan_reduce_kernel<T>, grid, dim3(kThreads), 0, stream, data, n, scratch);
        hipError_t status = hipGetLastError();
        if (status != hipSuccess) return status;
        status = exclusive_scan(scratch, blocks, scratch + blocks, stream);
        if (status != hipSuccess) return status;
    }
    hipLaunchKernelGGL(scan_apply_kernel<T>, grid, dim3(kThreads), 0, stream, data, n, blocks > 1 ? scratch : nullptr);
    return hipGetLastError();
}

// ---- the order -----------------------------------------------------------------------------------------------------------
// Where a lane stands among the lanes of its wave that hold the same digit: eight ballots of the digit's bits give the peers.
struct DigitMatch {
    uint32_t rank;   // peers in lower lanes
    uint32_t peers;  // lanes of the wave with this digit, the lane itself included
    bool leader;     // the lowest of them
};

__device__ __forceinline__ DigitMatch match_digit(uint32_t digit, bool valid) {
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (uint32_t bit = 0; bit < 8; ++bit) {
        const bool set = ((digit >> bit) & 1u) != 0;
        const uint64_t with = __ballot(set);
        peers &= set ? with : ~with;
    }
    const uint32_t lane = threadIdx.x & 63;
    DigitMatch match;
    match.rank = static_cast<uint32_t>(__popcll(peers & ((uint64_t(1) << lane) - 1)));
    match.peers = static_cast<uint32_t>(__popcll(peers));
    match.leader = valid && match.rank == 0;
    return match;
}

// the row at position j of the pass's input order (nullptr: the identity) and the pass's digit of its shard index; an index
// at or above the shard count goes to the last shard
__device__ __forceinline__ uint32_t digit_of(const uint32_t* __restrict__ shard_indices, const uint32_t* __restrict__ order_in,
                                             size_t j, uint32_t last, uint32_t shift, uint32_t& row) {
    row = order_in != nullptr ? order_in[j] : static_cast<uint32_t>(j);
    const uint32_t index = shard_indices[row];
    return ((index < last ? index : last) >> shift) & 0xffu;
}

// counts[digit][workgroup]: the rows of the workgroup's tile with that digit
__global__ void __launch_bounds__(kThreads)
    shard_digit_count_kernel(const uint32_t* __restrict__ shard_indices, const uint32_t* __restrict__ order_in, size_t count,
                             uint32_t last, uint32_t shift, size_t workgroups, uint32_t* __restrict__ counts) {
    __shared__ uint32_t wave_counts[kWaves][256];
    const unsigned tid = threadIdx.x, wave = tid >> 6;
#pragma unroll
    for (unsigned w = 0; w < kWaves; ++w) wave_counts[w][tid] = 0;
    __syncthreads();
    const size_t first = blockIdx.x * size_t(kShardSortTile);  // one tile per workgroup (launch_grid::exact_grid)
    for (unsigned round = 0; round < kRounds; ++round) {
        const size_t j = first + round * kThreads + tid;
        const bool valid = j < count;
        uint32_t row = 0;
        const uint32_t digit = valid ? digit_of(shard_indices, order_in, j, last, shift, row) : 0;
        const DigitMatch match = match_digit(digit, valid);
        if (match.leader) wave_counts[wave][digit] += match.peers;  // the leaders of a wave hold different digits
        __syncthreads();
    }
    uint32_t total = 0;
#pragma unroll
    for (unsigned w = 0; w < kWaves; ++w) total += wave_counts[w][tid];
    counts[tid * workgroups + blockIdx.x] = total;
}

// bases: the exclusive scan of counts.  A row's position is its digit's base, plus the rows of that digit in earlier rounds,
// plus those in earlier waves of its round, plus its rank in its wave: input order within a digit, so the pass is stable.
__global__ void __launch_bounds__(kThreads)
    shard_digit_scatter_kernel(const uint32_t* __restrict__ shard_indices, const uint32_t* __restrict__ order_in, size_t count,
                               uint32_t last, uint32_t shift, size_t workgroups, const uint32_t* __restrict__ bases,
                               uint32_t* __restrict__ order_out) {
    __shared__ uint32_t running[256];
    __shared__ uint32_t wave_counts[kWaves][256];
    const unsigned tid = threadIdx.x, wave = tid >> 6;
    running[tid] = bases[tid * workgroups + blockIdx.x];
#pragma unroll
    for (unsigned w = 0; w < kWaves; ++w) wave_counts[w][tid] = 0;
    __syncthreads();
    const size_t first = blockIdx.x * size_t(kShardSortTile);  // one tile per workgroup (launch_grid::exact_grid)
    for (unsigned round = 0; round < kRounds; ++round) {
        const size_t j = first + round * kThreads + tid;
        const bool valid = j < count;
        uint32_t row = 0;
        const uint32_t digit = valid ? digit_of(shard_indices, order_in, j, last, shift, row) : 0;
        const DigitMatch match = match_digit(digit, valid);
        if (match.leader) wave_counts[wave][digit] = match.peers;
        __syncthreads();
        if (valid) {
            uint32_t position = running[digit] + match.rank;
#pragma unroll
            for (unsigned w = 0; w < kWaves; ++w)
                if (w < wave) position += wave_counts[w][digit];
            if (position < count) order_out[position] = row;  // (always, while shard_indices holds what was counted)
        }
        __syncthreads();
        uint32_t total = 0;
#pragma unroll
        for (unsigned w = 0; w < kWaves; ++w) {
            total += wave_counts[w][tid];
            wave_counts[w][tid] = 0;
        }
        running[tid] += total;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kThreads) identity_order_kernel(size_t count, uint32_t* __restrict__ order) {
    const size_t j = blockIdx.x * size_t(kThreads) + threadIdx.x;  // one row per lane (launch_grid::exact_grid)
    if (j < count) order[j] = static_cast<uint32_t>(j);
}

// One lane per shard (and one for the end): the first output row whose shard index is not below the lane's.
__global__ void __launch_bounds__(kThreads)
    shard_starts_kernel(const uint32_t* __restrict__ shard_indices, const uint32_t* __restrict__ order, size_t count,
                        uint64_t shard_count, uint64_t first_shard, uint32_t* __restrict__ shard_starts) {
    const uint64_t shard = first_shard + blockIdx.x * uint64_t(kThreads) + threadIdx.x;  // (launch_grid::exact_grid)
    if (shard > shard_count) return;
    const uint32_t last = static_cast<uint32_t>(shard_count - 1);
    size_t lo = 0, hi = count;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        const uint32_t index = shard_indices[order[mid]];
        if ((index < last ? index : last) < shard) lo = mid + 1; else hi = mid;
    }
    shard_starts[shard] = static_cast<uint32_t>(lo);
}

__global__ void __launch_bounds__(kThreads)
    row_lengths_kernel(const uint64_t* __restrict__ offsets, const uint32_t* __restrict__ order, size_t count, uint64_t bytes,
                       const uint32_t* __restrict__ shard_indices, uint64_t shard_count, uint64_t* __restrict__ out_offsets,
                       uint32_t* __restrict__ mismatch) {
    const size_t j = blockIdx.x * size_t(kThreads) + threadIdx.x;  // one row per lane, one more lane (launch_grid::exact_grid)
    if (j > count) return;
    uint32_t flags = 0;
    if (j < count) {
        const uint32_t row = order[j];
        out_offsets[j] = offsets[row + size_t(1)] - offsets[row];
        if (mismatch != nullptr && shard_indices[row] >= shard_count) flags = 1;
    } else {
        out_offsets[count] = 0;
        if (offsets[count] - offsets[0] != bytes) flags = 2;
    }
    if (mismatch != nullptr && flags != 0) atomicOr(mismatch, flags);
}

// The last row that starts at or before output byte `position` (rows before it end there or earlier), searched in
// [row, above): out_offsets[row] <= position, and no row from `above` on starts at or before it.
__device__ __forceinline__ size_t row_of(const uint64_t* __restrict__ out_offsets, uint64_t position, size_t row, size_t above) {
    while (above - row > 1) {
        const size_t mid = row + (above - row) / 2;
        if (out_offsets[mid] <= position) row = mid; else above = mid;
    }
    return row;
}

constexpr uint64_t kGatherTile = 64;  // chunks of a tile: the 512 output bytes one wave writes

// tile_rows[t]: the row the first byte of tile t falls in, by binary search over all rows; the gather's lanes then search
// only between their tile's row and the next tile's (a few rows) instead of walking log2(count) dependent loads each.
__global__ void __launch_bounds__(kThreads)
    gather_tile_rows_kernel(const uint64_t* __restrict__ out_offsets, size_t count, uint64_t bytes, uint64_t head,
                            uint64_t tiles, uint32_t* __restrict__ tile_rows) {
    const uint64_t tile = blockIdx.x * uint64_t(kThreads) + threadIdx.x;  // one tile per lane, one more (launch_grid::exact_grid)
    if (tile > tiles) return;
    const uint64_t sorted_bytes = out_offsets[count];
    const uint64_t total = sorted_bytes < bytes ? sorted_bytes : bytes;
    const uint64_t position = tile == 0 ? 0 : 8 * kGatherTile * tile - head;
    tile_rows[tile] = static_cast<uint32_t>(tile == tiles || position >= total ? count - 1 : row_of(out_offsets, position, 0, count));
}

// A lane owns one aligned 8-byte chunk of the output: it finds the row its first byte falls in by binary search over the new
// offsets (between the rows of its tile's and the next tile's first bytes), gathers across as many rows as the chunk spans
// and issues one 8-byte store; byte stores only where the chunk crosses the first or last byte of [out, out + total).
__global__ void __launch_bounds__(kThreads)
    blob_gather_kernel(const uint8_t* __restrict__ blob, const uint64_t* __restrict__ offsets,
                       const uint32_t* __restrict__ order, const uint64_t* __restrict__ out_offsets,
                       const uint32_t* __restrict__ tile_rows, size_t count, uint64_t bytes, uint8_t* __restrict__ out,
                       uint64_t first_chunk, uint64_t chunks) {
    const uint64_t head = reinterpret_cast<uintptr_t>(out) & 7;  // chunk c holds output bytes [8 c - head, 8 c - head + 8)
    const uint64_t chunk = first_chunk + blockIdx.x * uint64_t(kThreads) + threadIdx.x;  // (launch_grid::exact_grid)
    if (chunk >= chunks) return;
    const uint64_t sorted_bytes = out_offsets[count];
    const uint64_t total = sorted_bytes < bytes ? sorted_bytes : bytes;
    const uint32_t lo = chunk == 0 ? static_cast<uint32_t>(head) : 0;
    const uint64_t position = 8 * chunk + lo - head;  // the first output byte of the chunk
    if (position >= total) return;
    const uint64_t left = total - position;
    const uint32_t hi = left < 8 - lo ? lo + static_cast<uint32_t>(left) : 8;
    const uint64_t tile = chunk / kGatherTile;
    size_t row = row_of(out_offsets, position, tile_rows[tile], size_t(tile_rows[tile + 1]) + 1);
    uint64_t row_start = out_offsets[row], row_end = out_offsets[row + 1];
    uint64_t shift = offsets[order[row]] - row_start;  // output byte p of this row is blob[p + shift]
    const bool whole = lo == 0 && hi == 8;
    uint64_t word = 0;
    if (whole && position + 8 <= row_end) {
        __builtin_memcpy(&word, blob + (position + shift), 8);  // inside one row: eight bytes from any address
    } else {
        uint64_t p = position;
        for (uint32_t k = lo; k < hi; ++k, ++p) {
            while (p >= row_end) {  // (p < total: a later row holds it)
                ++row;
                row_start = row_end;
                row_end = out_offsets[row + 1];
                shift = offsets[order[row]] - row_start;
            }
            word |= uint64_t(blob[p + shift]) << (8 * k);
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

__global__ void __launch_bounds__(kThreads)
    gather_words_kernel(const uint64_t* __restrict__ in, const uint32_t* __restrict__ order, size_t count,
                        uint64_t* __restrict__ out) {
    const size_t j = blockIdx.x * size_t(kThreads) + threadIdx.x;  // one word per lane (launch_grid::exact_grid)
    if (j < count) out[j] = in[order[j]];
}

uint32_t bit_length(uint64_t value) {
    uint32_t bits = 0;
    for (; value != 0; value >>= 1) ++bits;
    return bits;
}

}  // namespace

PartitionPlan partition_plan(size_t count, size_t shard_count) {
    PartitionPlan plan;
    if (count == 0) return plan;
    plan.digit_passes = shard_count <= 1 ? 0 : (bit_length(shard_count - 1) + 7) / 8;
    plan.workgroups = launch_grid::grid_blocks(count, kShardSortTile, SIZE_MAX);
    plan.last_rows = count - (plan.workgroups - 1) * size_t(kShardSortTile);
    return plan;
}

size_t scan_scratch_elements(size_t n) {
    size_t elements = 0;
    for (size_t blocks = launch_grid::grid_blocks(n, kScanTile, SIZE_MAX); blocks > 1;
         blocks = launch_grid::grid_blocks(blocks, kScanTile, SIZE_MAX))
        elements += blocks;
    return elements;
}

hipError_t launch_exclusive_scan(uint32_t* data, size_t n, uint32_t* scratch, hipStream_t stream) {
    return exclusive_scan(data, n, scratch, stream);
}
hipError_t launch_exclusive_scan(uint64_t* data, size_t n, uint64_t* scratch, hipStream_t stream) {
    return exclusive_scan(data, n, scratch, stream);
}

hipError_t launch_shard_order(const uint32_t* shard_indices, size_t count, size_t shard_count, const PartitionPlan& plan,
                              uint32_t* order, uint32_t* alternate, uint32_t* counts, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    if (plan.digit_passes == 0) {
        hipLaunchKernelGGL(identity_order_kernel, dim3(launch_grid::exact_grid(count, kThreads)), dim3(kThreads), 0, stream, count,
                           order);
        return hipGetLastError();
    }
    const size_t workgroups = plan.workgroups, bins = 256 * workgroups;
    if (!launch_grid::launch_fits(workgroups, kThreads)) return hipErrorInvalidConfiguration;
    const dim3 grid(launch_grid::exact_grid(workgroups * kThreads, kThreads));
    const uint32_t last = static_cast<uint32_t>(shard_count - 1);
    const uint32_t* order_in = nullptr;
    for (uint32_t pass = 0; pass < plan.digit_passes; ++pass) {
        uint32_t* order_out = (plan.digit_passes - 1 - pass) % 2 == 0 ? order : alternate;  // the last pass writes `order`
        hipLaunchKernelGGL(shard_digit_count_kernel, grid, dim3(kThreads), 0, stream, shard_indices, order_in, count, last,
                           8 * pass, workgroups, counts);
        hipError_t status = hipGetLastError();
        if (status != hipSuccess) return status;
        status = launch_exclusive_scan(counts, bins, counts + bins, stream);
        if (status != hipSuccess) return status;
        hipLaunchKernelGGL(shard_digit_scatter_kernel, grid, dim3(kThreads), 0, stream, shard_indices, order_in, count, last,
                           8 * pass, workgroups, static_cast<const uint32_t*>(counts), order_out);
        status = hipGetLastError();
        if (status != hipSuccess) return status;
        order_in = order_out;
    }
    return hipSuccess;
}

hipError_t launch_shard_starts(const uint32_t* shard_indices, const uint32_t* order, size_t count, size_t shard_count,
                               uint32_t* shard_starts, hipStream_t stream) {
    const uint64_t lanes = uint64_t(shard_count) + 1;
    const uint64_t most = launch_grid::max_blocks(kThreads) * kThreads;  // shards of one launch
    for (uint64_t first = 0; first < lanes; first += most) {
        const uint64_t now = lanes - first < most ? lanes - first : most;
        hipLaunchKernelGGL(shard_starts_kernel, dim3(launch_grid::exact_grid(now, kThreads)), dim3(kThreads), 0, stream,
                           shard_indices, order, count, uint64_t(shard_count), first, shard_starts);
        const hipError_t status = hipGetLastError();
        if (status != hipSuccess) return status;
    }
    return hipSuccess;
}

hipError_t launch_row_lengths(const uint64_t* offsets, const uint32_t* order, size_t count, uint64_t bytes,
                              const uint32_t* shard_indices, size_t shard_count, uint64_t* out_offsets, uint32_t* mismatch,
                              hipStream_t stream) {
    hipLaunchKernelGGL(row_lengths_kernel, dim3(launch_grid::exact_grid(count + 1, kThreads)), dim3(kThreads), 0, stream, offsets,
                       order, count, bytes, shard_indices, uint64_t(shard_count), out_offsets, mismatch);
    return hipGetLastError();
}

size_t gather_scratch_elements(uint64_t bytes) { return static_cast<size_t>(((bytes + 14) / 8 + kGatherTile - 1) / kGatherTile + 1); }

hipError_t launch_blob_gather(const uint8_t* blob, const uint64_t* offsets, const uint32_t* order, const uint64_t* out_offsets,
                              size_t count, uint64_t bytes, uint8_t* out, uint32_t* tile_rows, hipStream_t stream) {
    if (bytes == 0 || count == 0) return hipSuccess;
    const uint64_t head = reinterpret_cast<uintptr_t>(out) & 7;
    const uint64_t chunks = (head + bytes + 7) / 8;
    const uint64_t tiles = (chunks + kGatherTile - 1) / kGatherTile;  // (tiles + 1 <= gather_scratch_elements(bytes))
    hipLaunchKernelGGL(gather_tile_rows_kernel, dim3(launch_grid::exact_grid(tiles + 1, kThreads)), dim3(kThreads), 0, stream,
                       out_offsets, count, bytes, head, tiles, tile_rows);
    hipError_t status = hipGetLastError();
    if (status != hipSuccess) return status;
    const uint64_t most = launch_grid::max_blocks(kThreads) * kThreads;  // chunks of one launch: 32 GiB
    for (uint64_t first = 0; first < chunks; first += most) {
        const uint64_t now = chunks - first < most ? chunks - first : most;
        hipLaunchKernelGGL(blob_gather_kernel, dim3(launch_grid::exact_grid(now, kThreads)), dim3(kThreads), 0, stream, blob,
                           offsets, order, out_offsets, static_cast<const uint32_t*>(tile_rows), count, bytes, out, first, chunks);
        status = hipGetLastError();
        if (status != hipSuccess) return status;
    }
    return hipSuccess;
}

hipError_t launch_gather_words(const uint64_t* in, const uint32_t* order, size_t count, uint64_t* out, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(gather_words_kernel, dim3(launch_grid::exact_grid(count, kThreads)), dim3(kThreads), 0, stream, in, order,
                       count, out);
    return hipGetLastError();
}

}  // namespace heamd
