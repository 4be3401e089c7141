// simple_pir_shard_kernels.hip -- DatabaseMap.shardDatabase (reference Sources/PrivateInformationRetrieval/SimplePir/
// DatabaseMap.swift:82-110) and the two halves of SimplePirClientForAllShards (SimplePir+Shards.swift:71-99, :139-171).
//
// The split.  Entry e of len_e bytes has c_e = ceil(len_e / C) chunks; chunk k goes to shard order_e[k mod S], at the index that
// shard's row count had then.  Entry e therefore gives shard s exactly c_e / S + [position_e(s) < c_e mod S] rows, position_e
// being the inverse of its order, and chunk k = j + i S lands at (rows of shard order_e[j] from earlier entries) + i.  The
// per-shard row counts of earlier entries are a scan of S-vectors: a tile of kMapTile entries per workgroup, one entry per lane,
// the inverse orders in LDS (S bytes per lane), and per shard one scan over the tile.  Pass 1 writes the tile sums
// [shard][tile]; their exclusive scan in that order is at once the base of every (shard, tile) in the back-to-back slab, so
// pass 2 writes each chunk's (shard, index) and the inverse map row -> chunk.  Scratch: O(tiles x S) words.
//
// Every kernel runs on an exact grid (launch_grid::exact_grid): a lane owns a fixed item and none strides by the grid.  No
// kernel waits for another workgroup.  No atomic decides a position: the only atomic is the OR into the caller's mismatch word.
// Every store is bounded by the capacity the caller stated (total_chunks), whatever the offsets and orders hold.
#include <hip/hip_runtime.h>

#include "keyword_shard.hpp"
#include "launch_grid.hpp"
#include "simple_pir_shard.hpp"

namespace heamd {
namespace {

using simple_pir_shard::Form;
using simple_pir_shard::kMapTile;
using simple_pir_shard::kThreads;
constexpr unsigned kMapWaves = kMapTile / 64;
static_assert(simple_pir_shard::kScanTile == kScanTile, "simple_pir_shard_plan.hpp sizes the scans' scratch");
static_assert(kMapTile % 64 == 0 && simple_pir_shard::kMaxShardCount <= 256, "an order position is one byte");

// ---- the map -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
    shard_chunk_counts_kernel(const uint64_t* __restrict__ offsets, uint64_t count, uint64_t chunk_size,
                              uint64_t* __restrict__ chunk_starts) {
    const uint64_t e = blockIdx.x * uint64_t(kThreads) + threadIdx.x;  // one entry per lane, one more (launch_grid::exact_grid)
    if (e > count) return;
    uint64_t chunks = 0;
    if (e < count) {
        const uint64_t length = offsets[e + 1] - offsets[e];
        chunks = length / chunk_size + (length % chunk_size != 0 ? 1 : 0);
    }
    chunk_starts[e] = chunks;  // the input of the scan
}

// The exclusive scan of one value per lane over the tile's workgroup; total: the sum over it.  May be called in a loop.
__device__ __forceinline__ uint32_t tile_exclusive_scan(uint32_t value, uint32_t* wave_totals, uint32_t& total) {
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inclusive = value;
#pragma unroll
    for (unsigned distance = 1; distance < 64; distance <<= 1) {
        const uint32_t up = __shfl_up(inclusive, distance, 64);
        if (lane >= distance) inclusive += up;
    }
    if (lane == 63) wave_totals[wave] = inclusive;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (unsigned w = 0; w < kMapWaves; ++w) {
        const uint32_t of_wave = wave_totals[w];
        if (w < wave) before += of_wave;
        total += of_wave;
    }
    __syncthreads();
    return before + inclusive - value;
}

// positions[s * kMapTile + lane]: where shard s stands in the order of the lane's entry.  A lane touches its own column only.
// False for a row that is no permutation of 0 .. S - 1 (a value at or above S, or a repeat): the identity is stored then.
__device__ __forceinline__ bool entry_positions_of(const uint8_t* __restrict__ order, uint32_t S, uint8_t* positions) {
    uint8_t* mine = positions + threadIdx.x;
    bool valid = true;
    for (uint32_t j = 0; j < S; ++j) {
        const uint32_t shard = order[j];
        if (shard < S) mine[shard * kMapTile] = static_cast<uint8_t>(j); else valid = false;
    }
    if (valid)
        for (uint32_t j = 0; j < S; ++j)  // of two positions that name one shard, the earlier finds the later one's mark
            if (mine[uint32_t(order[j]) * kMapTile] != static_cast<uint8_t>(j)) valid = false;
    if (!valid)
        for (uint32_t s = 0; s < S; ++s) mine[s * kMapTile] = static_cast<uint8_t>(s);
    return valid;
}

// sums[s * tiles + tile]: the rows the tile's entries give shard s
__global__ void __launch_bounds__(kMapTile)
    shard_tile_sums_kernel(const uint64_t* __restrict__ chunk_starts, const uint8_t* __restrict__ orders, uint64_t count, uint32_t S,
                           uint64_t tiles, uint32_t* __restrict__ sums, uint32_t* __restrict__ mismatch) {
    extern __shared__ uint8_t positions[];  // [S][kMapTile]
    __shared__ uint32_t wave_totals[kMapWaves];
    const uint64_t e = blockIdx.x * uint64_t(kMapTile) + threadIdx.x;  // one tile per workgroup (launch_grid::exact_grid)
    const bool live = e < count;
    uint64_t chunks = 0;
    if (live) {
        chunks = chunk_starts[e + 1] - chunk_starts[e];
        if (!entry_positions_of(orders + e * S, S, positions) && mismatch != nullptr) atomicOr(mismatch, 1u);
    }
    const uint32_t whole = static_cast<uint32_t>(chunks / S), rest = static_cast<uint32_t>(chunks % S);
    for (uint32_t s = 0; s < S; ++s) {
        const uint32_t rows = live ? whole + (positions[s * kMapTile + threadIdx.x] < rest ? 1u : 0u) : 0u;
        uint32_t total;
        (void)tile_exclusive_scan(rows, wave_totals, total);
        if (threadIdx.x == 0) sums[s * tiles + blockIdx.x] = total;
    }
}

// bases: the exclusive scan of sums -- bases[s * tiles + tile] is the slab row of the first chunk the tile gives shard s
__global__ void __launch_bounds__(kMapTile)
    shard_tile_apply_kernel(const uint64_t* __restrict__ chunk_starts, const uint8_t* __restrict__ orders, uint64_t count, uint32_t S,
                            uint64_t tiles, const uint32_t* __restrict__ bases, uint64_t total_chunks,
                            uint32_t* __restrict__ chunk_shard, uint32_t* __restrict__ chunk_index, uint32_t* __restrict__ row_chunk) {
    extern __shared__ uint8_t positions[];  // [S][kMapTile]
    __shared__ uint32_t wave_totals[kMapWaves];
    const uint64_t e = blockIdx.x * uint64_t(kMapTile) + threadIdx.x;  // one tile per workgroup (launch_grid::exact_grid)
    const bool live = e < count;
    uint64_t first = 0, chunks = 0;
    if (live) {
        first = chunk_starts[e];
        chunks = chunk_starts[e + 1] - first;
        (void)entry_positions_of(orders + e * S, S, positions);
    }
    const uint32_t whole = static_cast<uint32_t>(chunks / S), rest = static_cast<uint32_t>(chunks % S);
    for (uint32_t s = 0; s < S; ++s) {
        const uint32_t position = live ? positions[s * kMapTile + threadIdx.x] : 0u;
        const uint32_t rows = live ? whole + (position < rest ? 1u : 0u) : 0u;
        uint32_t total;
        const uint32_t before = tile_exclusive_scan(rows, wave_totals, total);
        const uint32_t shard_first = bases[s * tiles];
        const uint32_t row = bases[s * tiles + blockIdx.x] + before;
        for (uint32_t i = 0; i < rows; ++i) {
            const uint64_t flat = first + position + uint64_t(i) * S;  // chunk position + i S of the entry
            if (flat >= total_chunks) break;                           // (never, while the caller's claim holds)
            const uint64_t at = uint64_t(row) + i;
            chunk_shard[flat] = s;
            chunk_index[flat] = static_cast<uint32_t>(at - shard_first);
            if (at < total_chunks) row_chunk[at] = static_cast<uint32_t>(flat);
        }
    }
}

__global__ void __launch_bounds__(kThreads)
    shard_row_starts_kernel(const uint64_t* __restrict__ chunk_starts, uint64_t count, uint32_t S, uint64_t tiles,
                            const uint32_t* __restrict__ bases, uint64_t total_chunks, uint64_t* __restrict__ shard_row_starts,
                            uint32_t* __restrict__ mismatch) {
    const uint32_t s = blockIdx.x * kThreads + threadIdx.x;  // one shard per lane, one more (launch_grid::exact_grid)
    if (s > S) return;
    const uint64_t all = chunk_starts[count];
    if (s == S) {
        shard_row_starts[S] = all;
        if (mismatch != nullptr && all != total_chunks) atomicOr(mismatch, 2u);
    } else {
        shard_row_starts[s] = tiles != 0 ? bases[s * tiles] : 0;
    }
}

// ---- moving bytes --------------------------------------------------------------------------------------------------------
template <unsigned W>
struct Piece {
    uint8_t bytes[W];
};

template <unsigned W>
__device__ __forceinline__ void store_piece(uint8_t* at, const Piece<W>& piece) {
    if constexpr (W == 16) {
        ulonglong2 words;
        __builtin_memcpy(&words, piece.bytes, 16);
        *reinterpret_cast<ulonglong2*>(at) = words;
    } else if constexpr (W == 8) {
        uint64_t word;
        __builtin_memcpy(&word, piece.bytes, 8);
        *reinterpret_cast<uint64_t*>(at) = word;
    } else {
        at[0] = piece.bytes[0];
    }
}

// The entry flat chunk `flat` belongs to: the last e with chunk_starts[e] <= flat (entries without a chunk share their start
// with the next one and are passed over).  count >= 1.
__device__ __forceinline__ uint64_t entry_of_chunk(const uint64_t* __restrict__ chunk_starts, uint64_t count, uint64_t flat) {
    uint64_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (chunk_starts[mid] <= flat) lo = mid; else hi = mid;
    }
    return lo;
}

// A lane owns one aligned piece of W bytes of the slab, inside one row: it finds the row's chunk through row_chunk, the chunk's
// entry by binary search over chunk_starts, reads the source bytes from whatever address they have and writes zeros past the
// value's end.
template <unsigned W>
__global__ void __launch_bounds__(kThreads)
    shard_scatter_kernel(const uint8_t* __restrict__ values, uint64_t values_bytes, const uint64_t* __restrict__ offsets,
                         SimplePirShardMapView map, uint8_t* __restrict__ shards, uint64_t first_piece, uint64_t pieces) {
    const uint64_t piece = first_piece + blockIdx.x * uint64_t(kThreads) + threadIdx.x;  // (launch_grid::exact_grid)
    if (piece >= pieces) return;
    const uint64_t byte = piece * W, row = byte / map.chunk_size, within = byte % map.chunk_size;
    Piece<W> out = {};
    const uint64_t flat = map.row_chunk[row];
    if (flat < map.total_chunks && map.count != 0) {
        const uint64_t e = entry_of_chunk(map.chunk_starts, map.count, flat);
        const uint64_t begin = offsets[e] + (flat - map.chunk_starts[e]) * map.chunk_size + within;
        uint64_t end = offsets[e + 1];
        if (end > values_bytes) end = values_bytes;
        if (begin < end) {
            if (end - begin >= W) {
                __builtin_memcpy(out.bytes, values + begin, W);  // W bytes from any address
            } else {
                for (unsigned i = 0; i < W; ++i)
                    if (i < end - begin) out.bytes[i] = values[begin + i];
            }
        }
    }
    store_piece<W>(shards + byte, out);
}

// One lane per output index: slot `slot` of lookup b in shard s's plane is the index of the slot-th chunk of the entry that
// lies in shard s, zero when the entry has fewer there (or does not exist).  The walk over the entry's chunks has
// maximum_chunk_count steps for every lane.
__global__ void __launch_bounds__(kThreads)
    shard_query_indices_kernel(const uint64_t* __restrict__ entry_positions, uint64_t batch, SimplePirShardMapView map,
                               uint64_t maximum_chunk_count, uint64_t chunks_per_shard, uint64_t lanes,
                               uint64_t* __restrict__ out_indices, uint32_t* __restrict__ out_found) {
    const uint64_t lane = blockIdx.x * uint64_t(kThreads) + threadIdx.x;  // (launch_grid::exact_grid)
    if (lane < batch) out_found[lane] = entry_positions[lane] < map.count ? 1u : 0u;
    if (lane >= lanes) return;
    const uint64_t slot = lane % chunks_per_shard, b = (lane / chunks_per_shard) % batch, s = lane / chunks_per_shard / batch;
    const uint64_t position = entry_positions[b];
    const bool present = position < map.count;
    const uint64_t e = present ? position : 0;
    uint64_t first = 0, chunks = 0;
    if (map.count != 0) {
        first = map.chunk_starts[e];
        chunks = present ? map.chunk_starts[e + 1] - first : 0;
    }
    uint64_t index = 0, seen = 0;
    for (uint64_t k = 0; k < maximum_chunk_count; ++k) {
        const uint64_t flat = first + k;
        const bool real = k < chunks && flat < map.total_chunks;
        const uint64_t at = real ? flat : 0;
        const uint32_t shard = map.total_chunks != 0 ? map.chunk_shard[at] : 0;
        const uint32_t value = map.total_chunks != 0 ? map.chunk_index[at] : 0;
        const bool here = real && shard == s;
        if (here && seen == slot) index = value;
        seen += here ? 1 : 0;
    }
    out_indices[lane] = index;
}

// A lane owns one aligned piece of W bytes of out_entries, inside chunk k of lookup b.  The chunk's (shard, index) come from
// the map for a real chunk and are (0, 0) otherwise; the slot is the last of that shard's query slots whose index equals the
// target, slot 0 when none does (SimplePir+Shards.swift:159-164).  Every lane reads one map pair, chunks_per_shard indices and
// W chunk bytes and writes W bytes, whether the entry exists or not; what lies at or past the entry's size is masked to zero.
template <unsigned W>
__global__ void __launch_bounds__(kThreads)
    shard_assemble_kernel(const uint8_t* __restrict__ chunks, const uint64_t* __restrict__ indices,
                          const uint64_t* __restrict__ entry_positions, uint64_t batch, const uint64_t* __restrict__ offsets,
                          SimplePirShardMapView map, uint64_t maximum_chunk_count, uint64_t chunks_per_shard, uint64_t pieces,
                          uint8_t* __restrict__ out_entries, uint64_t* __restrict__ out_sizes, uint32_t* __restrict__ out_found) {
    const uint64_t piece = blockIdx.x * uint64_t(kThreads) + threadIdx.x;  // (launch_grid::exact_grid)
    if (piece < batch) {
        const uint64_t position = entry_positions[piece];
        const bool present = position < map.count;
        const uint64_t e = present ? position : 0;
        const uint64_t size = map.count != 0 ? offsets[e + 1] - offsets[e] : 0;
        out_sizes[piece] = present ? size : 0;
        out_found[piece] = present ? 1u : 0u;
    }
    if (piece >= pieces) return;
    const uint64_t entry_bytes = maximum_chunk_count * map.chunk_size;
    const uint64_t byte = piece * W, b = byte / entry_bytes, inside = byte % entry_bytes;
    const uint64_t k = inside / map.chunk_size, within = inside % map.chunk_size;
    const uint64_t position = entry_positions[b];
    const bool present = position < map.count;
    const uint64_t e = present ? position : 0;
    uint64_t first = 0, count_of_entry = 0, size = 0;
    if (map.count != 0) {
        first = map.chunk_starts[e];
        count_of_entry = map.chunk_starts[e + 1] - first;
        size = offsets[e + 1] - offsets[e];
    }
    const bool real = present && k < count_of_entry && first + k < map.total_chunks;
    const uint64_t at = real ? first + k : 0;
    uint64_t shard = map.total_chunks != 0 ? map.chunk_shard[at] : 0;
    uint64_t target = map.total_chunks != 0 ? map.chunk_index[at] : 0;
    shard = real && shard < map.shard_count ? shard : 0;
    target = real ? target : 0;
    const uint64_t plane = (shard * batch + b) * chunks_per_shard;
    uint64_t slot = 0;
    for (uint64_t j = 0; j < chunks_per_shard; ++j) slot = indices[plane + j] == target ? j : slot;
    Piece<W> out;
    const uint8_t* source = chunks + (plane + slot) * map.chunk_size + within;
    if constexpr (W == 16) {
        const ulonglong2 words = *reinterpret_cast<const ulonglong2*>(source);
        __builtin_memcpy(out.bytes, &words, 16);
    } else if constexpr (W == 8) {
        const uint64_t word = *reinterpret_cast<const uint64_t*>(source);
        __builtin_memcpy(out.bytes, &word, 8);
    } else {
        out.bytes[0] = source[0];
    }
    const uint64_t kept = present && inside < size ? size - inside : 0;  // bytes of this piece below the entry's size
#pragma unroll
    for (unsigned i = 0; i < W; ++i) out.bytes[i] = i < kept ? out.bytes[i] : uint8_t(0);
    store_piece<W>(out_entries + byte, out);
}

template <typename Launch>
hipError_t for_each_launch(uint64_t lanes, Launch launch) {
    const uint64_t most = launch_grid::max_blocks(kThreads) * uint64_t(kThreads);  // lanes of one launch
    for (uint64_t first = 0; first < lanes; first += most) {
        const uint64_t now = lanes - first < most ? lanes - first : most;
        launch(dim3(launch_grid::exact_grid(now, kThreads)), first);
        const hipError_t status = hipGetLastError();
        if (status != hipSuccess) return status;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_simple_pir_shard_map(const uint64_t* value_offsets, const uint8_t* shard_orders, uint64_t count,
                                       uint64_t shard_count, uint64_t chunk_size, uint64_t total_chunks,
                                       const simple_pir_shard::Plan& plan, uint64_t* chunk_starts, uint32_t* chunk_shard,
                                       uint32_t* chunk_index, uint64_t* shard_row_starts, uint32_t* row_chunk, uint32_t* mismatch,
                                       uint32_t* sums, uint64_t* scan, hipStream_t stream) {
    const uint32_t S = static_cast<uint32_t>(shard_count);
    const uint64_t tiles = plan.map_tiles;
    if (!launch_grid::launch_fits(plan.count_workgroups, kThreads) || !launch_grid::launch_fits(tiles, kMapTile))
        return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(shard_chunk_counts_kernel, dim3(launch_grid::exact_grid(count + 1, kThreads)), dim3(kThreads), 0, stream,
                       value_offsets, count, chunk_size, chunk_starts);
    hipError_t status = hipGetLastError();
    if (status != hipSuccess) return status;
    status = launch_exclusive_scan(chunk_starts, static_cast<size_t>(count + 1), scan, stream);
    if (status != hipSuccess) return status;
    if (tiles != 0) {
        const dim3 grid(launch_grid::exact_grid(tiles * kMapTile, kMapTile));
        const size_t lds = size_t(S) * kMapTile;
        hipLaunchKernelGGL(shard_tile_sums_kernel, grid, dim3(kMapTile), lds, stream, static_cast<const uint64_t*>(chunk_starts),
                           shard_orders, count, S, tiles, sums, mismatch);
        status = hipGetLastError();
        if (status != hipSuccess) return status;
        const size_t bins = size_t(S) * tiles;
        status = launch_exclusive_scan(sums, bins, sums + bins, stream);
        if (status != hipSuccess) return status;
        hipLaunchKernelGGL(shard_tile_apply_kernel, grid, dim3(kMapTile), lds, stream, static_cast<const uint64_t*>(chunk_starts),
                           shard_orders, count, S, tiles, static_cast<const uint32_t*>(sums), total_chunks, chunk_shard, chunk_index,
                           row_chunk);
        status = hipGetLastError();
        if (status != hipSuccess) return status;
    }
    hipLaunchKernelGGL(shard_row_starts_kernel, dim3(launch_grid::exact_grid(S + 1, kThreads)), dim3(kThreads), 0, stream,
                       static_cast<const uint64_t*>(chunk_starts), count, S, tiles, static_cast<const uint32_t*>(sums), total_chunks,
                       shard_row_starts, mismatch);
    return hipGetLastError();
}

hipError_t launch_simple_pir_shard_scatter(const uint8_t* values, uint64_t values_bytes, const uint64_t* value_offsets,
                                           const SimplePirShardMapView& map, Form form, uint8_t* shards, hipStream_t stream) {
    if (form == Form::kNone) return hipSuccess;
    const uint64_t pieces = map.total_chunks * map.chunk_size / simple_pir_shard::piece_bytes(form);
    return for_each_launch(pieces, [&](dim3 grid, uint64_t first) {
        if (form == Form::kWide)
            hipLaunchKernelGGL(shard_scatter_kernel<16>, grid, dim3(kThreads), 0, stream, values, values_bytes, value_offsets, map,
                               shards, first, pieces);
        else if (form == Form::kWord)
            hipLaunchKernelGGL(shard_scatter_kernel<8>, grid, dim3(kThreads), 0, stream, values, values_bytes, value_offsets, map,
                               shards, first, pieces);
        else
            hipLaunchKernelGGL(shard_scatter_kernel<1>, grid, dim3(kThreads), 0, stream, values, values_bytes, value_offsets, map,
                               shards, first, pieces);
    });
}

hipError_t launch_simple_pir_shard_query_indices(const uint64_t* entry_positions, uint64_t batch, const SimplePirShardMapView& map,
                                                 uint64_t maximum_chunk_count, uint64_t chunks_per_shard, uint64_t* out_indices,
                                                 uint32_t* out_found, hipStream_t stream) {
    if (batch == 0) return hipSuccess;
    const uint64_t lanes = map.shard_count * batch * chunks_per_shard;
    const uint64_t grid_lanes = lanes > batch ? lanes : batch;
    if (!launch_grid::launch_fits(launch_grid::grid_blocks(grid_lanes, kThreads, SIZE_MAX), kThreads))
        return hipErrorInvalidConfiguration;
    hipLaunchKernelGGL(shard_query_indices_kernel, dim3(launch_grid::exact_grid(grid_lanes, kThreads)), dim3(kThreads), 0, stream,
                       entry_positions, batch, map, maximum_chunk_count, chunks_per_shard ? chunks_per_shard : 1, lanes, out_indices,
                       out_found);
    return hipGetLastError();
}

hipError_t launch_simple_pir_shard_assemble(const uint8_t* chunks, const uint64_t* indices, const uint64_t* entry_positions,
                                            uint64_t batch, const uint64_t* value_offsets, const SimplePirShardMapView& map,
                                            uint64_t maximum_chunk_count, uint64_t chunks_per_shard, Form form, uint8_t* out_entries,
                                            uint64_t* out_sizes, uint32_t* out_found, hipStream_t stream) {
    if (batch == 0) return hipSuccess;
    const uint32_t width = simple_pir_shard::piece_bytes(form);
    const uint64_t pieces = width != 0 ? batch * maximum_chunk_count * map.chunk_size / width : 0;
    const uint64_t grid_lanes = pieces > batch ? pieces : batch;
    if (!launch_grid::launch_fits(launch_grid::grid_blocks(grid_lanes, kThreads, SIZE_MAX), kThreads))
        return hipErrorInvalidConfiguration;
    const dim3 grid(launch_grid::exact_grid(grid_lanes, kThreads));
    if (form == Form::kWide)
        hipLaunchKernelGGL(shard_assemble_kernel<16>, grid, dim3(kThreads), 0, stream, chunks, indices, entry_positions, batch,
                           value_offsets, map, maximum_chunk_count, chunks_per_shard, pieces, out_entries, out_sizes, out_found);
    else if (form == Form::kWord)
        hipLaunchKernelGGL(shard_assemble_kernel<8>, grid, dim3(kThreads), 0, stream, chunks, indices, entry_positions, batch,
                           value_offsets, map, maximum_chunk_count, chunks_per_shard, pieces, out_entries, out_sizes, out_found);
    else
        hipLaunchKernelGGL(shard_assemble_kernel<1>, grid, dim3(kThreads), 0, stream, chunks, indices, entry_positions, batch,
                           value_offsets, map, maximum_chunk_count, chunks_per_shard, pieces, out_entries, out_sizes, out_found);
    return hipGetLastError();
}

}  // namespace heamd
