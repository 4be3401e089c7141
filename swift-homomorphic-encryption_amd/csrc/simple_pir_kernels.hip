// simple_pir_kernels.hip -- SimplePirServer (reference Sources/PrivateInformationRetrieval/SimplePir/) on the device.
//
// The database is the reference's transposed processedDatabase, [column_size][database_columns] row-major, but each element
// is stored in the narrowest of 1 / 2 / 4 / 8 bytes that holds plaintext_bits (the reference keeps a whole Scalar): the reply
// streams the database once, so its bytes are the reply's time.
//
//   simple_pir_database_kernel   process (SimplePir+Database.swift:252-275): entry bytes -> narrow elements
//   simple_pir_widen_kernel      narrow rows -> zero-padded blocks of N 8-byte coefficients (what the forward NTT takes)
//   simple_pir_hint_mac_kernel   hint row r = sum_k NTT(d_{r,k}) * NTT(sigma(a_k)), lazily accumulated in 128 bits
//   simple_pir_pack / unpack     the reference's wide Array2d<Scalar> image <-> the narrow layout
//   simple_pir_response_kernel   computeResponse (SimplePir+Server.swift:31-38, SimplePir+Precompute.swift:51-114)
#include "device_math.hpp"
#include "kernels.hpp"
#include "launch_grid.hpp"

namespace heamd {

namespace {

constexpr unsigned kFlatThreads = 256;
// at most 2^20 workgroups, grid-stride beyond: no launch nears the lane limit
inline unsigned flat_grid(size_t items) { return launch_grid::grid_for(items, kFlatThreads, size_t(1) << 20); }

// element (r, c) of the transposed database: flat index f = c * column_size + r of the reference's untransposed array, which
// holds entry e = f / padded at offset o = f % padded; coefficient o of an entry is bits [o b, (o + 1) b) of its bytes read
// as one big-endian bit string, zero-extended (CoefficientPacking.bytesToCoefficients, decode: false)
template <typename E>
__global__ __launch_bounds__(kFlatThreads) void simple_pir_database_kernel(const SimplePirLayout l,
                                                                            const uint8_t* __restrict__ entries,
                                                                            E* __restrict__ database) {
    const size_t total = l.column_size * l.database_columns;
    const size_t stride = static_cast<size_t>(gridDim.x) * kFlatThreads;
    for (size_t index = static_cast<size_t>(blockIdx.x) * kFlatThreads + threadIdx.x; index < total; index += stride) {
        const size_t r = index / l.database_columns, c = index - r * l.database_columns;
        const size_t f = c * l.column_size + r;
        const size_t e = f / l.padded_entry_size, o = f - e * l.padded_entry_size;
        uint64_t value = 0;
        if (e < l.entry_count && o < l.entry_size_in_scalar) {
            const uint8_t* entry = entries + e * l.entry_size_in_bytes;
            const uint64_t length_bits = l.entry_size_in_bytes * 8, last_bit = (o + 1) * l.plaintext_bits;
            for (uint64_t bit = o * l.plaintext_bits; bit < last_bit;) {
                const uint32_t byte = bit < length_bits ? entry[bit >> 3] : 0u;
                const uint32_t skip = static_cast<uint32_t>(bit & 7);
                const uint32_t take = static_cast<uint32_t>(min(uint64_t(8 - skip), last_bit - bit));
                value = (value << take) | ((byte >> (8 - skip - take)) & ((1u << take) - 1u));
                bit += take;
            }
        }
        database[index] = static_cast<E>(value);
    }
}

// staging [rows][blocks][N]: block k of row r is columns [k N, (k + 1) N) of database row first_row + r, zeros past the end
template <typename E>
__global__ __launch_bounds__(kFlatThreads) void simple_pir_widen_kernel(const E* __restrict__ database, size_t columns,
                                                                         size_t first_row, size_t rows, uint32_t blocks,
                                                                         uint32_t log_degree, uint64_t* __restrict__ staging) {
    const size_t padded = static_cast<size_t>(blocks) << log_degree, total = rows * padded;
    const size_t stride = static_cast<size_t>(gridDim.x) * kFlatThreads;
    for (size_t index = static_cast<size_t>(blockIdx.x) * kFlatThreads + threadIdx.x; index < total; index += stride) {
        const size_t r = index / padded, c = index - r * padded;
        staging[index] = c < columns ? static_cast<uint64_t>(database[(first_row + r) * columns + c]) : 0;
    }
}

// out [rows][N] = sum_k staging[row][k][.] * a_eval[k][.] mod p (Eval form, canonical operands); the 128-bit sum is reduced
// every `cadence` products: the caller passes PolyContext.maxLazyProductAccumulationCount - 1, because the sum restarts from a
// reduced word below p instead of zero (cadence (p - 1)^2 + p - 1 < 2^128)
__global__ __launch_bounds__(kFlatThreads) void simple_pir_hint_mac_kernel(const uint64_t* __restrict__ staging,
                                                                            const uint64_t* __restrict__ a_eval,
                                                                            uint64_t* __restrict__ out, size_t rows,
                                                                            uint32_t blocks, uint32_t log_degree,
                                                                            uint64_t cadence, const DeviceModulus* moduli) {
    const DeviceModulus m = moduli[0];
    const size_t n = size_t(1) << log_degree, total = rows << log_degree;
    const size_t stride = static_cast<size_t>(gridDim.x) * kFlatThreads;
    for (size_t index = static_cast<size_t>(blockIdx.x) * kFlatThreads + threadIdx.x; index < total; index += stride) {
        const size_t r = index >> log_degree, i = index & (n - 1);
        const uint64_t* row = staging + ((r * blocks) << log_degree) + i;
        U128 acc{0, 0};
        uint64_t pending = 0;
        for (uint32_t k = 0; k < blocks; ++k) {
            mac128(acc, stream_load(row + (static_cast<size_t>(k) << log_degree)), a_eval[(static_cast<size_t>(k) << log_degree) + i]);
            if (++pending == cadence) {
                acc = U128{barrett_reduce128(acc, m.p, m.barrett128_lo, m.barrett128_hi), 0};
                pending = 0;
            }
        }
        out[index] = barrett_reduce128(acc, m.p, m.barrett128_lo, m.barrett128_hi);
    }
}

__global__ void simple_pir_replicate_modulus_kernel(const DeviceModulus* moduli, DeviceModulus* out, uint32_t count) {
    for (uint32_t k = threadIdx.x; k < count; k += blockDim.x) out[k] = moduli[0];
}

template <typename W, typename E>
__global__ __launch_bounds__(kFlatThreads) void simple_pir_pack_kernel(const W* __restrict__ wide, E* __restrict__ database,
                                                                        size_t elements, uint64_t mask) {
    const size_t stride = static_cast<size_t>(gridDim.x) * kFlatThreads;
    for (size_t index = static_cast<size_t>(blockIdx.x) * kFlatThreads + threadIdx.x; index < elements; index += stride)
        database[index] = static_cast<E>(static_cast<uint64_t>(wide[index]) & mask);
}

template <typename W, typename E>
__global__ __launch_bounds__(kFlatThreads) void simple_pir_unpack_kernel(const E* __restrict__ database, W* __restrict__ wide,
                                                                          size_t elements) {
    const size_t stride = static_cast<size_t>(gridDim.x) * kFlatThreads;
    for (size_t index = static_cast<size_t>(blockIdx.x) * kFlatThreads + threadIdx.x; index < elements; index += stride)
        wide[index] = static_cast<W>(database[index]);
}

// ---- computeResponse ---------------------------------------------------------------------------------------------------
// responses[q][r] = (sum_c database[r][c] * requests[q][c]) & mask.  The mask comes last and ciphertext_bits fits the word,
// so the sum wraps in the word and may be formed in any order.
//
// A workgroup of four wavefronts owns kBlockRows = 64 database rows and walks the columns in tiles of kTileColumns.  Per tile
// it stages the QT requests' slice in LDS once; then every group of 16 lanes reads 16 bytes per lane of each of its kLaneRows
// rows (256 contiguous bytes of a row per group, non-temporal: the database is read once) and multiplies them with the staged
// request words, each LDS word serving kLaneRows products.  A lane's partial sums stay in its registers over the whole row;
// the 16 lanes of a group are summed once, at the end.  The slice is staged element-major within a group's span
// ([element of the lane's 16 bytes][lane]) so that the 16 lanes read consecutive LDS words.
constexpr unsigned kResponseThreads = 256, kGroupLanes = 16, kLaneRows = 4;
constexpr unsigned kBlockRows = (kResponseThreads / kGroupLanes) * kLaneRows;  // 64
constexpr unsigned kTileColumns = 512;

typedef uint32_t Chunk16 __attribute__((ext_vector_type(4)));

template <typename E>
__device__ __forceinline__ uint32_t chunk_element(const Chunk16& v, unsigned e);
template <>
__device__ __forceinline__ uint32_t chunk_element<uint8_t>(const Chunk16& v, unsigned e) {
    return (v[e >> 2] >> (8 * (e & 3))) & 0xffu;
}
template <>
__device__ __forceinline__ uint32_t chunk_element<uint16_t>(const Chunk16& v, unsigned e) {
    return (v[e >> 1] >> (16 * (e & 1))) & 0xffffu;
}
template <>
__device__ __forceinline__ uint32_t chunk_element<uint32_t>(const Chunk16& v, unsigned e) {
    return v[e];
}

template <typename W, typename E, unsigned QT>
__global__ __launch_bounds__(kResponseThreads) void simple_pir_response_kernel(const E* __restrict__ database, size_t rows,
                                                                                size_t columns,
                                                                                const W* __restrict__ requests,
                                                                                unsigned live_queries, W* __restrict__ responses,
                                                                                W mask) {
    constexpr unsigned kPerLane = 16 / sizeof(E);               // elements in a lane's 16 bytes
    constexpr unsigned kSpan = kGroupLanes * kPerLane;          // columns a group covers per load
    constexpr unsigned kSteps = kTileColumns / kSpan;
    __shared__ W slice[QT][kTileColumns];
    const unsigned lane = threadIdx.x & (kGroupLanes - 1), group = threadIdx.x / kGroupLanes;
    const size_t first_row = static_cast<size_t>(blockIdx.x) * kBlockRows + group * kLaneRows;
    // 16-byte loads need 16-byte rows; any other column count takes the element-wise path (wave-uniform choice)
    const bool aligned = (columns * sizeof(E)) % 16 == 0 && (reinterpret_cast<uintptr_t>(database) & 15u) == 0;
    W acc[kLaneRows][QT];
#pragma unroll
    for (unsigned j = 0; j < kLaneRows; ++j)
#pragma unroll
        for (unsigned q = 0; q < QT; ++q) acc[j][q] = 0;

    for (size_t tile = 0; tile < columns; tile += kTileColumns) {
        __syncthreads();  // the previous tile's readers are done
        for (unsigned t = threadIdx.x; t < QT * kTileColumns; t += kResponseThreads) {
            const unsigned q = t / kTileColumns, c = t - q * kTileColumns;
            const size_t column = tile + c;
            const W word = (q < live_queries && column < columns) ? requests[q * columns + column] : W(0);
            const unsigned step = c / kSpan, in_span = c - step * kSpan;
            // (consecutive threads store kGroupLanes words apart: a bank-conflicted write, once per tile and request word,
            // against kBlockRows products per word read back)
            slice[q][step * kSpan + (in_span % kPerLane) * kGroupLanes + in_span / kPerLane] = word;
        }
        __syncthreads();
#pragma unroll 2
        for (unsigned step = 0; step < kSteps; ++step) {
            const size_t column = tile + step * kSpan + lane * kPerLane;
            if constexpr (sizeof(E) == 8) {
                uint64_t d[kLaneRows][kPerLane];
#pragma unroll
                for (unsigned j = 0; j < kLaneRows; ++j) {
                    const size_t r = first_row + j;
#pragma unroll
                    for (unsigned e = 0; e < kPerLane; ++e)
                        d[j][e] = (r < rows && column + e < columns) ? stream_load(database + r * columns + column + e) : 0;
                }
#pragma unroll
                for (unsigned e = 0; e < kPerLane; ++e)
#pragma unroll
                    for (unsigned q = 0; q < QT; ++q) {
                        const W x = slice[q][step * kSpan + e * kGroupLanes + lane];
#pragma unroll
                        for (unsigned j = 0; j < kLaneRows; ++j) acc[j][q] += static_cast<W>(d[j][e]) * x;
                    }
            } else {
                Chunk16 d[kLaneRows];
#pragma unroll
                for (unsigned j = 0; j < kLaneRows; ++j) {
                    const size_t r = first_row + j;
                    d[j] = Chunk16{0, 0, 0, 0};
                    if (r < rows && column < columns) {
                        const E* source = database + r * columns + column;
                        if (aligned) {
                            d[j] = __builtin_nontemporal_load(reinterpret_cast<const Chunk16*>(source));
                        } else {
#pragma unroll
                            for (unsigned e = 0; e < kPerLane; ++e) {
                                const uint32_t value = column + e < columns ? static_cast<uint32_t>(source[e]) : 0u;
                                d[j][e * sizeof(E) / 4] |= value << (8 * ((e * sizeof(E)) & 3));
                            }
                        }
                    }
                }
#pragma unroll
                for (unsigned e = 0; e < kPerLane; ++e)
#pragma unroll
                    for (unsigned q = 0; q < QT; ++q) {
                        const W x = slice[q][step * kSpan + e * kGroupLanes + lane];
#pragma unroll
                        for (unsigned j = 0; j < kLaneRows; ++j) acc[j][q] += static_cast<W>(chunk_element<E>(d[j], e)) * x;
                    }
            }
        }
    }
#pragma unroll
    for (unsigned j = 0; j < kLaneRows; ++j)
#pragma unroll
        for (unsigned q = 0; q < QT; ++q) {
            W sum = acc[j][q];
#pragma unroll
            for (unsigned offset = kGroupLanes / 2; offset != 0; offset >>= 1) sum += __shfl_xor(sum, offset, kGroupLanes);
            const size_t r = first_row + j;
            if (lane == 0 && r < rows && q < live_queries) responses[q * rows + r] = sum & mask;
        }
}

template <typename W, typename E, unsigned QT>
hipError_t response_pass(const E* database, size_t rows, size_t columns, const W* requests, unsigned live, W* responses,
                         W mask, hipStream_t stream) {
    const size_t blocks = (rows + kBlockRows - 1) / kBlockRows;
    if (!launch_grid::launch_fits(blocks, kResponseThreads)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((simple_pir_response_kernel<W, E, QT>), dim3(static_cast<unsigned>(blocks)), dim3(kResponseThreads), 0,
                       stream, database, rows, columns, requests, live, responses, mask);
    return hipGetLastError();
}

template <typename W, typename E>
hipError_t response_typed(const E* database, size_t rows, size_t columns, const W* requests, size_t query_count, W* responses,
                          W mask, hipStream_t stream) {
    // passes of 8 requests; the last pass takes the smallest tile that holds what is left (its spare slots multiply zeros)
    for (size_t q = 0; q < query_count;) {
        const size_t left = query_count - q;
        const unsigned live = static_cast<unsigned>(left < 8 ? left : 8);
        const W* req = requests + q * columns;
        W* out = responses + q * rows;
        hipError_t status;
        if (live > 4) status = response_pass<W, E, 8>(database, rows, columns, req, live, out, mask, stream);
        else if (live > 2) status = response_pass<W, E, 4>(database, rows, columns, req, live, out, mask, stream);
        else if (live > 1) status = response_pass<W, E, 2>(database, rows, columns, req, live, out, mask, stream);
        else status = response_pass<W, E, 1>(database, rows, columns, req, live, out, mask, stream);
        if (status != hipSuccess) return status;
        q += live;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_simple_pir_database(const SimplePirLayout& layout, const uint8_t* entries, void* database,
                                      hipStream_t stream) {
    const size_t total = layout.column_size * layout.database_columns;
    if (total == 0) return hipSuccess;
    const dim3 grid(flat_grid(total)), block(kFlatThreads);
    switch (layout.element_bytes) {
        case 1: hipLaunchKernelGGL(simple_pir_database_kernel<uint8_t>, grid, block, 0, stream, layout, entries, static_cast<uint8_t*>(database)); break;
        case 2: hipLaunchKernelGGL(simple_pir_database_kernel<uint16_t>, grid, block, 0, stream, layout, entries, static_cast<uint16_t*>(database)); break;
        case 4: hipLaunchKernelGGL(simple_pir_database_kernel<uint32_t>, grid, block, 0, stream, layout, entries, static_cast<uint32_t*>(database)); break;
        case 8: hipLaunchKernelGGL(simple_pir_database_kernel<uint64_t>, grid, block, 0, stream, layout, entries, static_cast<uint64_t*>(database)); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_simple_pir_widen(const void* database, uint32_t element_bytes, size_t columns, size_t first_row, size_t rows,
                                   uint32_t blocks, uint32_t log_degree, uint64_t* staging, hipStream_t stream) {
    const size_t total = (rows * blocks) << log_degree;
    if (total == 0) return hipSuccess;
    const dim3 grid(flat_grid(total)), block(kFlatThreads);
    switch (element_bytes) {
        case 1: hipLaunchKernelGGL(simple_pir_widen_kernel<uint8_t>, grid, block, 0, stream, static_cast<const uint8_t*>(database), columns, first_row, rows, blocks, log_degree, staging); break;
        case 2: hipLaunchKernelGGL(simple_pir_widen_kernel<uint16_t>, grid, block, 0, stream, static_cast<const uint16_t*>(database), columns, first_row, rows, blocks, log_degree, staging); break;
        case 4: hipLaunchKernelGGL(simple_pir_widen_kernel<uint32_t>, grid, block, 0, stream, static_cast<const uint32_t*>(database), columns, first_row, rows, blocks, log_degree, staging); break;
        case 8: hipLaunchKernelGGL(simple_pir_widen_kernel<uint64_t>, grid, block, 0, stream, static_cast<const uint64_t*>(database), columns, first_row, rows, blocks, log_degree, staging); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_simple_pir_hint_mac(const uint64_t* staging, const uint64_t* a_eval, uint64_t* out, size_t rows,
                                      uint32_t blocks, uint64_t cadence, const DeviceContext& ctx, hipStream_t stream) {
    const size_t total = rows << ctx.log_degree;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(simple_pir_hint_mac_kernel, dim3(flat_grid(total)), dim3(kFlatThreads), 0, stream, staging, a_eval, out,
                       rows, blocks, ctx.log_degree, cadence ? cadence : 1, ctx.moduli);
    return hipGetLastError();
}

hipError_t launch_simple_pir_replicate_modulus(const DeviceContext& ctx, DeviceModulus* out, uint32_t count,
                                               hipStream_t stream) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(simple_pir_replicate_modulus_kernel, dim3(1), dim3(64), 0, stream, ctx.moduli, out, count);
    return hipGetLastError();
}

template <typename W>
hipError_t launch_simple_pir_pack(const W* wide, void* database, uint32_t element_bytes, uint32_t plaintext_bits,
                                  size_t elements, hipStream_t stream) {
    if (elements == 0) return hipSuccess;
    const uint64_t mask = plaintext_bits >= 64 ? ~uint64_t(0) : (uint64_t(1) << plaintext_bits) - 1;
    const dim3 grid(flat_grid(elements)), block(kFlatThreads);
    switch (element_bytes) {
        case 1: hipLaunchKernelGGL((simple_pir_pack_kernel<W, uint8_t>), grid, block, 0, stream, wide, static_cast<uint8_t*>(database), elements, mask); break;
        case 2: hipLaunchKernelGGL((simple_pir_pack_kernel<W, uint16_t>), grid, block, 0, stream, wide, static_cast<uint16_t*>(database), elements, mask); break;
        case 4: hipLaunchKernelGGL((simple_pir_pack_kernel<W, uint32_t>), grid, block, 0, stream, wide, static_cast<uint32_t*>(database), elements, mask); break;
        case 8: hipLaunchKernelGGL((simple_pir_pack_kernel<W, uint64_t>), grid, block, 0, stream, wide, static_cast<uint64_t*>(database), elements, mask); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template hipError_t launch_simple_pir_pack<uint64_t>(const uint64_t*, void*, uint32_t, uint32_t, size_t, hipStream_t);
template hipError_t launch_simple_pir_pack<uint32_t>(const uint32_t*, void*, uint32_t, uint32_t, size_t, hipStream_t);

template <typename W>
hipError_t launch_simple_pir_unpack(const void* database, uint32_t element_bytes, W* wide, size_t elements,
                                    hipStream_t stream) {
    if (elements == 0) return hipSuccess;
    const dim3 grid(flat_grid(elements)), block(kFlatThreads);
    switch (element_bytes) {
        case 1: hipLaunchKernelGGL((simple_pir_unpack_kernel<W, uint8_t>), grid, block, 0, stream, static_cast<const uint8_t*>(database), wide, elements); break;
        case 2: hipLaunchKernelGGL((simple_pir_unpack_kernel<W, uint16_t>), grid, block, 0, stream, static_cast<const uint16_t*>(database), wide, elements); break;
        case 4: hipLaunchKernelGGL((simple_pir_unpack_kernel<W, uint32_t>), grid, block, 0, stream, static_cast<const uint32_t*>(database), wide, elements); break;
        case 8: hipLaunchKernelGGL((simple_pir_unpack_kernel<W, uint64_t>), grid, block, 0, stream, static_cast<const uint64_t*>(database), wide, elements); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
template hipError_t launch_simple_pir_unpack<uint64_t>(const void*, uint32_t, uint64_t*, size_t, hipStream_t);
template hipError_t launch_simple_pir_unpack<uint32_t>(const void*, uint32_t, uint32_t*, size_t, hipStream_t);

template <typename W>
hipError_t launch_simple_pir_response(const void* database, uint32_t element_bytes, size_t rows, size_t columns,
                                      const W* requests, size_t query_count, W* responses, uint32_t ciphertext_bits,
                                      hipStream_t stream) {
    if (rows == 0 || query_count == 0) return hipSuccess;
    const W mask = ciphertext_bits >= 8 * sizeof(W) ? ~W(0) : static_cast<W>((W(1) << ciphertext_bits) - 1);
    switch (element_bytes) {
        case 1: return response_typed<W, uint8_t>(static_cast<const uint8_t*>(database), rows, columns, requests, query_count, responses, mask, stream);
        case 2: return response_typed<W, uint16_t>(static_cast<const uint16_t*>(database), rows, columns, requests, query_count, responses, mask, stream);
        case 4: return response_typed<W, uint32_t>(static_cast<const uint32_t*>(database), rows, columns, requests, query_count, responses, mask, stream);
        case 8:
            if constexpr (sizeof(W) == 8)
                return response_typed<W, uint64_t>(static_cast<const uint64_t*>(database), rows, columns, requests, query_count, responses, mask, stream);
            return hipErrorInvalidValue;
        default: return hipErrorInvalidValue;
    }
}
template hipError_t launch_simple_pir_response<uint64_t>(const void*, uint32_t, size_t, size_t, const uint64_t*, size_t,
                                                         uint64_t*, uint32_t, hipStream_t);
template hipError_t launch_simple_pir_response<uint32_t>(const void*, uint32_t, size_t, size_t, const uint32_t*, size_t,
                                                         uint32_t*, uint32_t, hipStream_t);

}  // namespace heamd
