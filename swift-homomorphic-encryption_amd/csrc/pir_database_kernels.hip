// pir_database_kernels.hip -- MulPirServer.process (reference Sources/PrivateInformationRetrieval/IndexPir/MulPir.swift:
// 431-556) on the device, the part that decides which bytes go into which plaintext slot: one workgroup per database slot
// gathers the slot's bytes from the raw entries (size prefix, entry bytes up to the entry's own size, zeros), unpacks them
// into N coefficients of floor(log2 t) bits (CoefficientPacking.bytesToCoefficients, CoefficientPacking.swift:59-136) and
// writes the slot's present byte.  The centred lift and forward NTT that follow are the existing Plaintext.convertToEvalFormat
// kernels (pir_database.cpp).
#include "launch_grid.hpp"
#include "pir_database.hpp"

namespace heamd {

namespace {

constexpr unsigned kUnpackThreads = 256;
// one workgroup per slot up to this many, grid-stride beyond: a launch stays far below the lane limit for any database size
constexpr size_t kUnpackGridCap = size_t(1) << 20;

// byte q of prefix(e) || entry_e || zeros (q < encoded): the prefix is the entry's size, little-endian (IndexPirProtocol.swift:
// 123-150); entry bytes at or past the entry's own size read as zero whatever the caller's buffer holds there
__device__ __forceinline__ uint32_t record_byte(const PirDatabaseLayout& l, uint64_t e, uint64_t q) {
    const uint64_t size = l.entry_sizes != nullptr ? l.entry_sizes[e] : l.entry_stride;
    if (q < l.width) return static_cast<uint32_t>(size >> (8 * q)) & 0xffu;
    q -= l.width;
    return q < size ? l.entries[e * l.entry_stride + q] : 0u;
}

template <typename W>
__global__ __launch_bounds__(kUnpackThreads) void pir_database_unpack_kernel(const PirDatabaseLayout l, size_t first_slot,
                                                                               size_t slots, W* __restrict__ staging,
                                                                               uint8_t* __restrict__ present) {
    const size_t n = size_t(1) << l.log_degree;
    const uint32_t bits = l.bits;
    for (size_t g = blockIdx.x; g < slots; g += gridDim.x) {  // wave-uniform: every lane of the block takes the same slots
        const uint64_t slot = first_slot + g;
        const uint64_t chunk = slot / l.per_chunk, s = slot - chunk * l.per_chunk;
        const uint64_t j = (s % l.d0) * l.columns + s / l.d0;
        // the slot's bytes: [begin, end) of record `record` (split) or of F (pack); empty for a padding plaintext
        uint64_t begin = 0, end = 0, record = 0;
        if (l.packed_bytes == 0) {
            if (j < l.entry_count) {
                record = j;
                const uint64_t size = l.entry_sizes != nullptr ? l.entry_sizes[j] : l.entry_stride;
                begin = chunk * l.bytes_per_plaintext;
                end = min(begin + l.bytes_per_plaintext, l.width + size);
            }
        } else if (j < l.plaintexts) {
            begin = j * l.packed_bytes;
            end = min(begin + l.packed_bytes, l.entry_count * l.encoded);
        }
        const uint64_t length_bits = end > begin ? (end - begin) * 8 : 0;
        uint64_t any = 0;
        for (size_t i = threadIdx.x; i < n; i += kUnpackThreads) {
            // coefficient i is bits [i b, (i + 1) b) of the slot's bytes read as one big-endian bit string, zero-extended
            const uint64_t first_bit = uint64_t(i) * bits;
            uint64_t value = 0;
            if (first_bit < length_bits) {
                const uint64_t last_bit = first_bit + bits;
                uint64_t byte_index = begin + (first_bit >> 3);
                // pack mode: the record and the offset inside it of the first byte, stepped byte by byte from there
                uint64_t e = record, q = byte_index;
                if (l.packed_bytes != 0) {
                    e = byte_index / l.encoded;
                    q = byte_index - e * l.encoded;
                }
                for (uint64_t bit = first_bit; bit < last_bit;) {
                    const uint32_t byte = bit < length_bits ? record_byte(l, e, q) : 0u;
                    const uint32_t skip = static_cast<uint32_t>(bit & 7);
                    const uint32_t take = static_cast<uint32_t>(min(uint64_t(8 - skip), last_bit - bit));
                    value = (value << take) | ((byte >> (8 - skip - take)) & ((1u << take) - 1u));
                    bit += take;
                    if (++q == l.encoded && l.packed_bytes != 0) {
                        q = 0;
                        ++e;
                    }
                }
            }
            staging[g * n + i] = static_cast<W>(value);
            any |= value;
        }
        // all coefficients zero exactly when all of the slot's bytes are: the reference's nil plaintext
        const int nonzero = __syncthreads_or(any != 0);
        if (threadIdx.x == 0) present[slot] = nonzero ? 1 : 0;
    }
}

}  // namespace

template <typename W>
hipError_t launch_pir_database_unpack(const PirDatabaseLayout& layout, size_t first_slot, size_t slots, W* staging,
                                      uint8_t* present, hipStream_t stream) {
    if (slots == 0) return hipSuccess;
    const unsigned grid = launch_grid::grid_for_blocks(slots, kUnpackThreads, kUnpackGridCap);
    hipLaunchKernelGGL(pir_database_unpack_kernel<W>, dim3(grid), dim3(kUnpackThreads), 0, stream, layout, first_slot, slots,
                       staging, present);
    return hipGetLastError();
}
template hipError_t launch_pir_database_unpack<uint64_t>(const PirDatabaseLayout&, size_t, size_t, uint64_t*, uint8_t*,
                                                         hipStream_t);
template hipError_t launch_pir_database_unpack<uint32_t>(const PirDatabaseLayout&, size_t, size_t, uint32_t*, uint8_t*,
                                                         hipStream_t);

}  // namespace heamd
