// pir_database_file_kernels.hip -- the body of a ProcessedDatabase file <-> the [count][L][N] Eval database and its present
// mask (gfx950).
//
// Reference: ProcessedDatabase.serialize() / init(from:context:) (PrivateInformationRetrieval/IndexPir/IndexPirProtocol.swift:
// 302-334, 362-378).  After the 5-byte header the file holds, per plaintext in array order, the tag byte 0
// (serializedZeroPlaintextTag, :258-260) and nothing else, or the tag byte 1 (serializedPlaintextTag, :263-265) followed by
// Plaintext<Eval>.serialize().poly: a bare PolyRq.serialize record over the top-level ciphertext context, skipLSBs 0, of S bytes
// (:317, :325-326, :371-372) -- per residue row a big-endian bit stream of N fields of ceilLog2(q_r) bits, zero-padded to a byte
// (CoefficientPacking.swift:169-213).  So the tag of plaintext i of a range lies at byte i + S rank(i) of the range, rank(i) the
// number of present plaintexts before i, and its payload right behind it: records abut without a gap, at every alignment.
//
//   ranks  an exclusive prefix count of the present bytes (any byte != 0 counts), 4 bytes per plaintext and the total behind
//          them: one workgroup walks the mask 1024 bytes a trip, a ballot per wave and 16 wave totals through the LDS;
//   load   the "field" form of ciphertext_wire_kernels.hip: a lane owns one coefficient and shifts its field out of the one or
//          two aligned 8-byte words around it, a word that reaches outside [records, records + records_bytes) gathered byte by
//          byte with what lies outside read as zero; the lanes of a nil plaintext store zero;
//   save   the "chunk" form: a lane owns one aligned 8-byte chunk of a present plaintext's payload -- one 8-byte store where
//          the chunk lies inside the payload, byte stores of exactly the payload's bytes where it holds its first or last ones
//          (the rest of such a chunk is a tag and a neighbour's payload: other lanes' bytes, neither read nor written here);
//          the lane of a plaintext's chunk 0 stores its tag.  No byte at or past records_bytes is written.
// Both report through an optional device word: bit 0 when the range needs more than records_bytes, bit 1 (load) when a tag byte
// differs from what the mask says.
#include <hip/hip_runtime.h>

#include "ciphertext_wire_form.hpp"
#include "kernels.hpp"
#include "launch_grid.hpp"
#include "wire_stream.hpp"

namespace heamd {

namespace {

using namespace wire_stream;

constexpr uint32_t kRankLanes = 1024;

__global__ void __launch_bounds__(kRankLanes)
    present_ranks_kernel(const uint8_t* __restrict__ present, size_t count, uint32_t* __restrict__ ranks) {
    __shared__ uint32_t wave_total[kRankLanes / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0;  // present plaintexts before this trip's 1024 (the same in every lane)
    for (size_t trip = 0; trip < count; trip += kRankLanes) {
        const size_t i = trip + threadIdx.x;
        const bool here = i < count && present[i] != 0;
        const uint64_t mask = __ballot(here);
        if (lane == 0) wave_total[wave] = static_cast<uint32_t>(__popcll(mask));
        __syncthreads();
        uint32_t below = 0, all = 0;
        for (uint32_t v = 0; v < kRankLanes / 64; ++v) {
            const uint32_t t = wave_total[v];
            below += v < wave ? t : 0;
            all += t;
        }
        if (i < count) ranks[i] = carry + below + static_cast<uint32_t>(__popcll(mask & ((uint64_t(1) << lane) - 1)));
        carry += all;
        __syncthreads();  // wave_total is rewritten by the next trip
    }
    if (threadIdx.x == 0) ranks[count] = carry;
}

template <typename W>
__global__ void __launch_bounds__(256)
    database_load_kernel(const uint8_t* __restrict__ records, uint64_t records_bytes, const uint8_t* __restrict__ present,
                         const uint32_t* __restrict__ ranks, size_t first, W* __restrict__ database,
                         const CiphertextWireLayout layout, uint32_t logn, size_t total, uint32_t* __restrict__ mismatch) {
    const uint32_t n = 1u << logn, rows = layout.rows;
    const uint64_t payload_bytes = layout.byte_offset[rows];
    const size_t idx = blockIdx.x * size_t(256) + threadIdx.x;  // one coefficient per lane (launch_grid::exact_grid)
    if (idx < total) {
        const size_t row_index = idx >> logn;
        const uint32_t k = static_cast<uint32_t>(idx) & (n - 1);
        const size_t local = row_index / rows;
        const uint32_t f = static_cast<uint32_t>(row_index - local * rows);
        const size_t p = first + local;
        const bool here = present[p] != 0;
        const uint64_t tag_at = p + payload_bytes * ranks[p];
        if (f == 0 && k == 0 && mismatch != nullptr) {
            // the reference reads tag and payload from the buffer and traps past its end; a kernel cannot
            if (tag_at + 1 + (here ? payload_bytes : 0) > records_bytes) atomicOr(mismatch, 1u);
            else if (records[tag_at] != (here ? 1 : 0)) atomicOr(mismatch, 2u);
        }
        uint64_t value = 0;
        if (here)
            value = load_stream_field(records + tag_at + 1 + layout.byte_offset[f], k, layout.width[f], records,
                                      records + records_bytes);
        database[((p * rows + f) << logn) + k] = static_cast<W>(value);
    }
}

template <typename W>
__global__ void __launch_bounds__(256)
    database_save_kernel(const W* __restrict__ database, const uint8_t* __restrict__ present,
                         const uint32_t* __restrict__ ranks, size_t first, uint8_t* __restrict__ records,
                         uint64_t records_bytes, const CiphertextWireLayout layout, uint32_t logn, uint64_t chunks_per_record,
                         size_t total, uint32_t* __restrict__ mismatch) {
    const uint32_t n = 1u << logn, rows = layout.rows;
    const uint64_t payload_bytes = layout.byte_offset[rows];
    const size_t idx = blockIdx.x * size_t(256) + threadIdx.x;  // one chunk per lane (launch_grid::exact_grid)
    if (idx < total) {
        const size_t local = idx / chunks_per_record;
        const uint64_t chunk = idx - local * chunks_per_record;
        const size_t p = first + local;
        const bool here = present[p] != 0;
        const uint64_t tag_at = p + payload_bytes * ranks[p];
        if (chunk == 0) {
            if (tag_at < records_bytes) records[tag_at] = here ? 1 : 0;
            if (mismatch != nullptr && tag_at + 1 + (here ? payload_bytes : 0) > records_bytes) atomicOr(mismatch, 1u);
        }
        if (!here || tag_at + 1 >= records_bytes) return;
        // the payload, cut where the buffer ends
        const uint64_t room = records_bytes - (tag_at + 1);
        const uint64_t record_bytes = payload_bytes < room ? payload_bytes : room;
        uint8_t* base = records + tag_at + 1;
        const uint64_t misaligned = reinterpret_cast<uintptr_t>(base) & 7;
        // aligned chunk `chunk` of this payload holds its bytes [8 chunk - misaligned, 8 chunk - misaligned + 8)
        const uint64_t begin = 8 * chunk < misaligned ? 0 : 8 * chunk - misaligned;
        uint64_t end = 8 * chunk + 8 - misaligned;
        if (end > record_bytes) end = record_bytes;
        if (begin >= end) return;  // the chunk lies past the payload's last byte
        uint64_t acc = 0, at = begin;  // the bytes [begin, at) so far, big-endian in the low bytes of acc
        uint32_t f = 0;
        while (at < end) {
            while (f + 1 < rows && at >= layout.byte_offset[f + 1]) ++f;
            const uint64_t row_end = layout.byte_offset[f + 1];
            const uint32_t take = static_cast<uint32_t>((end < row_end ? end : row_end) - at);  // 1 .. 8 bytes of row f
            const W* row = database + ((p * rows + f) << logn);
            const uint64_t piece = gather_row_bits(row, n, layout.width[f], 0, (at - layout.byte_offset[f]) * 8, 8 * take);
            acc = take == 8 ? piece : ((acc << (8 * take)) | piece);
            at += take;
        }
        const uint32_t held = static_cast<uint32_t>(end - begin);
        if (held == 8) {
            *reinterpret_cast<uint64_t*>(base + begin) = wire_byte_swap64(acc);  // base + begin is the aligned chunk
        } else {
            for (uint32_t b = 0; b < held; ++b) base[begin + b] = static_cast<uint8_t>(acc >> (8 * (held - 1 - b)));
        }
    }
}

// whole plaintexts whose lanes fit one launch of 256-lane workgroups (0: a single plaintext does not)
inline size_t plaintexts_per_launch(uint64_t items_per_plaintext) {
    const size_t lanes = launch_grid::max_blocks(256) * size_t(256);
    return items_per_plaintext == 0 ? 0 : static_cast<size_t>(lanes / items_per_plaintext);
}

}  // namespace

hipError_t launch_pir_database_file_ranks(const uint8_t* present, size_t count, uint32_t* ranks, hipStream_t stream) {
    hipLaunchKernelGGL(present_ranks_kernel, dim3(1), dim3(kRankLanes), 0, stream, present, count, ranks);
    return hipGetLastError();
}

template <typename W>
hipError_t launch_pir_database_file_load(const uint8_t* records, uint64_t records_bytes, const uint8_t* present,
                                         const uint32_t* ranks, size_t count, W* database,
                                         const CiphertextWireLayout& layout, uint32_t log_degree, uint32_t* mismatch,
                                         hipStream_t stream) {
    if (count == 0 || layout.rows == 0) return hipSuccess;
    const uint64_t items = static_cast<uint64_t>(layout.rows) << log_degree;
    // every lane takes one coefficient: a call of more lanes than one launch holds goes out as runs of whole plaintexts
    const size_t most = plaintexts_per_launch(items);
    if (most == 0) return hipErrorInvalidValue;
    for (size_t first = 0; first < count; first += most) {
        const size_t now = count - first < most ? count - first : most, total = now * items;
        hipLaunchKernelGGL(database_load_kernel<W>, dim3(launch_grid::exact_grid(total, 256)), dim3(256), 0, stream, records,
                           records_bytes, present, ranks, first, database, layout, log_degree, total, mismatch);
        const hipError_t status = hipGetLastError();
        if (status != hipSuccess) return status;
    }
    return hipSuccess;
}

template <typename W>
hipError_t launch_pir_database_file_save(const W* database, const uint8_t* present, const uint32_t* ranks, size_t count,
                                         uint8_t* records, uint64_t records_bytes, const CiphertextWireLayout& layout,
                                         uint32_t log_degree, uint32_t* mismatch, hipStream_t stream) {
    if (count == 0) return hipSuccess;
    // (a payload of no bytes still has its tag: one lane per plaintext)
    const uint64_t items = ciphertext_wire_form::chunks_per_record(layout.byte_offset[layout.rows]);
    const size_t most = plaintexts_per_launch(items);
    if (most == 0) return hipErrorInvalidValue;
    for (size_t first = 0; first < count; first += most) {
        const size_t now = count - first < most ? count - first : most, total = now * items;
        hipLaunchKernelGGL(database_save_kernel<W>, dim3(launch_grid::exact_grid(total, 256)), dim3(256), 0, stream, database,
                           present, ranks, first, records, records_bytes, layout, log_degree, items, total, mismatch);
        const hipError_t status = hipGetLastError();
        if (status != hipSuccess) return status;
    }
    return hipSuccess;
}

#define HEAMD_INSTANTIATE_PIR_DATABASE_FILE(W)                                                                                \
    template hipError_t launch_pir_database_file_load<W>(const uint8_t*, uint64_t, const uint8_t*, const uint32_t*, size_t,   \
                                                         W*, const CiphertextWireLayout&, uint32_t, uint32_t*, hipStream_t);  \
    template hipError_t launch_pir_database_file_save<W>(const W*, const uint8_t*, const uint32_t*, size_t, uint8_t*,         \
                                                         uint64_t, const CiphertextWireLayout&, uint32_t, uint32_t*,          \
                                                         hipStream_t);
HEAMD_INSTANTIATE_PIR_DATABASE_FILE(uint64_t)
HEAMD_INSTANTIATE_PIR_DATABASE_FILE(uint32_t)
#undef HEAMD_INSTANTIATE_PIR_DATABASE_FILE

}  // namespace heamd
