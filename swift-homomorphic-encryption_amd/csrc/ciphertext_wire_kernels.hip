// ciphertext_wire_kernels.hip -- whole ciphertexts <-> the reference's wire records, `count` of them per launch (gfx950).
//
// Reference: Ciphertext.serialize(forDecryption:) / Ciphertext(deserialize:) (SerializedCiphertext.swift:53-63,126-147) over
// Serialize.serializePolys / deserializePolys (Serialize.swift:31-94): a record is the polynomial count as a little-endian
// UInt16 followed by PolyRq.serialize(skipLSBs[p]) of each polynomial -- per residue row a big-endian bit stream of N fields of
// ceilLog2(q_r) - skipLSBs[p] bits (the value shifted right by skipLSBs[p]), zero-padded to a byte (CoefficientPacking.swift:
// 169-213, PolyRq/PolyRq+Serialize.swift:69-99).  Bfv.skipLSBsForDecryption gives the polynomials of a reply different skips,
// so the widths differ per (polynomial, row) and nothing after the header keeps an alignment: polynomial p + 1 starts where
// the bytes of polynomial p end, and records lie at any stride.  Each direction therefore has one kernel that holds for every
// address (ciphertext_wire_form.hpp):
//   serialize    a lane owns one aligned 8-byte chunk of the records buffer: coalesced 8-byte stores wherever the chunk lies
//                inside its record, byte stores where it holds the record's first or last bytes (the rest of such a chunk is
//                the caller's stride gap or a neighbouring record's lanes': it is neither read nor written here);
//   deserialize  a lane owns one coefficient and shifts its field out of the two aligned 8-byte words around it; a word that
//                reaches outside the records buffer is gathered byte by byte, what lies outside reading as zero.
// A layout without a header (byte_offset[0] == 0, one polynomial) is a bare PolyRq record: the seeded ciphertexts' poly0.
#include <hip/hip_runtime.h>

#include "ciphertext_wire_form.hpp"
#include "kernels.hpp"
#include "launch_grid.hpp"
#include "wire_stream.hpp"

namespace heamd {

namespace {

using namespace wire_stream;  // gather_row_bits, load_stream_field, wire_byte_swap64

template <typename W>
__global__ void __launch_bounds__(256)
    ciphertexts_serialize_kernel(const W* __restrict__ slab, size_t ct_words, uint8_t* __restrict__ records, size_t stride,
                                 const CiphertextWireLayout layout, uint32_t logn, uint64_t chunks_per_record,
                                 size_t total_chunks) {
    const uint32_t n = 1u << logn, flat_rows = layout.polys * layout.rows;
    const uint64_t header = layout.byte_offset[0], record_bytes = layout.byte_offset[flat_rows];
    const size_t idx = blockIdx.x * size_t(256) + threadIdx.x;  // one chunk per lane (launch_grid::exact_grid)
    if (idx < total_chunks) {
        const size_t record = idx / chunks_per_record;
        const uint64_t chunk = idx - record * chunks_per_record;
        uint8_t* base = records + record * stride;
        const uint64_t misaligned = reinterpret_cast<uintptr_t>(base) & 7;
        // aligned chunk `chunk` of this record holds its bytes [8 chunk - misaligned, 8 chunk - misaligned + 8)
        const uint64_t begin = 8 * chunk < misaligned ? 0 : 8 * chunk - misaligned;
        uint64_t end = 8 * chunk + 8 - misaligned;
        if (end > record_bytes) end = record_bytes;
        if (begin >= end) return;  // the chunk lies past the record's last byte
        uint64_t acc = 0, at = begin;  // the bytes [begin, at) so far, big-endian in the low bytes of acc
        for (; at < end && at < header; ++at) acc = (acc << 8) | (at == 0 ? layout.polys : 0);  // UInt16, little-endian
        uint32_t f = 0;
        while (at < end) {
            while (f + 1 < flat_rows && at >= layout.byte_offset[f + 1]) ++f;
            const uint64_t row_end = layout.byte_offset[f + 1];
            const uint32_t take = static_cast<uint32_t>((end < row_end ? end : row_end) - at);  // 1 .. 8 bytes of row f
            const W* row = slab + record * ct_words + (static_cast<size_t>(f) << logn);
            const uint64_t piece = gather_row_bits(row, n, layout.width[f], layout.skip[f / layout.rows],
                                                   (at - layout.byte_offset[f]) * 8, 8 * take);
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

template <typename W>
__global__ void __launch_bounds__(256)
    ciphertexts_deserialize_kernel(const uint8_t* __restrict__ records, size_t stride, W* __restrict__ slab, size_t ct_words,
                                   const CiphertextWireLayout layout, uint32_t logn, size_t count,
                                   uint32_t* __restrict__ mismatch) {
    const uint32_t n = 1u << logn, flat_rows = layout.polys * layout.rows;
    const uint64_t header = layout.byte_offset[0];
    const uint8_t* buffer_end = records + (count - 1) * stride + layout.byte_offset[flat_rows];
    const size_t total = (count * flat_rows) << logn;
    const size_t idx = blockIdx.x * size_t(256) + threadIdx.x;  // one coefficient per lane (launch_grid::exact_grid)
    if (idx < total) {
        const size_t row_index = idx >> logn;
        const uint32_t k = static_cast<uint32_t>(idx) & (n - 1);
        const size_t record = row_index / flat_rows;
        const uint32_t f = static_cast<uint32_t>(row_index - record * flat_rows);
        const uint8_t* base = records + record * stride;
        if (header != 0 && f == 0 && k == 0 && mismatch != nullptr) {
            // the reference takes the polynomial count from the buffer (Serialize.swift:70-94); a kernel cannot throw
            if ((uint32_t(base[0]) | (uint32_t(base[1]) << 8)) != layout.polys) *mismatch = 1;
        }
        const uint32_t w = layout.width[f], skip = layout.skip[f / layout.rows];
        const uint64_t field = load_stream_field(base + layout.byte_offset[f], k, w, records, buffer_end);
        slab[record * ct_words + (static_cast<size_t>(f) << logn) + k] = static_cast<W>(field << skip);
    }
}

// whole records whose lanes fit one launch of 256-lane workgroups (0: a single record does not)
inline size_t records_per_launch(uint64_t items_per_record) {
    const size_t lanes = launch_grid::max_blocks(256) * size_t(256);
    return items_per_record == 0 ? 0 : static_cast<size_t>(lanes / items_per_record);
}

}  // namespace

template <typename W>
hipError_t launch_ciphertexts_serialize(const W* slab, size_t ct_words, uint8_t* records, size_t record_stride,
                                        const CiphertextWireLayout& layout, uint32_t log_degree, size_t count,
                                        hipStream_t stream) {
    const uint64_t record_bytes = layout.byte_offset[layout.polys * layout.rows];
    if (count == 0 || record_bytes == 0) return hipSuccess;
    const ciphertext_wire_form::Plan plan =
        ciphertext_wire_form::for_serialize(record_bytes, record_stride, reinterpret_cast<uintptr_t>(records));
    // every lane takes one chunk: a call of more lanes than one launch holds goes out as runs of whole records
    const size_t most = records_per_launch(plan.items_per_record);
    if (most == 0) return hipErrorInvalidValue;
    for (size_t done = 0; done < count; done += most) {
        const size_t now = count - done < most ? count - done : most, total = now * plan.items_per_record;
        hipLaunchKernelGGL(ciphertexts_serialize_kernel<W>, dim3(launch_grid::exact_grid(total, 256)), dim3(256), 0, stream,
                           slab + done * ct_words, ct_words, records + done * record_stride, record_stride, layout, log_degree,
                           plan.items_per_record, total);
        const hipError_t status = hipGetLastError();
        if (status != hipSuccess) return status;
    }
    return hipSuccess;
}

template <typename W>
hipError_t launch_ciphertexts_deserialize(const uint8_t* records, size_t record_stride, W* slab, size_t ct_words,
                                          const CiphertextWireLayout& layout, uint32_t log_degree, size_t count,
                                          uint32_t* mismatch, hipStream_t stream) {
    if (count == 0 || layout.polys * layout.rows == 0) return hipSuccess;
    const ciphertext_wire_form::Plan plan = ciphertext_wire_form::for_deserialize(
        layout.polys, layout.rows, log_degree, record_stride, reinterpret_cast<uintptr_t>(records));
    const size_t most = records_per_launch(plan.items_per_record);
    if (most == 0) return hipErrorInvalidValue;
    for (size_t done = 0; done < count; done += most) {
        const size_t now = count - done < most ? count - done : most;
        hipLaunchKernelGGL(ciphertexts_deserialize_kernel<W>, dim3(launch_grid::exact_grid(now * plan.items_per_record, 256)),
                           dim3(256), 0, stream, records + done * record_stride, record_stride, slab + done * ct_words, ct_words,
                           layout, log_degree, now, mismatch);
        const hipError_t status = hipGetLastError();
        if (status != hipSuccess) return status;
    }
    return hipSuccess;
}

#define HEAMD_INSTANTIATE_CIPHERTEXT_WIRE(W)                                                                                  \
    template hipError_t launch_ciphertexts_serialize<W>(const W*, size_t, uint8_t*, size_t, const CiphertextWireLayout&,      \
                                                        uint32_t, size_t, hipStream_t);                                       \
    template hipError_t launch_ciphertexts_deserialize<W>(const uint8_t*, size_t, W*, size_t, const CiphertextWireLayout&,    \
                                                          uint32_t, size_t, uint32_t*, hipStream_t);
HEAMD_INSTANTIATE_CIPHERTEXT_WIRE(uint64_t)
HEAMD_INSTANTIATE_CIPHERTEXT_WIRE(uint32_t)
#undef HEAMD_INSTANTIATE_CIPHERTEXT_WIRE

}  // namespace heamd
