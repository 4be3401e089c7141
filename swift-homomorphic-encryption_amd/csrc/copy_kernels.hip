// copy_kernels.hip -- kernels that move words and compute nothing: the bridge between the two slab words (packed [UInt32]
// slabs <-> the 8-byte words of the Bfv<UInt32> scheme layer), the streaming copy that is the reference point of the
// transforms' roofline figures, and the strided record copy of the PIR tail.
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "kernels.hpp"
#include "launch_grid.hpp"

namespace heamd {

namespace {

constexpr unsigned kThreads = 256;

// one workgroup per kThreads work items, up to the grid limit (poly_kernels.hip says why)
inline unsigned grid_for(size_t work_items) { return launch_grid::grid_for(work_items, kThreads); }

// ---- word-size bridge between packed [UInt32] slabs and the 8-byte words of the Bfv<UInt32> scheme layer -------
// four words per lane: 16 B in / 32 B out (widen) or 32 B in / 16 B out (narrow); a narrowed word keeps its low half
// (scheme-layer results of a UInt32 context are < 2^30)
typedef uint32_t Packed4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(kThreads)
    widen_kernel(const uint32_t* __restrict__ in, uint64_t* __restrict__ out, size_t words) {
    const size_t quads = words >> 2;
    for (size_t q = blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x; q < quads;
         q += static_cast<size_t>(gridDim.x) * kThreads) {
        const Packed4 x = reinterpret_cast<const Packed4*>(in)[q];
        reinterpret_cast<U64x2*>(out)[2 * q] = U64x2{x.x, x.y};
        reinterpret_cast<U64x2*>(out)[2 * q + 1] = U64x2{x.z, x.w};
    }
    if (blockIdx.x == 0 && threadIdx.x < (words & 3)) out[(quads << 2) + threadIdx.x] = in[(quads << 2) + threadIdx.x];
}
__global__ void __launch_bounds__(kThreads)
    narrow_kernel(const uint64_t* __restrict__ in, uint32_t* __restrict__ out, size_t words) {
    const size_t quads = words >> 2;
    for (size_t q = blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x; q < quads;
         q += static_cast<size_t>(gridDim.x) * kThreads) {
        const U64x2 a = reinterpret_cast<const U64x2*>(in)[2 * q], b = reinterpret_cast<const U64x2*>(in)[2 * q + 1];
        Packed4 y;
        y.x = static_cast<uint32_t>(a.x);
        y.y = static_cast<uint32_t>(a.y);
        y.z = static_cast<uint32_t>(b.x);
        y.w = static_cast<uint32_t>(b.y);
        reinterpret_cast<Packed4*>(out)[q] = y;
    }
    if (blockIdx.x == 0 && threadIdx.x < (words & 3))
        out[(quads << 2) + threadIdx.x] = static_cast<uint32_t>(in[(quads << 2) + threadIdx.x]);
}
// the reference point of the transforms' roofline figures: every word read once and written once, 8 bytes per lane (the
// NTT's access width).  NT = non-temporal like the transforms' row loads and stores, or the default cache policy.
template <bool NT>
__global__ void __launch_bounds__(kThreads)
    stream_copy_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, size_t words) {
    for (size_t i = blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x; i < words;
         i += static_cast<size_t>(gridDim.x) * kThreads) {
        if constexpr (NT) stream_store(out + i, stream_load(in + i));
        else out[i] = in[i];
    }
}
// `records` runs of record_words words, source runs src_stride words apart, destination runs dst_stride apart; four 16-byte
// words per lane (one per lane made 65 536 workgroups of the PIR tail's copy: 75 us for 2 x 134 MB)
constexpr int kCopyRecordVectors = 4;
__global__ void __launch_bounds__(kThreads)
    copy_records_kernel(const uint64_t* __restrict__ in, size_t src_stride, uint64_t* __restrict__ out, size_t dst_stride,
                        uint32_t blocks_per_record) {
    const size_t record = blockIdx.x / blocks_per_record;
    const size_t first = (blockIdx.x - record * blocks_per_record) * size_t(kThreads) * kCopyRecordVectors + threadIdx.x;
    const U64x2* src = reinterpret_cast<const U64x2*>(in + record * src_stride) + first;
    U64x2* dst = reinterpret_cast<U64x2*>(out + record * dst_stride) + first;
    U64x2 words[kCopyRecordVectors];
#pragma unroll
    for (int v = 0; v < kCopyRecordVectors; ++v) words[v] = src[v * kThreads];
#pragma unroll
    for (int v = 0; v < kCopyRecordVectors; ++v) dst[v * kThreads] = words[v];
}
}  // namespace

hipError_t launch_copy_records(const uint64_t* in, size_t src_stride, uint64_t* out, size_t dst_stride, size_t record_words,
                               size_t records, hipStream_t stream) {
    if (records == 0 || record_words == 0) return hipSuccess;
    constexpr size_t block_words = 2 * size_t(kThreads) * kCopyRecordVectors;
    const size_t blocks_per_record = record_words / block_words;
    if (record_words % block_words != 0 || (src_stride | dst_stride) % 2 != 0 || !launch_grid::launch_fits(blocks_per_record * records, kThreads) ||
        ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15u) != 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(copy_records_kernel, dim3(static_cast<unsigned>(blocks_per_record * records)), dim3(kThreads), 0, stream, in,
                       src_stride, out, dst_stride, static_cast<uint32_t>(blocks_per_record));
    return hipGetLastError();
}

hipError_t launch_stream_copy(const uint64_t* in, uint64_t* out, size_t words, bool non_temporal, hipStream_t stream) {
    if (words == 0) return hipSuccess;
    if (non_temporal)
        hipLaunchKernelGGL(stream_copy_kernel<true>, dim3(grid_for(words)), dim3(kThreads), 0, stream, in, out, words);
    else
        hipLaunchKernelGGL(stream_copy_kernel<false>, dim3(grid_for(words)), dim3(kThreads), 0, stream, in, out, words);
    return hipGetLastError();
}

hipError_t launch_widen_words(const uint32_t* in, uint64_t* out, size_t words, hipStream_t stream) {
    if (words == 0) return hipSuccess;
    hipLaunchKernelGGL(widen_kernel, dim3(grid_for((words >> 2) + 1)), dim3(kThreads), 0, stream, in, out, words);
    return hipGetLastError();
}
hipError_t launch_narrow_words(const uint64_t* in, uint32_t* out, size_t words, hipStream_t stream) {
    if (words == 0) return hipSuccess;
    hipLaunchKernelGGL(narrow_kernel, dim3(grid_for((words >> 2) + 1)), dim3(kThreads), 0, stream, in, out, words);
    return hipGetLastError();
}

}  // namespace heamd
