// ntt_generic.hip -- the transform of any power-of-two degree without a tiled kernel, and its launcher.
#include <hip/hip_runtime.h>

#include "device_context.hpp"
#include "device_math.hpp"
#include "ntt_common.hpp"
#include "ntt_selectors.hpp"

namespace heamd {

namespace {

using namespace ntt;

// ---- any power-of-two degree: one workgroup per row, radix-2 stage loop over an LDS (or, for rows that do not
// fit, global-memory) buffer.  Exact Harvey butterflies in [0, 4p): valid for every modulus <= 2^62 - 1. ---------
template <bool USE_LDS>
__global__ void __launch_bounds__(256)
    ntt_forward_generic(uint64_t* __restrict__ slab, const DeviceContext ctx, uint32_t mod_base, uint32_t mod_period) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
    const uint32_t n = ctx.degree, logn = ctx.log_degree;
    const size_t row = blockIdx.x;
    const uint32_t mi = mod_base + static_cast<uint32_t>(row % mod_period);
    const DeviceModulus mod = ctx.moduli[mi];
    const U64x2* __restrict__ tw = ctx.forward_twiddles + static_cast<size_t>(mi) * n;
    uint64_t* x = slab + row * n;
    uint64_t* buf = USE_LDS ? lds : x;
    const uint64_t p = mod.p, two_p = 2 * p, neg_p = 0 - p;
    if (USE_LDS) {
        for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) buf[k] = x[k];
        __syncthreads();
    }
    for (uint32_t s = 0; s < logn; ++s) {
        const uint32_t t = n >> (s + 1);
        const bool last = (s + 1 == logn);
        for (uint32_t k = threadIdx.x; k < (n >> 1); k += blockDim.x) {
            const uint32_t i = k >> (logn - 1 - s), o = k & (t - 1);
            const uint32_t a = 2 * i * t + o;
            const U64x2 w = tw[(1u << s) + i];
            uint64_t xv = csub(buf[a], two_p);
            const uint64_t tv = shoup_lazy(buf[a + t], w.x, w.y, neg_p);
            uint64_t xo = xv + tv, yo = xv + two_p - tv;
            if (last) {
                xo = canonicalize<kModeExact>(xo, p);
                yo = canonicalize<kModeExact>(yo, p);
            }
            buf[a] = xo;
            buf[a + t] = yo;
        }
        __syncthreads();
    }
    if (USE_LDS) {
        for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) x[k] = buf[k];
    }
}

template <bool USE_LDS>
__global__ void __launch_bounds__(256)
    ntt_inverse_generic(uint64_t* __restrict__ slab, const DeviceContext ctx, uint32_t mod_base, uint32_t mod_period) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
    const uint32_t n = ctx.degree, logn = ctx.log_degree;
    const size_t row = blockIdx.x;
    const uint32_t mi = mod_base + static_cast<uint32_t>(row % mod_period);
    const DeviceModulus mod = ctx.moduli[mi];
    const U64x2* __restrict__ tw = ctx.inverse_twiddles + static_cast<size_t>(mi) * n;
    uint64_t* x = slab + row * n;
    uint64_t* buf = USE_LDS ? lds : x;
    const uint64_t p = mod.p, two_p = 2 * p, neg_p = 0 - p;
    if (USE_LDS) {
        for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) buf[k] = x[k];
        __syncthreads();
    }
    for (uint32_t b = 0; b < logn; ++b) {
        const uint32_t t = 1u << b, m = n >> (b + 1);
        const bool last = (b + 1 == logn);
        for (uint32_t k = threadIdx.x; k < (n >> 1); k += blockDim.x) {
            const uint32_t i = k >> b, o = k & (t - 1);
            const uint32_t a = 2 * i * t + o;
            const uint64_t xv = buf[a], yv = buf[a + t];
            const uint64_t sum = xv + yv, diff = xv + two_p - yv;
            if (last) {
                buf[a] = shoup_mul(sum, mod.inv_degree, mod.inv_degree_shoup, p);
                buf[a + t] = shoup_mul(diff, mod.inv_degree_root, mod.inv_degree_root_shoup, p);
            } else {
                const U64x2 w = tw[(n - 2 * m + 1) + i];
                buf[a] = csub(sum, two_p);
                buf[a + t] = shoup_lazy(diff, w.x, w.y, neg_p);
            }
        }
        __syncthreads();
    }
    if (USE_LDS) {
        for (uint32_t k = threadIdx.x; k < n; k += blockDim.x) x[k] = buf[k];
    }
}

}  // namespace

hipError_t launch_generic(bool inverse, uint64_t* slab, const DeviceContext& ctx, uint32_t mod_base, uint32_t mod_period, size_t rows,
                          hipStream_t stream) {
    const uint32_t n = ctx.degree;
    if (n < 2) return hipSuccess;  // degree 1: no stages (the reference loops over zero stages)
    const bool use_lds = n <= 4096;
    const unsigned threads = n / 2 < 256 ? (n / 2 < 64 ? 64 : n / 2) : 256;
    const size_t lds_bytes = use_lds ? n * sizeof(uint64_t) : 0;
    using Kernel = void (*)(uint64_t*, const DeviceContext, uint32_t, uint32_t);
    Kernel kernel = inverse ? (use_lds ? ntt_inverse_generic<true> : ntt_inverse_generic<false>)
                            : (use_lds ? ntt_forward_generic<true> : ntt_forward_generic<false>);
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(rows)), dim3(threads), lds_bytes, stream, slab, ctx,
                       mod_base, mod_period);
    return hipGetLastError();
}

}  // namespace heamd
