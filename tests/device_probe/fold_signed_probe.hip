// fold_signed_probe.hip -- TEST INFRASTRUCTURE (tests/test_gpu_fold_signed_probe.py): runs csrc/device_math.hpp's
// fold_mul_signed on caller-supplied operands, one lane per (signed word, constant) pair, so that every result can be compared
// with the limb-by-limb Python model of tests/fold_signed_model.py.  It computes no constant but the ones the kernels compute
// themselves (fold_constants): the caller passes the constant's second word in signed limbs.  Not part of libhe_amd.so;
// built by __graft_entry__.build() into tests/device_probe/libfold_signed_probe.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.hpp"

namespace {

using namespace heamd;

__device__ __forceinline__ uint64_t uniform_word(uint64_t v) {
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(v))));
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(v >> 32))));
    return lo | (static_cast<uint64_t>(hi) << 32);
}

// UNIFORM = false: lane i multiplies operand[i] by constant i (its words in vector registers, K the scalar operand);
// UNIFORM = true: every lane multiplies by constant 0, its words wave-uniform, K in a VGPR pair -- as the passes hand it over
template <bool UNIFORM>
__global__ void fold_signed_kernel(const uint64_t* __restrict__ operand, const uint64_t* __restrict__ w,
                                   const uint64_t* __restrict__ wt_signed_limbs, uint64_t p, uint64_t* __restrict__ out, size_t count) {
    const size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x;
    if (i >= count) return;
    const FoldConstants fc = fold_constants<false>(uniform_word(p));
    if constexpr (UNIFORM) {
        uint64_t bias;
        asm volatile("v_mov_b64 %0, %1" : "=v"(bias) : "s"(fc.signed_bias));
        out[i] = fold_mul_signed<true>(operand[i], uniform_word(w[0]), uniform_word(wt_signed_limbs[0]), fc, bias);
    } else {
        out[i] = fold_mul_signed<false>(operand[i], w[i], wt_signed_limbs[i], fc, fc.signed_bias);
    }
}

}  // namespace

// operand[count] (two's complement), w[count], wt_signed_limbs[count] -> out[count] (two's complement); uniform != 0: constant 0
// serves every lane.  Host pointers.  Returns 0, -1 for a bad call or the hipError_t that stopped it.
extern "C" int fold_signed_probe_product(int uniform, uint64_t p, const uint64_t* operand, const uint64_t* w,
                                         const uint64_t* wt_signed_limbs, size_t count, uint64_t* out) {
    if (count == 0) return -1;
    uint64_t* device = nullptr;
    hipError_t e = hipMalloc(&device, 4 * count * sizeof(uint64_t));
    if (e != hipSuccess) return int(e);
    uint64_t *d_operand = device, *d_w = device + count, *d_wt = device + 2 * count, *d_out = device + 3 * count;
    e = hipMemcpy(d_operand, operand, count * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_w, w, count * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_wt, wt_signed_limbs, count * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const dim3 grid(static_cast<unsigned>((count + 255) / 256)), block(256);
        if (uniform != 0) hipLaunchKernelGGL(fold_signed_kernel<true>, grid, block, 0, 0, d_operand, d_w, d_wt, p, d_out, count);
        else hipLaunchKernelGGL(fold_signed_kernel<false>, grid, block, 0, 0, d_operand, d_w, d_wt, p, d_out, count);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out, count * sizeof(uint64_t), hipMemcpyDeviceToHost);
    (void)hipFree(device);
    return int(e);
}
