// arith_probe.hip -- TEST INFRASTRUCTURE (tests/test_gpu_device_math.py): runs the device-side arithmetic of
// csrc/device_math.hpp on caller-supplied operands, one lane per operand tuple, so that the stated ranges, congruences and
// exact values can be checked against Python integers.  One `kind` number per function or template variant: 0 .. 7 the
// limb-wise and shift-folded products, 10 .. 52 every other function of one result, 60 .. 83 the ProductSum accumulations.
// Apart from the limb-wise products' tables it computes no constant: the caller passes every factor in.  Not part of
// libhe_amd.so; built by __graft_entry__.build() into tests/device_probe/libarith_probe.so.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.hpp"
#include "host_math.hpp"

namespace {

using namespace heamd;

// a 64-bit word the compiler knows to be wave-uniform (it then keeps it in scalar registers)
__device__ __forceinline__ uint64_t uniform_word(uint64_t v) {
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(v))));
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(static_cast<uint32_t>(v >> 32))));
    return lo | (static_cast<uint64_t>(hi) << 32);
}

// kind 0: split_mul_add<false, false>(0, y, ...) on an unsigned word; kind 1: split_mul_signed<false> on a signed word
// (the constant's second word in signed limbs, as the inverse tables hold it); kinds 2 / 3: the same with the constant's
// words wave-uniform (every lane of a launch then takes constant 0)
template <int KIND>
__global__ void product_kernel(const uint64_t* __restrict__ operand, const uint64_t* __restrict__ w,
                               const uint64_t* __restrict__ wt, const uint64_t* __restrict__ factors, uint64_t p,
                               uint64_t* __restrict__ out, size_t count) {
    const size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x;
    if (i >= count) return;
    const uint64_t neg_2p = 0 - 2 * p;
    if constexpr (KIND == 0) {
        out[i] = split_mul_add<false, false>(0, operand[i], w[i], wt[i], factors[i], neg_2p);
    } else if constexpr (KIND == 1) {
        out[i] = split_mul_signed<false>(operand[i], w[i], wt[i], factors[i], neg_2p, p + (p << 31));
    } else {
        const uint64_t w0 = uniform_word(w[0]), t0 = uniform_word(wt[0]), f0 = uniform_word(factors[0]);
        if constexpr (KIND == 2) {
            out[i] = split_mul_add<true, false>(0, operand[i], w0, t0, f0, neg_2p);
        } else {
            uint64_t bias;
            asm volatile("v_mov_b64 %0, %1" : "=v"(bias) : "s"(p + (p << 31)));
            out[i] = split_mul_signed<true>(operand[i], w0, t0, f0, neg_2p, bias);
        }
    }
}

// kinds 4 / 5: fold_mul<false, false> / fold_mul<true, false> (p = 2^b - d: kModeFoldLazy and kModeFoldMinus); kinds 6 / 7:
// fold_mul<false, true> / fold_mul<true, true> (p = 2^60 + e: kModeFoldPlus).  The uniform kinds take constant 0 for every lane.
template <bool UNIFORM, bool PLUS>
__global__ void fold_kernel(const uint64_t* __restrict__ operand, const uint64_t* __restrict__ w, const uint64_t* __restrict__ wt,
                            uint64_t p, uint64_t* __restrict__ out, size_t count) {
    const size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x;
    if (i >= count) return;
    const FoldConstants fc = fold_constants<PLUS>(uniform_word(p));
    if constexpr (UNIFORM) out[i] = fold_mul<true, PLUS>(operand[i], uniform_word(w[0]), uniform_word(wt[0]), fc);
    else out[i] = fold_mul<false, PLUS>(operand[i], w[i], wt[i], fc);
}


// ---- every other primitive of device_math.hpp (kinds 10 .. 52) -------------------------------------------------------
// Words travel in columns: input j of lane i is in[j * count + i], output j goes to out[j * count + i].  V(j) is the
// lane's own word, U(j) element 0 of the column made wave-uniform (one constant per launch) -- taken wherever the
// function under test reads that operand from scalar registers.  The 32-bit functions use the low word of each column.
struct ProbeModulus {
    uint64_t p, barrett64, two64_mod_p, two64_mod_p_shoup;
    uint32_t wide_shift;
    uint64_t wide_factor;
};

struct Arity {
    int inputs, outputs;
};
constexpr int kFirstContractKind = 10, kLastContractKind = 52;
constexpr Arity kContractArity[kLastContractKind - kFirstContractKind + 1] = {
    {2, 1}, {2, 1}, {2, 1}, {2, 1}, {4, 1}, {2, 2},          // 10-15 mulhi32 mullo32 mulhi64 mulhi64_approx mullo64_sum2 mul_wide
    {2, 1}, {2, 1},                                          // 16-17 csub63<false> csub63<true>
    {3, 1}, {3, 1}, {2, 1}, {3, 1}, {3, 1}, {2, 1},          // 18-23 add_mod sub_mod neg_mod and the _uniform twins
    {4, 1}, {4, 1},                                          // 24-25 shoup_lazy shoup_mul
    {2, 1}, {2, 1}, {2, 1}, {2, 1},                          // 26-29 shoup_quotient<U, C>: <0,0> <1,0> <0,1> <1,1>
    {4, 1}, {4, 1}, {5, 1}, {5, 1},                          // 30-33 shoup_lazy4 _uniform _fma<false> _fma<true>
    {4, 1}, {4, 1}, {5, 1}, {5, 1},                          // 34-37 shoup_headroom _uniform _fma<false> _fma<true>
    {4, 1}, {4, 1},                                          // 38-39 shoup_mul_uniform_lazy shoup_mul_uniform
    {3, 1}, {3, 1}, {3, 1}, {5, 1}, {5, 1},                  // 40-44 barrett_reduce64 _uniform_lazy _uniform barrett_mul barrett_reduce128
    {5, 2}, {11, 1}, {11, 1}, {11, 1}, {11, 1},              // 45-49 product_sum_value reduce_product_sum _lazy _bounded_lazy _bounded
    {4, 1}, {4, 1}, {4, 1},                                  // 50-52 shoup32_lazy shoup32_lazy_mad<false> <true>
};

template <int KIND>
__global__ void contract_kernel(const uint64_t* __restrict__ in, size_t count, uint64_t* __restrict__ out) {
    const size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x;
    if (i >= count) return;
    auto V = [&](int j) { return in[size_t(j) * count + i]; };
    auto U = [&](int j) { return uniform_word(in[size_t(j) * count]); };
    auto O = [&](int j, uint64_t v) { out[size_t(j) * count + i] = v; };
    // word products: (a, b) or (a, b, c, d)
    if constexpr (KIND == 10) O(0, mulhi32(lo32(V(0)), lo32(V(1))));
    if constexpr (KIND == 11) O(0, mullo32(lo32(V(0)), lo32(V(1))));
    if constexpr (KIND == 12) O(0, mulhi64(V(0), V(1)));
    if constexpr (KIND == 13) O(0, mulhi64_approx(V(0), V(1)));
    if constexpr (KIND == 14) O(0, mullo64_sum2(V(0), V(1), V(2), V(3)));
    if constexpr (KIND == 15) {
        const U128 r = mul_wide(V(0), V(1));
        O(0, r.lo);
        O(1, r.hi);
    }
    // (x, neg_m)
    if constexpr (KIND == 16) O(0, csub63<false>(V(0), V(1)));
    if constexpr (KIND == 17) O(0, csub63<true>(V(0), U(1)));
    // (a, b, p) or (a, p)
    if constexpr (KIND == 18) O(0, add_mod(V(0), V(1), V(2)));
    if constexpr (KIND == 19) O(0, sub_mod(V(0), V(1), V(2)));
    if constexpr (KIND == 20) O(0, neg_mod(V(0), V(1)));
    if constexpr (KIND == 21) O(0, add_mod_uniform(V(0), V(1), U(2)));
    if constexpr (KIND == 22) O(0, sub_mod_uniform(V(0), V(1), U(2)));
    if constexpr (KIND == 23) O(0, neg_mod_uniform(V(0), U(1)));
    // (x, w, wf, p)
    if constexpr (KIND == 24) O(0, shoup_lazy(V(0), V(1), V(2), 0 - V(3)));
    if constexpr (KIND == 25) O(0, shoup_mul(V(0), V(1), V(2), V(3)));
    // (x, f)
    if constexpr (KIND == 26) O(0, shoup_quotient<false, false>(V(0), V(1)));
    if constexpr (KIND == 27) O(0, shoup_quotient<true, false>(V(0), U(1)));
    if constexpr (KIND == 28) O(0, shoup_quotient<false, true>(V(0), V(1)));
    if constexpr (KIND == 29) O(0, shoup_quotient<true, true>(V(0), U(1)));
    // (x, w, wf, p[, addend]): the reduction constant is always wave-uniform, the twiddle in the uniform forms
    if constexpr (KIND == 30) O(0, shoup_lazy4(V(0), V(1), V(2), 0 - U(3)));
    if constexpr (KIND == 31) O(0, shoup_lazy4_uniform(V(0), U(1), U(2), 0 - U(3)));
    if constexpr (KIND == 32) O(0, shoup_lazy4_fma<false>(V(4), V(0), V(1), V(2), 0 - U(3)));
    if constexpr (KIND == 33) O(0, shoup_lazy4_fma<true>(V(4), V(0), U(1), U(2), 0 - U(3)));
    // (x, w, wf >> 1, p[, addend])
    if constexpr (KIND == 34) O(0, shoup_headroom(V(0), V(1), V(2), 0 - 2 * U(3)));
    if constexpr (KIND == 35) O(0, shoup_headroom_uniform(V(0), U(1), U(2), 0 - 2 * U(3)));
    if constexpr (KIND == 36) O(0, shoup_headroom_fma<false>(V(4), V(0), V(1), V(2), 0 - 2 * U(3)));
    if constexpr (KIND == 37) O(0, shoup_headroom_fma<true>(V(4), V(0), U(1), U(2), 0 - 2 * U(3)));
    // (x, w, wf, p), all constants wave-uniform
    if constexpr (KIND == 38) O(0, shoup_mul_uniform_lazy(V(0), U(1), U(2), U(3)));
    if constexpr (KIND == 39) O(0, shoup_mul_uniform(V(0), U(1), U(2), U(3)));
    // (x, p, floor(2^64 / p))
    if constexpr (KIND == 40) O(0, barrett_reduce64(V(0), V(1), V(2)));
    if constexpr (KIND == 41) O(0, barrett_reduce64_uniform_lazy(V(0), U(1), U(2)));
    if constexpr (KIND == 42) O(0, barrett_reduce64_uniform(V(0), U(1), U(2)));
    // (x, y, p, floor(2^(bits + 62) / p), bits - 2)
    if constexpr (KIND == 43) O(0, barrett_mul(V(0), V(1), V(2), V(3), static_cast<int>(V(4))));
    // (x.lo, x.hi, p, floor(2^128 / p) low word, high word)
    if constexpr (KIND == 44) O(0, barrett_reduce128(U128{V(0), V(1)}, V(2), V(3), V(4)));
    // (t, c, h, t_carry, c_carry[, p, floor(2^64 / p), 2^64 mod p, its Shoup factor, wide_shift, wide_factor])
    if constexpr (KIND >= 45 && KIND <= 49) {
        const ProductSum s{V(0), V(1), V(2), lo32(V(3)), lo32(V(4))};
        if constexpr (KIND == 45) {
            const U128 r = product_sum_value(s);
            O(0, r.lo);
            O(1, r.hi);
        } else {
            const ProbeModulus m{U(5), U(6), U(7), U(8), lo32(U(9)), U(10)};
            if constexpr (KIND == 46) O(0, reduce_product_sum(s, m));
            if constexpr (KIND == 47) O(0, reduce_product_sum_lazy(s, m));
            if constexpr (KIND == 48) O(0, reduce_product_sum_bounded_lazy(s, m));
            if constexpr (KIND == 49) O(0, reduce_product_sum_bounded(s, m));
        }
    }
    // (x, w, floor(w 2^32 / p), p)
    if constexpr (KIND == 50) O(0, shoup32_lazy(lo32(V(0)), lo32(V(1)), lo32(V(2)), lo32(V(3))));
    if constexpr (KIND == 51) O(0, shoup32_lazy_mad<false>(lo32(V(0)), lo32(V(1)), lo32(V(2)), 0u - lo32(U(3))));
    if constexpr (KIND == 52) O(0, shoup32_lazy_mad<true>(lo32(V(0)), lo32(U(1)), lo32(U(2)), 0u - lo32(U(3))));
}

template <int KIND>
void launch_contract(int kind, dim3 grid, dim3 block, const uint64_t* in, size_t count, uint64_t* out) {
    if (kind == KIND) hipLaunchKernelGGL(contract_kernel<KIND>, grid, block, 0, 0, in, count, out);
    else if constexpr (KIND < kLastContractKind) launch_contract<KIND + 1>(kind, grid, block, in, count, out);
}

// ---- sums of products (kinds 60 .. 83): each lane accumulates `terms` products per sum ---------------------------
//   60 product_sum_add | 61 / 62 _add_one<false / true> | 63 / 64 _add_pair | 65 / 66 _add_triple
//   67 + 2 k + NARROW: _add_all<POLYS, NARROW>, POLYS = 1, 2, 3, 4, 5, 7 for k = 0 .. 5
//   79 _add_uniform | 80 _add_uniform_short
//   81 _first then _add | 82 _first_uniform then _add_uniform | 83 _first_uniform_short then _add_uniform_short
// a[(j * terms + k) * count + i]: term k of sum j of lane i; b[k * count + i] (element 0 of each term in the uniform kinds);
// out[(j * 7 + f) * count + i]: f = t, c, h, t_carry, c_carry, value.lo, value.hi.  Sums start from product_sum_zero()
// unless a _first opens them.
constexpr int kFirstSumKind = 60, kLastSumKind = 83;
constexpr int kAllPolys[6] = {1, 2, 3, 4, 5, 7};
constexpr int sums_of(int kind) {
    return kind == 63 || kind == 64 ? 2 : kind == 65 || kind == 66 ? 3 : kind >= 67 && kind <= 78 ? kAllPolys[(kind - 67) / 2] : 1;
}

template <int KIND>
__global__ void product_sum_kernel(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, size_t terms, size_t count,
                                   uint64_t* __restrict__ out) {
    const size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x;
    if (i >= count) return;
    constexpr int SUMS = sums_of(KIND);
    auto A = [&](int j, size_t k) { return a[(size_t(j) * terms + k) * count + i]; };
    auto B = [&](size_t k) { return b[k * count + i]; };
    auto BU = [&](size_t k) { return uniform_word(b[k * count]); };
    ProductSum s[SUMS];
#pragma unroll
    for (int j = 0; j < SUMS; ++j) s[j] = product_sum_zero();
    size_t k = 0;
    if constexpr (KIND == 81) s[0] = product_sum_first(A(0, 0), B(0));
    if constexpr (KIND == 82) s[0] = product_sum_first_uniform(A(0, 0), BU(0));
    if constexpr (KIND == 83) s[0] = product_sum_first_uniform_short(A(0, 0), BU(0));
    if constexpr (KIND >= 81) k = 1;
    for (; k < terms; ++k) {
        if constexpr (KIND == 60 || KIND == 81) product_sum_add(s[0], A(0, k), B(k));
        if constexpr (KIND == 61) product_sum_add_one<false>(s[0], A(0, k), B(k));
        if constexpr (KIND == 62) product_sum_add_one<true>(s[0], A(0, k), B(k));
        if constexpr (KIND == 63) product_sum_add_pair<false>(s[0], s[1], A(0, k), A(1, k), B(k));
        if constexpr (KIND == 64) product_sum_add_pair<true>(s[0], s[1], A(0, k), A(1, k), B(k));
        if constexpr (KIND == 65) product_sum_add_triple<false>(s[0], s[1], s[2], A(0, k), A(1, k), A(2, k), B(k));
        if constexpr (KIND == 66) product_sum_add_triple<true>(s[0], s[1], s[2], A(0, k), A(1, k), A(2, k), B(k));
        if constexpr (KIND >= 67 && KIND <= 78) {
            uint64_t words[SUMS];
#pragma unroll
            for (int j = 0; j < SUMS; ++j) words[j] = A(j, k);
            product_sum_add_all<SUMS, ((KIND - 67) & 1) != 0>(s, words, B(k));
        }
        if constexpr (KIND == 79 || KIND == 82) product_sum_add_uniform(s[0], A(0, k), BU(k));
        if constexpr (KIND == 80 || KIND == 83) product_sum_add_uniform_short(s[0], A(0, k), BU(k));
    }
#pragma unroll
    for (int j = 0; j < SUMS; ++j) {
        const U128 value = product_sum_value(s[j]);
        const uint64_t fields[7] = {s[j].t, s[j].c, s[j].h, s[j].t_carry, s[j].c_carry, value.lo, value.hi};
#pragma unroll
        for (int f = 0; f < 7; ++f) out[(size_t(j) * 7 + f) * count + i] = fields[f];
    }
}

template <int KIND>
void launch_product_sum(int kind, dim3 grid, dim3 block, const uint64_t* a, const uint64_t* b, size_t terms, size_t count,
                        uint64_t* out) {
    if (kind == KIND) hipLaunchKernelGGL(product_sum_kernel<KIND>, grid, block, 0, 0, a, b, terms, count, out);
    else if constexpr (KIND < kLastSumKind) launch_product_sum<KIND + 1>(kind, grid, block, a, b, terms, count, out);
}

// host words -> device, kernel, device words -> host; 0 or the hipError_t that stopped it
template <typename Launch>
int run_on_device(const uint64_t* const* inputs, const size_t* input_words, int input_count, uint64_t* out, size_t out_words,
                  Launch launch) {
    size_t total = out_words;
    for (int j = 0; j < input_count; ++j) total += input_words[j];
    uint64_t* device = nullptr;
    hipError_t e = hipMalloc(&device, total * sizeof(uint64_t));
    if (e != hipSuccess) return int(e);
    const uint64_t* d_in[2] = {nullptr, nullptr};
    uint64_t* cursor = device;
    for (int j = 0; j < input_count && e == hipSuccess; ++j) {
        d_in[j] = cursor;
        e = hipMemcpy(cursor, inputs[j], input_words[j] * sizeof(uint64_t), hipMemcpyHostToDevice);
        cursor += input_words[j];
    }
    if (e == hipSuccess) {
        launch(d_in[0], d_in[1], cursor);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, cursor, out_words * sizeof(uint64_t), hipMemcpyDeviceToHost);
    (void)hipFree(device);
    return int(e);
}

}  // namespace

// operand[count], constant[count] -> out[count] = the shift-folded product (kinds 4..7 above).  Host pointers.
extern "C" int arith_probe_fold_product(int kind, uint64_t p, const uint64_t* operand, const uint64_t* constant, size_t count,
                                        uint64_t* out) {
    if (kind < 4 || kind > 7 || count == 0) return -1;
    uint64_t* host = static_cast<uint64_t*>(malloc(count * sizeof(uint64_t)));
    for (size_t i = 0; i < count; ++i) host[i] = heamd::split_shifted(constant[i], p);
    uint64_t* device = nullptr;
    hipError_t e = hipMalloc(&device, 4 * count * sizeof(uint64_t));
    if (e != hipSuccess) { free(host); return int(e); }
    uint64_t *d_operand = device, *d_w = device + count, *d_wt = device + 2 * count, *d_out = device + 3 * count;
    e = hipMemcpy(d_operand, operand, count * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_w, constant, count * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_wt, host, count * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const dim3 grid(static_cast<unsigned>((count + 255) / 256)), block(256);
        switch (kind) {
            case 4: hipLaunchKernelGGL((fold_kernel<false, false>), grid, block, 0, 0, d_operand, d_w, d_wt, p, d_out, count); break;
            case 5: hipLaunchKernelGGL((fold_kernel<true, false>), grid, block, 0, 0, d_operand, d_w, d_wt, p, d_out, count); break;
            case 6: hipLaunchKernelGGL((fold_kernel<false, true>), grid, block, 0, 0, d_operand, d_w, d_wt, p, d_out, count); break;
            default: hipLaunchKernelGGL((fold_kernel<true, true>), grid, block, 0, 0, d_operand, d_w, d_wt, p, d_out, count); break;
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out, count * sizeof(uint64_t), hipMemcpyDeviceToHost);
    (void)hipFree(device);
    free(host);
    return int(e);
}

// operand[count], constant[count] (constants below p; kinds 2 / 3 use constant[0] for every operand) -> out[count].
// Host pointers.  Returns 0 or the hipError_t that stopped it.
extern "C" int arith_probe_split_product(int kind, uint64_t p, const uint64_t* operand, const uint64_t* constant, size_t count,
                                         uint64_t* out) {
    if (kind < 0 || kind > 3 || count == 0) return -1;
    const bool signed_limbs = (kind & 1) != 0;
    uint64_t* host = static_cast<uint64_t*>(malloc(3 * count * sizeof(uint64_t)));
    for (size_t i = 0; i < count; ++i) {
        uint64_t shifted = heamd::split_shifted(constant[i], p);
        if (signed_limbs) shifted += (shifted & 0x80000000ull) << 1;  // as PolyContext::upload stores the inverse tables
        host[i] = shifted;
        host[count + i] = heamd::split_factors(constant[i], p);
    }
    uint64_t* device = nullptr;
    hipError_t e = hipMalloc(&device, 5 * count * sizeof(uint64_t));
    if (e != hipSuccess) { free(host); return int(e); }
    uint64_t *d_operand = device, *d_w = device + count, *d_wt = device + 2 * count, *d_f = device + 3 * count,
             *d_out = device + 4 * count;
    e = hipMemcpy(d_operand, operand, count * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_w, constant, count * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_wt, host, count * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_f, host + count, count * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const dim3 grid(static_cast<unsigned>((count + 255) / 256)), block(256);
        switch (kind) {
            case 0: hipLaunchKernelGGL(product_kernel<0>, grid, block, 0, 0, d_operand, d_w, d_wt, d_f, p, d_out, count); break;
            case 1: hipLaunchKernelGGL(product_kernel<1>, grid, block, 0, 0, d_operand, d_w, d_wt, d_f, p, d_out, count); break;
            case 2: hipLaunchKernelGGL(product_kernel<2>, grid, block, 0, 0, d_operand, d_w, d_wt, d_f, p, d_out, count); break;
            default: hipLaunchKernelGGL(product_kernel<3>, grid, block, 0, 0, d_operand, d_w, d_wt, d_f, p, d_out, count); break;
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out, count * sizeof(uint64_t), hipMemcpyDeviceToHost);
    (void)hipFree(device);
    free(host);
    return int(e);
}

// in[inputs][count] -> out[outputs][count] through the function that `kind` names (10 .. 52, the table above).  Host
// pointers; `inputs` and `outputs` must be the kind's own.  Returns 0, -1 for a bad call or the hipError_t.
extern "C" int arith_probe_contract(int kind, const uint64_t* in, int inputs, size_t count, uint64_t* out, int outputs) {
    if (kind < kFirstContractKind || kind > kLastContractKind || count == 0) return -1;
    const Arity arity = kContractArity[kind - kFirstContractKind];
    if (inputs != arity.inputs || outputs != arity.outputs) return -1;
    const uint64_t* host_in[1] = {in};
    const size_t words[1] = {size_t(inputs) * count};
    return run_on_device(host_in, words, 1, out, size_t(outputs) * count, [&](const uint64_t* d_in, const uint64_t*, uint64_t* d_out) {
        launch_contract<kFirstContractKind>(kind, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), d_in, count, d_out);
    });
}

// the number of sums a product-sum kind accumulates side by side (0 for an unknown kind)
extern "C" int arith_probe_product_sum_sums(int kind) { return kind < kFirstSumKind || kind > kLastSumKind ? 0 : sums_of(kind); }

// a[sums][terms][count], b[terms][count] -> out[sums][7][count] (kinds 60 .. 83, layout above).  Host pointers.
extern "C" int arith_probe_product_sum(int kind, const uint64_t* a, const uint64_t* b, size_t terms, size_t count, uint64_t* out) {
    if (kind < kFirstSumKind || kind > kLastSumKind || count == 0 || terms == 0) return -1;
    const size_t sums = size_t(sums_of(kind));
    const uint64_t* host_in[2] = {a, b};
    const size_t words[2] = {sums * terms * count, terms * count};
    return run_on_device(host_in, words, 2, out, sums * 7 * count, [&](const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out) {
        launch_product_sum<kFirstSumKind>(kind, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), d_a, d_b, terms, count,
                                          d_out);
    });
}
