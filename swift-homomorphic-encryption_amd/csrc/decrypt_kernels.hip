// decrypt_kernels.hip -- the last step of every server path, on ciphertexts resident in HBM (reference Sources/
// HomomorphicEncryption/Bfv/):
//   Bfv.dotProduct            Bfv+Decrypt.swift:188-204   c0 + c1 s [+ c2 s^2] in Eval form, one pass over the ciphertexts
//                                                         (Coeff-form input: c1 s [+ c2 s^2], and c0 added in Coeff form)
//   Bfv.noiseBudgetEval       Bfv+Decrypt.swift:116-149   max_k |[t dot_k]_Q| as an exact integer, one workgroup per ciphertext
//   Bfv.isTransparent         Bfv+Encrypt.swift:48-62     polynomials 1.. all zero
//
// The norm is taken in a mixed radix (Garner's digits) instead of composing every coefficient as CrtComposer.compose does
// (CrtComposer.swift:76-97): digit i lies under q_i, digits compare lexicographically, and a coefficient costs L (L - 1) / 2
// one-word products with constants the context already holds (inverse_q_last: q_k^-1 mod q_i for i < k) and no multi-limb
// arithmetic.  Only the maximum of a ciphertext is turned into 64-bit limbs, by one lane.  The maximum is a compare-and-select
// over the lanes' digits (wave shuffles, then LDS across the waves): no atomics, no floating point, the same result in any
// order.  All stores are ordinary vector stores.
//
// Every kernel runs on an exact grid (launch_grid::exact_grid): a lane of the dot product owns one 16-byte vector, a workgroup of
// the other two one ciphertext, and none strides by the grid; a batch HIP cannot launch is refused, not covered in part.
#include <hip/hip_runtime.h>

#include "decrypt_kernels.hpp"
#include "device_math.hpp"
#include "launch_grid.hpp"

namespace heamd {
namespace {

constexpr unsigned kThreads = 256;
constexpr unsigned kWaves = kThreads / 64;

typedef unsigned int QuadWords __attribute__((ext_vector_type(4)));

// V consecutive words of a row per lane: one 16-byte access (V = 2 of 8 bytes, V = 4 of 4 bytes), or V = 1.
// STREAM: ciphertext words, touched once (non-temporal); the secret key is re-read by every ciphertext and stays cached.
template <int V, bool STREAM, typename W>
__device__ __forceinline__ void load_words(const W* p, uint64_t (&x)[V]) {
    if constexpr (V == 1) {
        x[0] = STREAM ? stream_load(p) : uint64_t(*p);
    } else if constexpr (sizeof(W) == 8) {
        static_assert(V == 2, "two 8-byte words per lane");
        const U64x2 pair = STREAM ? stream_load(reinterpret_cast<const U64x2*>(p)) : *reinterpret_cast<const U64x2*>(p);
        x[0] = pair.x;
        x[1] = pair.y;
    } else {
        static_assert(V == 4 && sizeof(W) == 4, "four 4-byte words per lane");
        const QuadWords quad = STREAM ? __builtin_nontemporal_load(reinterpret_cast<const QuadWords*>(p))
                                      : *reinterpret_cast<const QuadWords*>(p);
        x[0] = quad.x;
        x[1] = quad.y;
        x[2] = quad.z;
        x[3] = quad.w;
    }
}
template <int V, typename W>
__device__ __forceinline__ void store_words(W* p, const uint64_t (&x)[V]) {
    if constexpr (V == 1) {
        stream_store(p, x[0]);
    } else if constexpr (sizeof(W) == 8) {
        stream_store(reinterpret_cast<U64x2*>(p), U64x2{x[0], x[1]});
    } else {
        const QuadWords quad = {lo32(x[0]), lo32(x[1]), lo32(x[2]), lo32(x[3])};
        __builtin_nontemporal_store(quad, reinterpret_cast<QuadWords*>(p));
    }
}
template <int V>
constexpr uint32_t log2_of() {
    return V == 4 ? 2 : V == 2 ? 1 : 0;
}
template <typename W>
constexpr int kWordsPer16Bytes = 16 / sizeof(W);
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ---- secret-key dot product ------------------------------------------------------------------------------------------
// One lane = V consecutive coefficients of one residue row of one ciphertext: it reads the POLYS ciphertext words and the
// key's word there once, forms s^2 in registers (no slab of key powers exists) and writes the sum.  Results are canonical, so
// the order of the additions is free.  vectors_per_poly = L N / V.
// WITH_C0 = false: `cts` holds the POLYS - 1 polynomials behind the first only ([batch][POLYS - 1][L][N]) and the sum is
// c1 s [+ c2 s^2] -- what Coeff-form input needs in Eval form: the transform is linear, so c0 joins after the inverse
// transform (add_first_polynomial_kernel) and is neither copied nor transformed.
template <int POLYS, bool WITH_C0, int V, typename W>
__global__ void __launch_bounds__(kThreads)
    secret_dot_product_kernel(const W* __restrict__ cts, const W* __restrict__ secret_key, W* __restrict__ out,
                              const DeviceContext ctx, size_t vectors_per_poly, size_t batch) {
    static_assert(WITH_C0 || POLYS > 1, "a single polynomial is its own dot product");
    constexpr int kStored = WITH_C0 ? POLYS : POLYS - 1, kFirstTerm = WITH_C0 ? 1 : 0;
    const uint32_t log_vectors_per_row = ctx.log_degree - log2_of<V>();
    const size_t i = blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x;  // (launch_grid::exact_grid)
    if (i >= vectors_per_poly * batch) return;
    const size_t b = i / vectors_per_poly, k = i - b * vectors_per_poly;
    const DeviceModulus* m = ctx.moduli + (k >> log_vectors_per_row);
    const uint64_t p = m->p, factor = m->product_factor;
    const int shift = static_cast<int>(m->product_shift);
    const W* ct = cts + (b * kStored * vectors_per_poly + k) * V;
    uint64_t sum[V];
    if constexpr (WITH_C0) {
        load_words<V, true>(ct, sum);
    } else {
#pragma unroll
        for (int v = 0; v < V; ++v) sum[v] = 0;
    }
    if constexpr (POLYS > 1) {
        uint64_t s[V], c[V];
        load_words<V, false>(secret_key + k * V, s);
        load_words<V, true>(ct + kFirstTerm * vectors_per_poly * V, c);
#pragma unroll
        for (int v = 0; v < V; ++v) sum[v] = add_mod(sum[v], barrett_mul(c[v], s[v], p, factor, shift), p);
        if constexpr (POLYS > 2) {
            load_words<V, true>(ct + (kFirstTerm + 1) * vectors_per_poly * V, c);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const uint64_t s_squared = barrett_mul(s[v], s[v], p, factor, shift);
                sum[v] = add_mod(sum[v], barrett_mul(c[v], s_squared, p, factor, shift), p);
            }
        }
    }
    store_words<V>(out + i * V, sum);
}

// out [batch][L][N] += c0 of cts [batch][poly_count][L][N], both Coeff: the last step of the dot product of Coeff-form input
template <int V, typename W>
__global__ void __launch_bounds__(kThreads)
    add_first_polynomial_kernel(const W* __restrict__ cts, W* __restrict__ out, const DeviceContext ctx, uint32_t poly_count,
                                size_t vectors_per_poly, size_t batch) {
    const uint32_t log_vectors_per_row = ctx.log_degree - log2_of<V>();
    const size_t i = blockIdx.x * static_cast<size_t>(kThreads) + threadIdx.x;  // (launch_grid::exact_grid)
    if (i >= vectors_per_poly * batch) return;
    const size_t b = i / vectors_per_poly, k = i - b * vectors_per_poly;
    const uint64_t p = ctx.moduli[k >> log_vectors_per_row].p;
    uint64_t sum[V], c0[V];
    load_words<V, true>(out + i * V, sum);
    load_words<V, true>(cts + (b * poly_count * vectors_per_poly + k) * V, c0);
#pragma unroll
    for (int v = 0; v < V; ++v) sum[v] = add_mod(sum[v], c0[v], p);
    store_words<V>(out + i * V, sum);
}

// the exact grid of one lane per V words of [batch][L][N]; false when HIP cannot launch it
template <int V>
bool vector_grid(const DeviceContext& ctx, size_t batch, size_t& vectors_per_poly, dim3& grid) {
    vectors_per_poly = (static_cast<size_t>(ctx.moduli_count) << ctx.log_degree) / V;
    if (!launch_grid::launch_fits(launch_grid::grid_blocks(vectors_per_poly * batch, kThreads, SIZE_MAX), kThreads)) return false;
    grid = dim3(launch_grid::exact_grid(vectors_per_poly * batch, kThreads));
    return true;
}

template <int V, typename W>
hipError_t launch_secret_dot_product_vectors(const W* cts, const W* secret_key, W* out, const DeviceContext& ctx,
                                             uint32_t poly_count, bool with_c0, size_t batch, hipStream_t stream) {
    size_t vectors_per_poly = 0;
    dim3 grid, block(kThreads);
    if (!vector_grid<V>(ctx, batch, vectors_per_poly, grid)) return hipErrorInvalidValue;
#define HEAMD_DOT_LAUNCH(POLYS, WITH_C0)                                                                                 \
    hipLaunchKernelGGL((secret_dot_product_kernel<POLYS, WITH_C0, V, W>), grid, block, 0, stream, cts, secret_key, out, ctx, \
                       vectors_per_poly, batch)
    switch (poly_count * 2 + (with_c0 ? 1 : 0)) {
        case 3: HEAMD_DOT_LAUNCH(1, true); break;
        case 4: HEAMD_DOT_LAUNCH(2, false); break;
        case 5: HEAMD_DOT_LAUNCH(2, true); break;
        case 6: HEAMD_DOT_LAUNCH(3, false); break;
        case 7: HEAMD_DOT_LAUNCH(3, true); break;
        default: return hipErrorInvalidValue;
    }
#undef HEAMD_DOT_LAUNCH
    return hipGetLastError();
}

// every row starts on a 16-byte boundary when the degree is a multiple of the vector and the bases are aligned
template <typename W>
bool rows_are_16_byte_aligned(const DeviceContext& ctx, const void* a, const void* b, const void* c) {
    return ctx.degree >= static_cast<uint32_t>(kWordsPer16Bytes<W>) && aligned16(a) && aligned16(b) && aligned16(c);
}

template <typename W>
hipError_t launch_secret_dot_product_words(const W* cts, const W* secret_key, W* out, const DeviceContext& ctx,
                                           uint32_t poly_count, bool with_c0, size_t batch, hipStream_t stream) {
    if (batch == 0) return hipSuccess;
    if (poly_count == 0 || poly_count > kMaxDecryptPolys || ctx.moduli_count == 0) return hipErrorInvalidValue;
    if (rows_are_16_byte_aligned<W>(ctx, cts, secret_key, out))
        return launch_secret_dot_product_vectors<kWordsPer16Bytes<W>>(cts, secret_key, out, ctx, poly_count, with_c0, batch, stream);
    return launch_secret_dot_product_vectors<1>(cts, secret_key, out, ctx, poly_count, with_c0, batch, stream);
}

template <int V, typename W>
hipError_t launch_add_first_polynomial_vectors(const W* cts, W* out, const DeviceContext& ctx, uint32_t poly_count, size_t batch,
                                               hipStream_t stream) {
    size_t vectors_per_poly = 0;
    dim3 grid;
    if (!vector_grid<V>(ctx, batch, vectors_per_poly, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((add_first_polynomial_kernel<V, W>), grid, dim3(kThreads), 0, stream, cts, out, ctx, poly_count,
                       vectors_per_poly, batch);
    return hipGetLastError();
}

template <typename W>
hipError_t launch_add_first_polynomial_words(const W* cts, W* out, const DeviceContext& ctx, uint32_t poly_count, size_t batch,
                                             hipStream_t stream) {
    if (batch == 0) return hipSuccess;
    if (poly_count == 0 || ctx.moduli_count == 0) return hipErrorInvalidValue;
    if (rows_are_16_byte_aligned<W>(ctx, cts, out, out))
        return launch_add_first_polynomial_vectors<kWordsPer16Bytes<W>>(cts, out, ctx, poly_count, batch, stream);
    return launch_add_first_polynomial_vectors<1>(cts, out, ctx, poly_count, batch, stream);
}

// ---- noise norm --------------------------------------------------------------------------------------------------------
// a > b for digit arrays whose index 0 is the most significant
template <int L>
__device__ __forceinline__ bool digits_greater(const uint64_t (&a)[L], const uint64_t (&b)[L]) {
    bool greater = false;
#pragma unroll
    for (int i = L - 1; i >= 0; --i) greater = a[i] > b[i] || (a[i] == b[i] && greater);
    return greater;
}

// One workgroup per ciphertext, a lane per coefficient (striding by the workgroup).  Per coefficient:
// r_i = t dot_i mod q_i, its mixed-radix digits e, the centring (x > (Q + 1) >> 1 ? Q - x : x, Bfv+Decrypt.swift:136-143) on
// the digits -- Q - x = (Q - 1 - x) + 1, and Q - 1 has every digit at its largest --, then the running maximum.
template <int L, typename W>
__global__ void __launch_bounds__(kThreads)
    noise_norm_kernel(const W* __restrict__ dot, uint64_t* __restrict__ out_limbs, const DeviceContext ctx,
                      const NoiseNormTables tables, size_t batch) {
    __shared__ uint64_t wave_best[kWaves][L];
    const uint32_t n = ctx.degree;
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t ct = blockIdx.x;  // (launch_grid::exact_grid: one workgroup per ciphertext)
    if (ct >= batch) return;
    const W* src = dot + ((ct * L) << ctx.log_degree);
    uint64_t best[L];
#pragma unroll
    for (int i = 0; i < L; ++i) best[i] = 0;
    for (uint32_t k = threadIdx.x; k < n; k += kThreads) {
        uint64_t e[L];
#pragma unroll
        for (int i = 0; i < L; ++i)
            e[i] = shoup_mul(stream_load(src + (static_cast<size_t>(i) << ctx.log_degree) + k), tables.t_mod_q[i].x,
                             tables.t_mod_q[i].y, ctx.moduli[i].p);
        // Garner from the last modulus down: e[j] is final once every later digit has been taken out of it
#pragma unroll
        for (int j = L - 1; j > 0; --j) {
            const U64x2* inverse_q_j = ctx.inverse_q_last + static_cast<size_t>(j) * ctx.moduli_stride;
#pragma unroll
            for (int i = 0; i < j; ++i) {
                const uint64_t q = ctx.moduli[i].p;
                const uint64_t digit = barrett_reduce64(e[j], q, ctx.moduli[i].barrett64);
                e[i] = shoup_mul(sub_mod(e[i], digit, q), inverse_q_j[i].x, inverse_q_j[i].y, q);
            }
        }
        bool above = false;  // x > (Q + 1) >> 1
#pragma unroll
        for (int i = L - 1; i >= 0; --i)
            above = e[i] > tables.half_digits[i] || (e[i] == tables.half_digits[i] && above);
        if (above) {
            uint64_t carry = 1;
#pragma unroll
            for (int i = L - 1; i >= 0; --i) {
                const uint64_t q = ctx.moduli[i].p;
                const uint64_t digit = q - 1 - e[i] + carry;
                carry = digit == q ? 1 : 0;
                e[i] = digit == q ? 0 : digit;
            }
        }
        if (digits_greater<L>(e, best)) {
#pragma unroll
            for (int i = 0; i < L; ++i) best[i] = e[i];
        }
    }
#pragma unroll
    for (int distance = 32; distance > 0; distance >>= 1) {
        uint64_t other[L];
#pragma unroll
        for (int i = 0; i < L; ++i)
            other[i] = static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(best[i]), distance, 64));
        if (digits_greater<L>(other, best)) {
#pragma unroll
            for (int i = 0; i < L; ++i) best[i] = other[i];
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < L; ++i) wave_best[wave][i] = best[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (unsigned w = 1; w < kWaves; ++w) {
            uint64_t other[L];
#pragma unroll
            for (int i = 0; i < L; ++i) other[i] = wave_best[w][i];
            if (digits_greater<L>(other, best)) {
#pragma unroll
                for (int i = 0; i < L; ++i) best[i] = other[i];
            }
        }
        // digits -> limbs: value = (...(e_0 q_1 + e_1) q_2 + ...) q_{L-1} + e_{L-1}; below q_0 .. q_j after step j
        uint64_t limb[L];
#pragma unroll
        for (int i = 0; i < L; ++i) limb[i] = 0;
        limb[0] = best[0];
#pragma unroll
        for (int j = 1; j < L; ++j) {
            const uint64_t q = ctx.moduli[j].p;
            uint64_t carry = best[j];
#pragma unroll
            for (int i = 0; i < j; ++i) {
                U128 product = mul_wide(limb[i], q);
                product.lo += carry;
                product.hi += product.lo < carry ? 1 : 0;
                limb[i] = product.lo;
                carry = product.hi;
            }
            limb[j] = carry;
        }
        uint64_t* dst = out_limbs + ct * tables.limbs;
#pragma unroll
        for (int i = 0; i < L; ++i)
            if (static_cast<uint32_t>(i) < tables.limbs) dst[i] = limb[i];
    }
}

template <int L, typename W>
hipError_t launch_noise_norm_moduli(const W* dot, uint64_t* out_limbs, const DeviceContext& ctx, const NoiseNormTables& tables,
                                    size_t batch, hipStream_t stream) {
    hipLaunchKernelGGL((noise_norm_kernel<L, W>), dim3(launch_grid::exact_grid(batch * kThreads, kThreads)), dim3(kThreads), 0,
                       stream, dot, out_limbs, ctx, tables, batch);
    return hipGetLastError();
}

template <typename W>
hipError_t launch_noise_norm_words(const W* dot, uint64_t* out_limbs, const DeviceContext& ctx, const NoiseNormTables& tables,
                                   size_t batch, hipStream_t stream) {
    if (batch == 0) return hipSuccess;
    if (tables.limbs == 0 || tables.limbs > ctx.moduli_count || !launch_grid::launch_fits(batch, kThreads))
        return hipErrorInvalidValue;
    switch (ctx.moduli_count) {
#define HEAMD_NOISE_CASE(L) \
    case L: return launch_noise_norm_moduli<L>(dot, out_limbs, ctx, tables, batch, stream);
        HEAMD_NOISE_CASE(1)
        HEAMD_NOISE_CASE(2)
        HEAMD_NOISE_CASE(3)
        HEAMD_NOISE_CASE(4)
        HEAMD_NOISE_CASE(5)
        HEAMD_NOISE_CASE(6)
        HEAMD_NOISE_CASE(7)
        HEAMD_NOISE_CASE(8)
        HEAMD_NOISE_CASE(9)
        HEAMD_NOISE_CASE(10)
        HEAMD_NOISE_CASE(11)
        HEAMD_NOISE_CASE(12)
        HEAMD_NOISE_CASE(13)
        HEAMD_NOISE_CASE(14)
        HEAMD_NOISE_CASE(15)
        HEAMD_NOISE_CASE(16)
#undef HEAMD_NOISE_CASE
        default: return hipErrorNotSupported;
    }
}
static_assert(kMaxNoiseModuli == 16, "the switch covers 1..16");

// ---- transparency ------------------------------------------------------------------------------------------------------
// One workgroup per ciphertext: the OR of every word behind the first polynomial.
template <int V, typename W>
__global__ void __launch_bounds__(kThreads)
    is_transparent_kernel(const W* __restrict__ cts, uint8_t* __restrict__ out_flags, size_t poly_words, uint32_t poly_count,
                          size_t batch) {
    const size_t vectors = (poly_count - 1) * poly_words / V;
    const size_t ct = blockIdx.x;  // (launch_grid::exact_grid: one workgroup per ciphertext)
    if (ct >= batch) return;
    const W* tail = cts + (ct * poly_count + 1) * poly_words;
    uint64_t any = 0;
    for (size_t v = threadIdx.x; v < vectors; v += kThreads) {
        uint64_t x[V];
        load_words<V, true>(tail + v * V, x);
#pragma unroll
        for (int j = 0; j < V; ++j) any |= x[j];
    }
    const int nonzero = __syncthreads_or(any != 0 ? 1 : 0);
    if (threadIdx.x == 0) out_flags[ct] = nonzero != 0 ? 0 : 1;
}

template <typename W>
hipError_t launch_is_transparent_words(const W* cts, uint8_t* out_flags, uint32_t log_degree, uint32_t rows, uint32_t poly_count,
                                       size_t batch, hipStream_t stream) {
    if (batch == 0) return hipSuccess;
    if (poly_count == 0 || rows == 0 || !launch_grid::launch_fits(batch, kThreads)) return hipErrorInvalidValue;
    const size_t poly_words = static_cast<size_t>(rows) << log_degree;
    const dim3 grid(launch_grid::exact_grid(batch * kThreads, kThreads)), block(kThreads);
    constexpr int kWide = kWordsPer16Bytes<W>;
    if (poly_words % kWide == 0 && aligned16(cts))
        hipLaunchKernelGGL((is_transparent_kernel<kWide, W>), grid, block, 0, stream, cts, out_flags, poly_words, poly_count, batch);
    else
        hipLaunchKernelGGL((is_transparent_kernel<1, W>), grid, block, 0, stream, cts, out_flags, poly_words, poly_count, batch);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_secret_dot_product(const uint64_t* cts, const uint64_t* secret_key, uint64_t* out, const DeviceContext& ctx,
                                     uint32_t poly_count, bool with_c0, size_t batch, hipStream_t stream) {
    return launch_secret_dot_product_words(cts, secret_key, out, ctx, poly_count, with_c0, batch, stream);
}
hipError_t launch_secret_dot_product(const uint32_t* cts, const uint32_t* secret_key, uint32_t* out, const DeviceContext& ctx,
                                     uint32_t poly_count, bool with_c0, size_t batch, hipStream_t stream) {
    return launch_secret_dot_product_words(cts, secret_key, out, ctx, poly_count, with_c0, batch, stream);
}
hipError_t launch_add_first_polynomial(const uint64_t* cts, uint64_t* out, const DeviceContext& ctx, uint32_t poly_count,
                                       size_t batch, hipStream_t stream) {
    return launch_add_first_polynomial_words(cts, out, ctx, poly_count, batch, stream);
}
hipError_t launch_add_first_polynomial(const uint32_t* cts, uint32_t* out, const DeviceContext& ctx, uint32_t poly_count,
                                       size_t batch, hipStream_t stream) {
    return launch_add_first_polynomial_words(cts, out, ctx, poly_count, batch, stream);
}
hipError_t launch_noise_norm(const uint64_t* dot, uint64_t* out_limbs, const DeviceContext& ctx, const NoiseNormTables& tables,
                             size_t batch, hipStream_t stream) {
    return launch_noise_norm_words(dot, out_limbs, ctx, tables, batch, stream);
}
hipError_t launch_noise_norm(const uint32_t* dot, uint64_t* out_limbs, const DeviceContext& ctx, const NoiseNormTables& tables,
                             size_t batch, hipStream_t stream) {
    return launch_noise_norm_words(dot, out_limbs, ctx, tables, batch, stream);
}
hipError_t launch_is_transparent(const uint64_t* cts, uint8_t* out_flags, uint32_t log_degree, uint32_t rows, uint32_t poly_count,
                                 size_t batch, hipStream_t stream) {
    return launch_is_transparent_words(cts, out_flags, log_degree, rows, poly_count, batch, stream);
}
hipError_t launch_is_transparent(const uint32_t* cts, uint8_t* out_flags, uint32_t log_degree, uint32_t rows, uint32_t poly_count,
                                 size_t batch, hipStream_t stream) {
    return launch_is_transparent_words(cts, out_flags, log_degree, rows, poly_count, batch, stream);
}

}  // namespace heamd
