// encrypt_kernels.hpp -- launchers of encrypt_kernels.hip (asynchronous on `stream`): the ternary and centred binomial
// samplers of PolyRq+Randomize.swift over the byte stream of NistAes128Ctr(seed:), and the element-wise steps that join them
// into Bfv.encryptZero and Bfv._generateKeySwitchKey.  Each launcher is a template on the slab word (uint64_t, or uint32_t
// with every modulus <= 2^30 - 1); both read the 8-byte image of the context.
// `chain`: the records launch_seeded_chain (aes_ctr_drbg.hpp) wrote for the seeds, [batch][chunks][48] words.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "device_context.hpp"

namespace heamd {

// 4096-byte chunks of the stream that one polynomial of degree N consumes
constexpr uint32_t ternary_chunks(uint32_t degree) { return (12u * degree + 4095u) / 4096u; }   // 12 bytes a coefficient
constexpr uint32_t binomial_chunks(uint32_t degree) { return (16u * degree + 4095u) / 4096u; }  // 16 bytes a coefficient
constexpr size_t kChainRecordBytes = 192;

// randomizeTernary (PolyRq+Randomize.swift:87-104): out [batch][L][N] Coeff, polynomial b at out + b * poly_stride,
// L = ctx.moduli_count.  chain: ternary_chunks(N) records per seed.
template <typename W>
hipError_t launch_sample_ternary(const uint32_t* chain, W* out, size_t poly_stride, const DeviceContext& ctx, size_t batch,
                                 hipStream_t stream);
// randomizeCenteredBinomialDistribution (PolyRq+Randomize.swift:120-167) at ErrorStdDev.stdDev32 (21 trial bits a side):
// out [batch][L][N] Coeff.  chain: binomial_chunks(N) records per seed.
template <typename W>
hipError_t launch_sample_centered_binomial(const uint32_t* chain, W* out, size_t poly_stride, const DeviceContext& ctx,
                                           size_t batch, hipStream_t stream);

// cts [batch][2][m][N] (m = ctx.moduli_count), `a` in polynomial 1, secret_key [>= m][N], both Eval: polynomial 0 = a s
template <typename W>
hipError_t launch_encrypt_mul_secret(W* cts, const W* secret_key, const DeviceContext& ctx, size_t batch, hipStream_t stream);
// The last step of Bfv.encryptZero in Coeff form (Bfv+Encrypt.swift:168-176): polynomial 0 of cts [batch][2][m][N] holds
// INTT(a s) and becomes -(INTT(a s) + e), e drawn from error_chain in registers (it never reaches memory).
template <typename W>
hipError_t launch_encrypt_finish_coeff(W* cts, const uint32_t* error_chain, const DeviceContext& ctx, size_t batch,
                                       hipStream_t stream);

// (q_ks mod q_j, Shoup factor) for the ciphertext moduli of a key-switch key (Bfv+Keys.swift:88-91)
constexpr uint32_t kMaxKeySwitchCiphertexts = 32;
struct KeySwitchFactors {
    U64x2 factor[kMaxKeySwitchCiphertexts];
};
// Bfv.encryptZero in Eval form: cts [count][2][m][N] with `a` in polynomial 1, error_eval [count][m][N] = NTT(e),
// secret_key [>= m][N]: polynomial 0 = -(a s + NTT(e)).
// current_keys != nullptr: Bfv._generateKeySwitchKey's last step as well -- ciphertext c belongs to key c / per_key and is
// its ciphertext j = c % per_key; row j of its polynomial 0 gains factors.factor[j] * current_keys[c / per_key][j]
// (current_keys [keys][m][N] Eval).
template <typename W>
hipError_t launch_encrypt_finish_eval(W* cts, const W* error_eval, const W* secret_key, const W* current_keys,
                                      uint32_t per_key, const KeySwitchFactors& factors, const DeviceContext& ctx, size_t count,
                                      hipStream_t stream);

// The current keys of evaluation-key generation from secret_key [m][N] Eval, m = ctx.moduli_count:
// s s (Bfv+Keys.swift:62) -> out [m][N], and applyGalois(s, elements[e]) (Bfv+Keys.swift:39) for `count` elements (a HOST
// array, each odd and below 2N) -> out [count][m][N], kGaloisElementsPerLaunch keys to a launch
template <typename W>
hipError_t launch_secret_key_square(const W* secret_key, W* out, const DeviceContext& ctx, hipStream_t stream);
constexpr size_t kGaloisElementsPerLaunch = 64;
struct GaloisElementTable {
    uint32_t element[kGaloisElementsPerLaunch];
};
template <typename W>
hipError_t launch_secret_key_galois(const W* secret_key, W* out, const DeviceContext& ctx, const uint64_t* elements, size_t count,
                                    hipStream_t stream);

}  // namespace heamd
