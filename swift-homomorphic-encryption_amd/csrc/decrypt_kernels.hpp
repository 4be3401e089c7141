// decrypt_kernels.hpp -- launchers of decrypt_kernels.hip (asynchronous on `stream`): the secret-key dot product of
// Bfv.decrypt, the exact infinity norm behind Bfv.noiseBudget and Bfv.isTransparent, over ciphertexts resident in HBM.
// Each launcher is overloaded on the slab word (uint64_t, or uint32_t with every modulus <= 2^30 - 1); both read the
// 8-byte image of the level's context.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "device_context.hpp"

namespace heamd {

constexpr uint32_t kMaxDecryptPolys = 3;
constexpr uint32_t kMaxNoiseModuli = 16;  // mixed-radix digits a lane keeps in registers

// Bfv.dotProduct before its inverse transform (Bfv+Decrypt.swift:188-204): cts [batch][poly_count][L][N] Eval, secret_key
// [>= L][N] Eval (the first L = ctx.moduli_count rows are read, PolyRq.swift:184-194) -> out [batch][L][N] Eval =
// c0 + c1 s [+ c2 s^2], canonical.  poly_count 1..kMaxDecryptPolys.  Slabs that are 16-byte aligned move 16 bytes per lane.
// with_c0 = false (poly_count >= 2): cts holds [batch][poly_count - 1][L][N], the polynomials behind the first, and out =
// c1 s [+ c2 s^2] -- the part of Coeff-form input that has to be in Eval form.
hipError_t launch_secret_dot_product(const uint64_t* cts, const uint64_t* secret_key, uint64_t* out, const DeviceContext& ctx,
                                     uint32_t poly_count, bool with_c0, size_t batch, hipStream_t stream);
hipError_t launch_secret_dot_product(const uint32_t* cts, const uint32_t* secret_key, uint32_t* out, const DeviceContext& ctx,
                                     uint32_t poly_count, bool with_c0, size_t batch, hipStream_t stream);
// out [batch][L][N] += c0 of cts [batch][poly_count][L][N], both Coeff (the transform is linear: c0 needs none)
hipError_t launch_add_first_polynomial(const uint64_t* cts, uint64_t* out, const DeviceContext& ctx, uint32_t poly_count,
                                       size_t batch, hipStream_t stream);
hipError_t launch_add_first_polynomial(const uint32_t* cts, uint32_t* out, const DeviceContext& ctx, uint32_t poly_count,
                                       size_t batch, hipStream_t stream);

// What the norm kernel needs beside the context: t mod q_i as Shoup pairs, and (Q + 1) >> 1 in the kernel's mixed radix
// (digit i under q_i; digit 0 the most significant: x = e_{L-1} + q_{L-1} (e_{L-2} + q_{L-2} (... + q_1 e_0))).
struct NoiseNormTables {
    U64x2 t_mod_q[kMaxNoiseModuli];
    uint64_t half_digits[kMaxNoiseModuli];
    uint32_t limbs;  // ceil(bitlength(Q) / 64)
};
// dot [batch][L][N] Coeff -> out_limbs [batch][tables.limbs] little-endian: max_k |[t dot_k]_Q| centred as
// Bfv+Decrypt.swift:136-143 does.  L = ctx.moduli_count in 1..kMaxNoiseModuli (hipErrorNotSupported beyond).
hipError_t launch_noise_norm(const uint64_t* dot, uint64_t* out_limbs, const DeviceContext& ctx, const NoiseNormTables& tables,
                             size_t batch, hipStream_t stream);
hipError_t launch_noise_norm(const uint32_t* dot, uint64_t* out_limbs, const DeviceContext& ctx, const NoiseNormTables& tables,
                             size_t batch, hipStream_t stream);

// Bfv.isTransparent (Bfv+Encrypt.swift:48-62): out_flags[b] = 1 iff polynomials 1.. of ciphertext b are all zero (always 1
// for poly_count 1).  cts [batch][poly_count][rows][N].
hipError_t launch_is_transparent(const uint64_t* cts, uint8_t* out_flags, uint32_t log_degree, uint32_t rows, uint32_t poly_count,
                                 size_t batch, hipStream_t stream);
hipError_t launch_is_transparent(const uint32_t* cts, uint8_t* out_flags, uint32_t log_degree, uint32_t rows, uint32_t poly_count,
                                 size_t batch, hipStream_t stream);

}  // namespace heamd
