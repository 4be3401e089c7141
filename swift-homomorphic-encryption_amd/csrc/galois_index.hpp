// galois_index.hpp -- the index arithmetic of PolyRq<Eval>.applyGalois (PolyRq/Galois.swift:153-168, GaloisEvalIterator
// :81-92), shared by the kernels that permute Eval rows: galois_kernels.hip (polynomials) and encrypt_kernels.hip (the rotated
// secret keys of Galois-key generation).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace heamd {

// Output word i of an Eval (bit-reversed) row of 2^logn words takes input word
// bitrev_logn(((element * bitrev_{logn+1}(i + N)) >> 1) mod N)
__device__ __forceinline__ uint32_t galois_eval_source(uint32_t i, uint32_t logn, uint32_t element) {
    const uint32_t n = 1u << logn;
    const uint32_t reversed = __brev(i + n) >> (32 - (logn + 1));
    const uint32_t raw = ((element * reversed) >> 1) & (n - 1);
    return logn == 0 ? 0 : __brev(raw) >> (32 - logn);
}

}  // namespace heamd
