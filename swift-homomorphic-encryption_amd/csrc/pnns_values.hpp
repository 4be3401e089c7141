// pnns_values.hpp -- how a signed value of a PlaintextMatrix becomes a residue mod t (PlaintextMatrix.swift:172-181), for the
// packing kernels of pnns_kernels.hip (diagonal) and pnns_client_kernels.hip (dense row).
#pragma once

#include <hip/hip_runtime.h>

namespace heamd {

// reduce: Modulus.reduce(SignedScalar), the remainder in [0, t).  Otherwise centeredToRemainder; a value outside
// [-(t >> 1), (t - 1) >> 1] sets `outside` (the reference's precondition) and its residue is unspecified.
__device__ __forceinline__ unsigned long long pnns_signed_to_residue(long long v, long long t, bool reduce, bool& outside) {
    if (reduce) {
        v %= t;
        if (v < 0) v += t;
    } else {
        outside |= v > ((t - 1) >> 1) || v < -(t >> 1);
        if (v < 0) v += t;
    }
    return static_cast<unsigned long long>(v);
}

}  // namespace heamd
