// ntt_inverse_8192.hip -- the inverse kernels built on the 8192-word row: tiled N = 8192 with every fused source, the tiled
// N = 16384 slab forms (which no launch reaches -- launch_tiled takes the interleaved kernels first -- but its template
// names: kept for unoptimised builds and so that the set of kernels is the single unit's), and N = 16384 / 32768 as
// interleaved sub-rows of 8192 words.  The shapes ntt_routing.hip refers to, one family after the other.
#include "ntt_inverse_tiled.hpp"
#include "ntt_interleaved.hpp"

namespace heamd {

HEAMD_INVERSE_TILED(13, 10, kInverseFromSlabScaled, 1);
HEAMD_INVERSE_TILED(13, 10, kInverseFromKeyMacFinish, 2);
HEAMD_INVERSE_TILED(13, 10, kInverseFromKeyMacFinish, 1);
HEAMD_INVERSE_TILED(13, 10, kInverseFromTensor, 1);
HEAMD_INVERSE_TILED(13, 10, kInverseFromKeyMac, 2);
HEAMD_INVERSE_TILED(13, 10, kInverseFromKeyMac, 1);
HEAMD_INVERSE_TILED(13, 10, kInverseFromSlab, 2);
HEAMD_INVERSE_TILED(13, 10, kInverseFromSlab, 1);
HEAMD_INVERSE_TILED(13, 9, kInverseFromSlab, 1);
HEAMD_INVERSE_TILED(14, 10, kInverseFromSlabScaled, 1);
HEAMD_INVERSE_TILED(14, 10, kInverseFromSlab, 1);
HEAMD_INTERLEAVED_INVERSE(1, kInverseFromSlab);
HEAMD_INTERLEAVED_INVERSE(1, kInverseFromTensor);
HEAMD_INTERLEAVED_INVERSE(2, kInverseFromTensor);
HEAMD_INTERLEAVED_INVERSE(2, kInverseFromSlab);

}  // namespace heamd
