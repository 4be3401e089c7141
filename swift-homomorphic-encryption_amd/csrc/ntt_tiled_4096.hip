// ntt_tiled_4096.hip -- the tiled kernels of N = 4096, both directions (their passes share the helpers of the 4096-word row):
// the shapes ntt_routing.hip refers to (launch_forward_tiled, launch_tiled, launch_fused_inverse there), one family after the other.
// 8 words per lane with every row source; 16 words per lane (test variant) from the slab.
#include "ntt_forward_tiled.hpp"
#include "ntt_inverse_tiled.hpp"

namespace heamd {

HEAMD_FORWARD_TILED(12, 9, kSourceSpread, 2);
HEAMD_FORWARD_TILED(12, 9, kSourceSpread, 1);
HEAMD_FORWARD_TILED(12, 9, kSourceLift, 2);
HEAMD_FORWARD_TILED(12, 9, kSourceLift, 1);
HEAMD_FORWARD_TILED(12, 9, kSourceSlab, 2);
HEAMD_FORWARD_TILED(12, 9, kSourceSlab, 1);
HEAMD_FORWARD_TILED(12, 9, kSourceRows, 2);
HEAMD_FORWARD_TILED(12, 9, kSourceRows, 1);
HEAMD_FORWARD_TILED(12, 8, kSourceSlab, 1);
HEAMD_INVERSE_TILED(12, 9, kInverseFromSlabScaled, 1);
HEAMD_INVERSE_TILED(12, 9, kInverseFromKeyMacFinish, 2);
HEAMD_INVERSE_TILED(12, 9, kInverseFromKeyMacFinish, 1);
HEAMD_INVERSE_TILED(12, 9, kInverseFromTensor, 1);
HEAMD_INVERSE_TILED(12, 9, kInverseFromKeyMac, 2);
HEAMD_INVERSE_TILED(12, 9, kInverseFromKeyMac, 1);
HEAMD_INVERSE_TILED(12, 9, kInverseFromSlab, 2);
HEAMD_INVERSE_TILED(12, 9, kInverseFromSlab, 1);
HEAMD_INVERSE_TILED(12, 8, kInverseFromSlab, 1);

}  // namespace heamd
