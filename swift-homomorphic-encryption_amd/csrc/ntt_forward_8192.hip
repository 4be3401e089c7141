// ntt_forward_8192.hip -- the forward kernels built on the 8192-word row: tiled N = 8192, the tiled N = 16384 kernels that are
// left (the automorphism's row permutation; the slab form, which no launch reaches but launch_tiled's template names), and N = 16384 / 32768 as interleaved sub-rows of
// 8192 words.  The shapes ntt_routing.hip refers to, one family after the other.
#include "ntt_forward_tiled.hpp"
#include "ntt_interleaved.hpp"

namespace heamd {

HEAMD_FORWARD_TILED(13, 10, kSourceSpread, 2);
HEAMD_FORWARD_TILED(13, 10, kSourceSpread, 1);
HEAMD_FORWARD_TILED(14, 10, kSourceSpread, 1);
HEAMD_FORWARD_TILED(13, 10, kSourceLift, 2);
HEAMD_FORWARD_TILED(13, 10, kSourceLift, 1);
HEAMD_FORWARD_TILED(13, 10, kSourceSlab, 2);
HEAMD_FORWARD_TILED(13, 10, kSourceSlab, 1);
HEAMD_FORWARD_TILED(14, 10, kSourceSlab, 1);
HEAMD_FORWARD_TILED(13, 10, kSourceRows, 2);
HEAMD_FORWARD_TILED(13, 10, kSourceRows, 1);
HEAMD_FORWARD_TILED(13, 9, kSourceSlab, 1);
HEAMD_INTERLEAVED_FORWARD(1, kSourceSpread);
HEAMD_INTERLEAVED_FORWARD(2, kSourceSpread);
HEAMD_INTERLEAVED_FORWARD(1, kSourceLift);
HEAMD_INTERLEAVED_FORWARD(2, kSourceLift);
HEAMD_INTERLEAVED_FORWARD(1, kSourceSlab);
HEAMD_INTERLEAVED_FORWARD(2, kSourceSlab);
HEAMD_INTERLEAVED_FORWARD(1, kSourceRows);
HEAMD_INTERLEAVED_FORWARD(2, kSourceRows);

}  // namespace heamd
