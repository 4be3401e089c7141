COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]
DESCRIPTION = ("the plain-slab inverse transform at N = 8192 in the signed form too (kModeSplitSigned, lane index re-derived), as the "
               "other limb-wise inverse kernels")
EDITS = [
    ("ntt_policy.hpp", "constexpr bool kSignedInverse = !(LOGN == 13 && (SOURCE == kInverseFromSlab || SOURCE == kInverseFromSlabScaled));",
     "constexpr bool kSignedInverse = true;"),
]
