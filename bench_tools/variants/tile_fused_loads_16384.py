COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]
DESCRIPTION = ("N = 16384: the fused-load transforms (decomposition, lift, Q band; tensor product, key MAC) on the 16-words-per-lane "
               "tile, one workgroup per CU, with the key switch's end in the key-MAC transform's store (rounds 2-4)")
EDITS = [("ntt_policy.hpp", "constexpr bool kInterleavedFusedLoads = true;", "constexpr bool kInterleavedFusedLoads = false;"),
         # the selector shapes ntt_routing.hip refers to under this constant, which the product does not instantiate
         ("ntt_forward_8192.hip", "\n}  // namespace heamd\n",
          "HEAMD_FORWARD_TILED(14, 10, kSourceLift, 1);\nHEAMD_FORWARD_TILED(14, 10, kSourceRows, 1);\n\n}  // namespace heamd\n"),
         ("ntt_inverse_8192.hip", "\n}  // namespace heamd\n",
          "HEAMD_INVERSE_TILED(14, 10, kInverseFromTensor, 1);\nHEAMD_INVERSE_TILED(14, 10, kInverseFromKeyMac, 1);\n\n}  // namespace heamd\n")]
