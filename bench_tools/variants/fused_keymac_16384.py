COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]
DESCRIPTION = ("N = 16384: the q_ks row's key inner product fused into the interleaved inverse transform, the other rows on the "
               "16-words-per-lane tile with the key switch's end in its store (the first form of round 5)")
EDITS = [("ntt_policy.hpp", "constexpr bool kFusedKeyMacAt16384 = false;", "constexpr bool kFusedKeyMacAt16384 = true;"),
         # the selector shapes ntt_routing.hip refers to under this constant, which the product does not instantiate
         ("ntt_inverse_8192.hip", "\n}  // namespace heamd\n",
          "HEAMD_INVERSE_TILED(14, 10, kInverseFromKeyMacFinish, 1);\nHEAMD_INTERLEAVED_INVERSE(1, kInverseFromKeyMac);\n\n}  // namespace heamd\n")]
