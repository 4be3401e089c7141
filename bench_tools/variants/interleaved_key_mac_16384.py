COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]
DESCRIPTION = ("N = 16384: the key MAC as interleaved sub-rows + the separate finish kernel instead of the 16-words-per-lane tile with "
               "the key switch's end in its store")
EDITS = [("ntt_policy.hpp", "constexpr bool kInterleavedKeyMacAt16384 = false;", "constexpr bool kInterleavedKeyMacAt16384 = true;"),
         ("ntt_policy.hpp", "constexpr bool kFusedKeyMacAt16384 = false;", "constexpr bool kFusedKeyMacAt16384 = true;"),
         # the selector shapes ntt_routing.hip refers to under these constants, which the product does not instantiate
         ("ntt_inverse_8192.hip", "\n}  // namespace heamd\n",
          "HEAMD_INVERSE_TILED(14, 10, kInverseFromKeyMacFinish, 1);\nHEAMD_INTERLEAVED_INVERSE(1, kInverseFromKeyMac);\n\n}  // namespace heamd\n")]
