COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]
DESCRIPTION = "N = 32768: the key inner product fused into the interleaved inverse transform's load (four sub-rows, one workgroup per CU)"
EDITS = [("ntt_policy.hpp", "constexpr bool kFusedSpreadAt32768 = true, kFusedKeyMacAt32768 = false;", "constexpr bool kFusedSpreadAt32768 = true, kFusedKeyMacAt32768 = true;"),
         # the selector shape ntt_routing.hip refers to under this constant, which the product does not instantiate
         ("ntt_inverse_8192.hip", "\n}  // namespace heamd\n", "HEAMD_INTERLEAVED_INVERSE(2, kInverseFromKeyMac);\n\n}  // namespace heamd\n")]
