COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]
DESCRIPTION = "N = 32768: the key-switching decomposition as its own kernel + plain forward transforms"
EDITS = [("ntt_policy.hpp", "constexpr bool kFusedSpreadAt32768 = true, kFusedKeyMacAt32768 = false;", "constexpr bool kFusedSpreadAt32768 = false, kFusedKeyMacAt32768 = false;")]
