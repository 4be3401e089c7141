COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]
DESCRIPTION = "N = 16384 / 32768: the BEHZ primes' rows on the [0, 8p) butterflies, as until round 6 (production: the fold butterflies of the plus form)"
EDITS = [("ntt_policy.hpp", "constexpr bool kFoldPlusInterleaved = true;", "constexpr bool kFoldPlusInterleaved = false;")]
