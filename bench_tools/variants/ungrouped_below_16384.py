COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]
DESCRIPTION = "launches of at most 16384 rows go one row per workgroup: the headline batch without its row pairs (production: 4096)"
EDITS = [("ntt_policy.hpp", "constexpr size_t kUngroupedBelowRows = 4096;", "constexpr size_t kUngroupedBelowRows = 16384;")]
