COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]
DESCRIPTION = "launches of at most 512 rows go one row per workgroup -- one row per workgroup slot of the chip (production: 4096)"
EDITS = [("ntt_policy.hpp", "constexpr size_t kUngroupedBelowRows = 4096;", "constexpr size_t kUngroupedBelowRows = 512;")]
