COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]
DESCRIPTION = "row pairs per workgroup at every launch size (production: launches of at most 4096 rows go one row per workgroup)"
EDITS = [("ntt_policy.hpp", "constexpr size_t kUngroupedBelowRows = 4096;", "constexpr size_t kUngroupedBelowRows = 0;")]
