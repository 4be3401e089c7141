COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]
DESCRIPTION = "N = 32768: the ct x ct / key-switching pipelines unfused over the plain interleaved transforms (rounds 3-4)"
EDITS = [("ntt_policy.hpp", "constexpr uint32_t kMaxFusedLoadLogDegree = 15;", "constexpr uint32_t kMaxFusedLoadLogDegree = 14;")]
