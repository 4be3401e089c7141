COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]
DESCRIPTION = "plain-slab inverse transform on the shift-folded products: one twiddle of the first pass requested behind the row loads (production: three, before them)"
EDITS = [("ntt_policy.hpp", "constexpr int kInverseHeadTwiddles = (is_fold_lazy(MODE) && SOURCE == 0) ? 3 : 1;", "constexpr int kInverseHeadTwiddles = 1;")]
