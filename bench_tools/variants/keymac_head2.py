COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]
DESCRIPTION = "key-MAC inverse transforms on the shift-folded products: 2 twiddles of the first pass requested before the inner product's loads (production: one, behind them)"
EDITS = [("ntt_policy.hpp", "constexpr int kInverseHeadTwiddles = (is_fold_lazy(MODE) && SOURCE == 0) ? 3 : 1;", "constexpr int kInverseHeadTwiddles = (is_fold_lazy(MODE) && SOURCE == 0) ? 3 : (MODE == kModeFoldLazy && (SOURCE == 2 || SOURCE == 4)) ? 2 : 1;")]
