DESCRIPTION = "the fold-at-2^(b+2) butterflies with one twiddle in flight like the limb-wise form (production: three -- a twiddle is 4 registers there, not 6)"
EDITS = [("ntt_common.hpp", "template <int MODE>\nconstexpr int kTwiddlesAhead = is_fold_lazy(MODE) ? 3 : 1;", "template <int MODE>\nconstexpr int kTwiddlesAhead = 1;")]
COMPILE = ["behz_kernels.hip", "ntt_forward_8192.hip", "ntt_generic.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip", "ntt_word32.hip"]
