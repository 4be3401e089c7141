DESCRIPTION = "the shift-folded butterflies with two twiddles in flight (production: three)"
EDITS = [("ntt_common.hpp", "template <int MODE>\nconstexpr int kTwiddlesAhead = is_fold_lazy(MODE) ? 3 : 1;", "template <int MODE>\nconstexpr int kTwiddlesAhead = is_fold_lazy(MODE) ? 2 : 1;")]
COMPILE = ["behz_kernels.hip", "ntt_forward_8192.hip", "ntt_generic.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip", "ntt_word32.hip"]
