DESCRIPTION = "the shift-folded butterflies with two twiddles in flight (production: three)"
EDITS = [("ntt_common.hpp", "template <int MODE>\nconstexpr int kTwiddlesAhead = is_fold_lazy(MODE) ? 3 : 1;", "template <int MODE>\nconstexpr int kTwiddlesAhead = is_fold_lazy(MODE) ? 2 : 1;")]
COMPILE = ["ntt_kernels.hip", "behz_kernels.hip"]
