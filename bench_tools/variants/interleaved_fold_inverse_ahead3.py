COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip"]
DESCRIPTION = "N = 16384 / 32768 on the shift-folded products: the inverse's cross stages with three twiddles in flight as the forward transform has (production: two; three keep 20 B of scratch)"
EDITS = [("ntt_interleaved.hpp", "constexpr int kCrossAheadInverse = MODE == kModeFoldLazy ? 2 :", "constexpr int kCrossAheadInverse = MODE == kModeFoldLazy ? 3 :")]
