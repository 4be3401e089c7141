COMPILE = ["behz_kernels.hip", "ntt_forward_8192.hip", "ntt_generic.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]  # the edited text lives in a header both include
DESCRIPTION = ("the first twiddle of every inverse pass on the limb-wise butterflies requested BEFORE the exchange that feeds "
               "the pass (with late lane addresses: 12 B of scratch in the plain-slab kernel instead of 0)")
EDITS = [("ntt_rows.hpp", "template <int MODE>\nconstexpr bool kInverseFirstTwiddleEarly = false;",
          "template <int MODE>\nconstexpr bool kInverseFirstTwiddleEarly = MODE == kModeSplit;")]
