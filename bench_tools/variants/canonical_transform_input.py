COMPILE = ["behz_kernels.hip", "ntt_forward_8192.hip", "ntt_generic.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]  # the edited text lives in a header both include
DESCRIPTION = ("the fused inverse loads (tensor product, key MAC) reduce their words to [0, p) before the transform (rounds 2-4) "
               "instead of handing it the bounded reduction's remainder in [0, 5p)")
EDITS = [("ntt_rows.hpp", "constexpr bool kLazyTransformInput = is_split(MODE) || is_fold(MODE);",
          "constexpr bool kLazyTransformInput = false;")]
