COMPILE = ["behz_kernels.hip", "ntt_forward_8192.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]
DESCRIPTION = "every transform of moduli 2^b - d on the limb-wise Shoup butterflies (8 multiply-adds, tabulated factors; the inverse in its signed form) instead of the fold-at-2^(b+2) ones -- the tree before r05ad"
EDITS = [
    ("ntt_policy.hpp", "constexpr bool kFoldLazyForward = (LOGN == 12 && LOGT == 9) || (LOGN == 13 && LOGT == 10);", "constexpr bool kFoldLazyForward = false;"),
    ("ntt_policy.hpp", "constexpr bool kFoldLazyInverse = (LOGN == 12 && LOGT == 9) || (LOGN == 13 && LOGT == 10);", "constexpr bool kFoldLazyInverse = false;"),
    ("behz_kernels.hip", "constexpr bool kBehzFoldLazy = true;", "constexpr bool kBehzFoldLazy = false;"),
]
