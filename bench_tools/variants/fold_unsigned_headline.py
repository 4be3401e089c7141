COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip", "ntt_routing.hip", "ntt_tiled_4096.hip"]
DESCRIPTION = ("the plain-slab pair at N = 8192 on the unsigned shift-folded butterflies (kModeFoldLazy: x + B - r, one 64-bit addition "
               "more per butterfly; the inverse folds its sums once instead of twice) instead of the signed ones (kModeFoldSigned) -- "
               "the tree before the signed products")
EDITS = [
    ("ntt_policy.hpp", "constexpr bool kFoldSignedForward = true, kFoldSignedInverse = true;",
     "constexpr bool kFoldSignedForward = false, kFoldSignedInverse = false;"),
]
