DESCRIPTION = ("the plain-slab pair at N = 8192 on the unsigned shift-folded butterflies (kModeFoldLazy: x + B - r, one 64-bit addition "
               "more per butterfly; the inverse folds its sums once instead of twice) instead of the signed ones (kModeFoldSigned) -- "
               "the tree before the signed products")
EDITS = [
    ("ntt_kernels.hip", "constexpr bool kFoldSignedForward = true, kFoldSignedInverse = true;",
     "constexpr bool kFoldSignedForward = false, kFoldSignedInverse = false;"),
]
