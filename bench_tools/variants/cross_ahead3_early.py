COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip"]
DESCRIPTION = "... three in flight, the inverse's first three requested before the row is loaded"
EDITS = [("ntt_interleaved.hpp", 'constexpr int kCrossAheadSplit = 1;', 'constexpr int kCrossAheadSplit = 3;'), ("ntt_interleaved.hpp", 'constexpr bool kCrossEarlySplit = false;', 'constexpr bool kCrossEarlySplit = true;')]
