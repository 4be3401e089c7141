COMPILE = ["ntt_forward_8192.hip", "ntt_inverse_8192.hip"]
DESCRIPTION = "... one in flight, the inverse's first one requested before the row is loaded"
EDITS = [("ntt_interleaved.hpp", 'constexpr bool kCrossEarlySplit = false;', 'constexpr bool kCrossEarlySplit = true;')]
