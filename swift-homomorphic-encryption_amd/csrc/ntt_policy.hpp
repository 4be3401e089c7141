// ntt_policy.hpp -- the launch policy of the 8-byte NTT: every constant and trait that decides which kernel is instantiated
// or launched (butterfly form per shape and source, rows per workgroup, which degrees take the interleaved kernels and the
// fused loads), each with the measurement behind it, and the two kernel-body constants that more than one kernel unit reads.
// The kernel units instantiate by it and the routing layer (ntt_routing.hip) launches by it.
#pragma once

#include <hip/hip_runtime.h>

#include "device_context.hpp"
#include "ntt_common.hpp"
#include "ntt_rows.hpp"
#include "ntt_sources.hpp"

namespace heamd {
namespace ntt {

// ---- which butterflies ----------------------------------------------------------------------------------------------------
// Where the shift-folded products (ntt_common.hpp kModeFoldLazy) replace the limb-wise Shoup ones for launches whose moduli
// are all of the form 2^b - d (DeviceContext::shift_prefix): every kernel of the 8-words-per-lane shapes at N = 4096 / 8192 --
// plain slabs and the fused loads, both directions -- and the Q band of the row-fused ct x ct kernel (behz_kernels.hip); since
// round 6 the interleaved sub-rows of N = 16384 / 32768 too, where every modulus of the launch qualifies (at N = 16384 only the
// first two of the standard 55-bit primes do: with 4-register twiddles the cross stages keep three in flight and the inverse
// requests its first ones before the row's loads -- forward -4 %, inverse -3 % on two such moduli,
// profiles/r06p_fold_interleaved_eligible_moduli_ab.txt; round 5's "the same either way" was measured on a context that did
// not qualify).
template <int LOGN, int LOGT>
constexpr bool kFoldLazyForward = (LOGN == 12 && LOGT == 9) || (LOGN == 13 && LOGT == 10);
template <int LOGN, int LOGT, int SOURCE>
constexpr bool kFoldLazyInverse = (LOGN == 12 && LOGT == 9) || (LOGN == 13 && LOGT == 10);
constexpr bool kFoldLazyInterleaved = true;
// Where the signed form of those products (ntt_common.hpp kModeFoldSigned: one 64-bit addition less per butterfly) replaces them:
// the plain-slab pair at N = 8192, each direction on its own measurement
constexpr bool kFoldSignedForward = true, kFoldSignedInverse = true;
template <int LOGN, int LOGT, int SPREAD>
constexpr int kFoldLazyForwardMode =
    (kFoldSignedForward && LOGN == 13 && LOGT == 10 && SPREAD == kSourceSlab) ? kModeFoldSigned : kModeFoldLazy;
template <int LOGN, int LOGT, int SOURCE>
constexpr int kFoldLazyInverseMode =
    (kFoldSignedInverse && LOGN == 13 && LOGT == 10 && SOURCE == kInverseFromSlab) ? kModeFoldSigned : kModeFoldLazy;
// ... and the fold butterflies of the plus form (ntt_common.hpp kModeFoldPlus) for the BEHZ primes' rows of N = 16384 / 32768: the
// Bsk bands of ct x ct ran on the [0, 8p) butterflies there (0.38 / 0.27 of 8 TB/s forward / inverse at N = 16384 against the Q
// band's 0.54 / 0.35: profiles/r06q_fold_plus_interleaved.txt)
constexpr bool kFoldPlusInterleaved = true;
// every modulus of a launch is of the form 2^b - d (DeviceContext::shift_prefix)
inline bool fold_lazy_band(const DeviceContext& ctx, const RowMap& map) {
    return map.band_rows != 0 && map.mod_base + map.band_rows <= ctx.shift_prefix;
}
// Where the limb-wise inverse transform multiplies its differences as signed words (ntt_common.hpp kModeSplitSigned): the
// plain-slab transform at N = 8192 (partial pass on the top bits) is 2.5 % faster in the unsigned form, N = 4096 1.8 % and the
// interleaved rows of N = 16384 3.3 % faster in the signed one, the key-MAC transforms 1.9 % (profiles/r04t_inverse_forms_ab.txt).
template <int LOGN, int SOURCE>
constexpr bool kSignedInverse = !(LOGN == 13 && (SOURCE == kInverseFromSlab || SOURCE == kInverseFromSlabScaled));
// the limb-wise butterflies of the interleaved inverse: the signed difference (ntt_common.hpp kModeSplitSigned; N = 16384 -3.9 %,
// profiles/r04t_inverse_forms_ab.txt)
constexpr int kInterleavedInverseSplit = kModeSplitSigned;

// ---- rows per workgroup ---------------------------------------------------------------------------------------------------
// Row pairs: where the register file allows it (8 words per lane), a workgroup transforms the same band row of two
// consecutive records -- one modulus, every twiddle fetched once for both.
constexpr int kRowGroup = 2;
// ... unless the launch is small: below a few rows per workgroup slot (256 CUs x 2 workgroups of 64 registers) a pair only
// doubles the launch's latency -- the levels of a query's expansion and key switches on a few ciphertexts are chains of such
// launches.  Measured (profiles/r06w_small_launches.txt): one query's expansion to 320 ciphertexts 1.078 -> 0.898 ms,
// relinearize on 8 / 64 ciphertexts 67.7 -> 45.5 / 133 -> 114 us; from 8192 rows up the pairs win (the key MAC of 1024
// ciphertexts -1.3 %, the headline transform's 16384 rows -6 % without them).
constexpr size_t kUngroupedBelowRows = 4096;
template <int LOGN, int LOGT>
constexpr int kRowsPerWorkgroup = (LOGN - LOGT <= 3 && Schedule<LOGN, LOGN - LOGT>::P >= 2) ? kRowGroup : 1;

// Which two rows a key-MAC workgroup takes where the register file holds two: the same key column of two consecutive
// polynomials, the other column in a sibling workgroup of the same XCD.  The counters read 1.7 x the spread slab for this
// kernel (profiles/r03z_pmc_traffic_per_kernel.txt), which suggested pairing the two COLUMNS of one polynomial instead
// (every spread word fetched once).  Measured both ways and dropped: with per-word sums (8-byte loads at a 16-byte lane
// stride, twice the load instructions) relinearize 727 -> 671 k/s (profiles/r04j_keymac_loads_and_column_words_ab.txt,
// the variant lived under bench_tools/variants/ until round 4, commit 006a646); with the two columns summed one after the other through the same 16-byte
// loads 723 -> 708 k/s
// (profiles/r04c_keymac_columns_in_turn_ab.txt).  The slab's re-reads come out of L2 / the memory-side cache; they are not
// what binds the kernel.
// Rows per workgroup of the fused-load inverse kernels.  The tensor load gains nothing from a second row (the three
// workgroups of a replica set already gather the same twiddles side by side; profiles/r02i_c3_fused_row_groups.txt,
// r03j_c3_fused_row_groups.txt).  The key MAC does since its load is a rolled loop over the terms with the next term
// requested ahead -- two rows then cost 20 bytes of scratch per lane instead of the 104 of the unrolled
// carry-counting form that lost 6 % in round 2: relinearize 638 -> 659 k/s.  (The fused FORWARD loads -- spread, lift --
// are plain row loads and run two rows per workgroup: relinearize +7 %, convertToEvalFormat +21 %.)
constexpr int kTensorRowGroup = 1, kKeyMacRowGroup = 2;
template <int LOGN, int LOGT>
constexpr int kTensorRows = kRowsPerWorkgroup<LOGN, LOGT> > 1 ? kTensorRowGroup : 1;
template <int LOGN, int LOGT>
constexpr int kKeyMacRows = kRowsPerWorkgroup<LOGN, LOGT> > 1 ? kKeyMacRowGroup : 1;

// ---- interleaved kernels and fused loads per degree -----------------------------------------------------------------------
// Interleaved launches (ntt_forward_interleaved / ntt_inverse_interleaved): one workgroup per row of 2^(13 + LOGS) words.
// N = 16384 takes them for plain slabs instead of the streamed rows (profiles/r03p_ntt_interleaved.txt); N = 32768 has no
// other tiled kernel.  Round 5: the fused loads at N = 16384 (key-switching decomposition, plaintext lift, the Q band of the
// lifted records into the forward transform; tensor product and key inner product into the inverse one) take the same form
// -- two workgroups per CU at 64 registers instead of the 16-words-per-lane tile at one (kInterleavedFusedLoads).
constexpr bool kInterleaved16384 = true;
constexpr bool kInterleavedFusedLoads = true;
// The largest degree whose pipelines take the fused loads (2^15: as four interleaved sub-rows, round 5; 14: N = 32768 runs its
// pipelines unfused over the plain interleaved transforms, rounds 3-4)
constexpr uint32_t kMaxFusedLoadLogDegree = 15;
// ... of which, at N = 32768, the key switch's two are decided on their own measurements (128 pairs, L = 6,
// profiles/r05p_fused_loads_32768_ab.txt): the decomposition into the forward transform gains (relinearize 50.5 -> 62.4 k/s),
// the key inner product into the inverse one -- a rolled loop over the terms in a 128-register workgroup that is alone on its
// CU -- loses (40.5 k/s with both, 34.9 k/s with it alone) and stays a kernel of its own in front of the plain transforms
constexpr bool kFusedSpreadAt32768 = true, kFusedKeyMacAt32768 = false;
// N = 16384: the key inner product as a kernel of its own in front of the plain interleaved inverse transforms, then the finish
// kernel: 163.3 k relinearize/s at L = 6 against 157.4 k with the q_ks row's MAC fused into the interleaved inverse and the other
// rows on the 16-words-per-lane tile with the fused end (profiles/r05s_keymac_16384_ab.txt) -- a fused load pays where its kernel
// has a second workgroup on the CU to run under it (N = 4096 / 8192), not where the workgroup is alone
constexpr bool kFusedKeyMacAt16384 = false;
// (the key MAC's rows r < L stay on the 16-words-per-lane tile, whose store carries the key switch's end: interleaved sub-rows
// plus the separate finish kernel measured 134.9 k relinearize/s at N = 16384, L = 6 against 157.8 k this way and 143.7 k with
// every fused load on the tile -- profiles/r05f_fused_loads_16384_ab.txt; the q_ks row and the other fused loads are interleaved)
constexpr bool kInterleavedKeyMacAt16384 = false;

// ---- kernel-body constants read by more than one kernel unit --------------------------------------------------------------
constexpr bool kKeyMacBoundedReduce = true;
// How many twiddles of the first (gather-heavy) pass are requested before the rows are loaded and then kept in flight
// through that pass (inverse_row_head).  1: the first one only, requested once the rows are in (the schedule of rounds 2-3, and
// of every limb-wise kernel: their twiddles are 6 registers each).  The plain-slab transform on the shift-folded products
// (4 registers per twiddle, 62 of its 64 in use) takes three: -2.9 % at N = 8192 (two: -2.0 %; four spill: +7.7 %;
// profiles/r05ao_inverse_head_twiddles_ab.txt) -- with no gathers at all the kernel would be 12 % faster (r05an).
template <int LOGN, int LOGE, int MODE, int SOURCE, int ROWS>
constexpr int kInverseHeadTwiddles = (is_fold_lazy(MODE) && SOURCE == 0) ? 3 : 1;

}  // namespace ntt
}  // namespace heamd
