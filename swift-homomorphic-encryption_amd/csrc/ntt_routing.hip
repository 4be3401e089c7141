// ntt_routing.hip -- batched negacyclic NTT over the (batch x moduli x N) slab, hand-written for gfx950: the design notes of
// the NTT units, the routing from a request to kernel launches, and the public launchers of kernels.hpp.
//
// Computes exactly what _NttContext.forwardNtt / inverseNtt compute (reference
// Sources/HomomorphicEncryption/PolyRq/PolyRq+Ntt.swift:237-319, 379-483): Cooley-Tukey, natural order in ->
// bit-reversed order out (forward); Gentleman-Sande, bit-reversed in -> natural out with N^-1 folded into the last
// stage (inverse); all outputs canonical.  The lazy-reduction *schedule* is ours (only canonical words are
// observable).
//
// Mapping to the machine (DESIGN.md "NTT kernel"):
//   * one workgroup per residue row; a row of N = 2^LOGN words is held entirely in registers, E = N / T words per
//     lane (T = 2^LOGT lanes), and is touched in HBM exactly once in and once out (buffer loads / stores: one 32-bit
//     lane offset, scalar row offsets -- no 64-bit address arithmetic on the vector ALU);
//   * log2(N) radix-2 stages are grouped into passes of LOGE stages executed on registers; between passes the row
//     is transposed through a padded LDS tile (4 transposes for N = 8192 with 8 words per lane: 13 = 3+3+3+3+1, the
//     one-stage pass on bit 0 or -- the plain-slab inverse -- on bit 12: ntt_rows.hpp kTopPartialOrder);
//   * twiddles of the first two passes are wave-uniform (scalar loads); later passes gather them from the L2-resident
//     per-modulus tables, shared by every workgroup of that modulus;
//   * butterflies: limb-wise Shoup products for the usual <= 55-bit moduli (ntt_common.hpp kModeSplit), products folded
//     by a shift for larger moduli next to a power of two (kModeFoldMinus / kModeFoldPlus: the 60-bit parameter sets, the
//     BEHZ auxiliary primes), Harvey butterflies with a 3- or 4-multiply quotient for the other moduli up to 2^61 / 2^62;
//   * N = 16384 / 32768: the row as 2 / 4 interleaved sub-rows of 8192 words through the same machinery
//     (ntt_forward_interleaved / ntt_inverse_interleaved, ntt_interleaved.hpp).
//
// The files: ntt_sources.hpp (row-source descriptors); ntt_policy.hpp (every constant that decides which kernel is instantiated or
// launched); one header per kernel family with the selector that names its kernels -- ntt_forward_tiled.hpp, ntt_inverse_tiled.hpp,
// ntt_interleaved.hpp; the units that compile them, grouped by the sub-transform whose helpers the kernels share --
// ntt_tiled_4096.hip, ntt_forward_8192.hip, ntt_inverse_8192.hip -- and ntt_generic.hip; and this unit, which reaches them through
// ntt_selectors.hpp only: it contains no __global__ function and names no kernel.
#include <hip/hip_runtime.h>

#include "device_context.hpp"
#include "kernels.hpp"
#include "ntt_common.hpp"
#include "ntt_policy.hpp"
#include "ntt_rows.hpp"
#include "ntt_selectors.hpp"
#include "ntt_sources.hpp"

namespace heamd {

namespace {

using namespace ntt;

template <int LOGS>
hipError_t launch_interleaved(bool inverse, int mode, uint64_t* slab, const DeviceContext& ctx, const RowMap& map, size_t rows,
                              hipStream_t stream) {
    if (!inverse) return launch_interleaved_forward<LOGS, kSourceSlab>(mode, slab, ctx, map, rows, {}, stream);
    return launch_interleaved_inverse<LOGS, kInverseFromSlab>(mode, slab, ctx, map, rows, {}, stream);
}

template <int LOGN, int LOGT, int SPREAD>
hipError_t launch_forward_tiled(int mode, uint64_t* slab, const DeviceContext& ctx, uint32_t mod_base,
                                uint32_t mod_period, size_t rows, const SpreadSource& spread, hipStream_t stream,
                                uint32_t row_period = 0, uint32_t row_offset = 0) {
    constexpr bool INTERLEAVED = LOGN == 14 && LOGT == 10 && SPREAD != kSourceSlab && kInterleavedFusedLoads;
    if constexpr (INTERLEAVED && SPREAD != kSourceSpread) {
        // as two interleaved sub-rows (the tile kernel of this source is not instantiated)
        return launch_interleaved_forward<1, SPREAD>(mode, slab, ctx, make_row_map(mod_base, mod_period, row_period, row_offset), rows,
                                                     spread, stream);
    } else {
        if constexpr (INTERLEAVED) {
            // (the automorphism of a Galois key switch permutes whole rows through the tile: the tiled kernel below)
            if (spread.galois_inverse == 0)
                return launch_interleaved_forward<1, SPREAD>(mode, slab, ctx, make_row_map(mod_base, mod_period, row_period, row_offset),
                                                             rows, spread, stream);
        }
        size_t paired_records = 0;  // records covered by the launch of row groups
        constexpr int GROUP = kRowsPerWorkgroup<LOGN, LOGT>;
        if constexpr (GROUP > 1) {
            paired_records = rows <= kUngroupedBelowRows ? 0 : (rows / mod_period) / GROUP * GROUP;
            if (paired_records != 0) {
                hipError_t e = launch_forward_kernel<LOGN, LOGT, SPREAD, GROUP>(
                    mode, slab, ctx, make_row_map(mod_base, mod_period, row_period, row_offset),
                    paired_records / GROUP * mod_period, spread, stream);
                if (e != hipSuccess) return e;
            }
        }
        const size_t rest = rows - paired_records * mod_period;
        if (rest == 0) return hipSuccess;
        return launch_forward_kernel<LOGN, LOGT, SPREAD, 1>(
            mode, slab, ctx, make_row_map(mod_base, mod_period, row_period, row_offset, static_cast<uint32_t>(paired_records)),
            rest, spread, stream);
    }
}

// One fused inverse source over records (item, c): groups of consecutive ITEMS share a workgroup (same c, same band row); the
// odd items at the end go one per workgroup.  record_base counts items for these kernels.
template <int LOGN, int LOGT, int SOURCE>
hipError_t launch_fused_inverse(int mode, uint64_t* slab, const DeviceContext& ctx, uint32_t mod_base, uint32_t mod_period,
                                size_t rows, uint32_t row_period, uint32_t row_offset, const InverseSource& source_spec,
                                hipStream_t stream) {
    constexpr bool TENSOR = SOURCE == kInverseFromTensor;
    constexpr size_t REPLICAS = TENSOR ? 3 : 2;
    constexpr int GROUP = TENSOR ? kTensorRows<LOGN, LOGT> : kKeyMacRows<LOGN, LOGT>;
    const size_t items = rows / mod_period / REPLICAS;
    const size_t grouped = (GROUP > 1 && rows > kUngroupedBelowRows) ? items / GROUP * GROUP : 0;
    auto map_from = [&](size_t first_item) {
        return make_row_map(mod_base, mod_period, row_period, row_offset, static_cast<uint32_t>(first_item));
    };
    if constexpr (GROUP > 1) {
        if (grouped != 0) {
            hipError_t e = launch_inverse_kernel<LOGN, LOGT, SOURCE, GROUP>(mode, slab, ctx, map_from(0),
                                                                            grouped / GROUP * REPLICAS * mod_period, source_spec, stream);
            if (e != hipSuccess) return e;
        }
    }
    if (items == grouped) return hipSuccess;
    return launch_inverse_kernel<LOGN, LOGT, SOURCE, 1>(mode, slab, ctx, map_from(grouped), (items - grouped) * REPLICAS * mod_period,
                                                        source_spec, stream);
}

template <int LOGN, int LOGT>
hipError_t launch_tiled(bool inverse, int mode, uint64_t* slab, const DeviceContext& ctx, uint32_t mod_base,
                        uint32_t mod_period, size_t rows, hipStream_t stream, uint32_t row_period = 0,
                        uint32_t row_offset = 0, int source = kInverseFromSlab,
                        const InverseSource& source_spec = {}) {
    if constexpr (LOGN == 14 && LOGT == 10 && kInterleaved16384) {
        if (source == kInverseFromSlab || !inverse)
            return launch_interleaved<1>(inverse, mode, slab, ctx, make_row_map(mod_base, mod_period, row_period, row_offset),
                                         rows, stream);
    }
    if (!inverse) {
        return launch_forward_tiled<LOGN, LOGT, kSourceSlab>(mode, slab, ctx, mod_base, mod_period, rows, {}, stream, row_period, row_offset);
    }
    constexpr int LOGE = LOGN - LOGT;
    if (source != kInverseFromSlab && (row_period == 0 || Schedule<LOGN, LOGE>::P == 1)) return hipErrorInvalidValue;
    const RowMap map = make_row_map(mod_base, mod_period, row_period, row_offset);
    // The fused loads and the scaled contexts of dropExtendedBase exist for the PRODUCTION shape of each degree only (8 words
    // per lane; N = 16384: 16): the 16- and 32-words-per-lane shapes are test variants of the plain transform
    // (kNttVariantWide, public contexts only) -- instantiating every source for them was a hundred kernels
    // nobody could launch, the exact-mode ones among them with their register tile in scratch.
    constexpr bool FUSED_SHAPE = (LOGN == 12 && LOGT == 9) || (LOGN == 13 && LOGT == 10) || (LOGN == 14 && LOGT == 10);
    if constexpr (!FUSED_SHAPE) {
        if (source != kInverseFromSlab || ctx.scaled_inverse_degree != 0) return hipErrorInvalidValue;
    } else {
        if (ctx.scaled_inverse_degree != 0) {
            if (is_key_mac(source)) return hipErrorInvalidValue;  // the key-switching contexts are never scaled
            if (source == kInverseFromSlab)
                return launch_inverse_kernel<LOGN, LOGT, kInverseFromSlabScaled, 1>(mode, slab, ctx, map, rows, source_spec, stream);
        } else if (source == kInverseFromTensor) {
            return hipErrorInvalidValue;  // the fused tensor load belongs to dropExtendedBase (t N^-1)
        }
    }
    constexpr int GROUP = kRowsPerWorkgroup<LOGN, LOGT>;
    if constexpr (LOGN == 14 && LOGT == 10 && kInterleavedFusedLoads) {
        // tensor product / key inner product into the interleaved inverse: one record (item, c) per workgroup; the key switch's
        // fused end (kInverseFromKeyMacFinish) is not offered at this degree (ntt_key_mac_finish_supported)
        if (source == kInverseFromTensor)
            return launch_interleaved_inverse<1, kInverseFromTensor>(mode, slab, ctx, map, rows, source_spec, stream);
        if constexpr (kFusedKeyMacAt16384) {
            if (source == kInverseFromKeyMac)
                return launch_interleaved_inverse<1, kInverseFromKeyMac>(mode, slab, ctx, map, rows, source_spec, stream);
        }
    }
    if constexpr (FUSED_SHAPE) {
        // (N = 16384 with the interleaved fused loads: only the key switch's fused end is left to the tile -- the others are
        // not instantiated for it)
        constexpr bool ONLY_FINISH = LOGN == 14 && kInterleavedFusedLoads;
        if constexpr (LOGN != 14 || kFusedKeyMacAt16384) {
            if (source == kInverseFromKeyMacFinish)
                return launch_fused_inverse<LOGN, LOGT, kInverseFromKeyMacFinish>(mode, slab, ctx, mod_base, mod_period, rows,
                                                                                  row_period, row_offset, source_spec, stream);
        }
        if constexpr (!ONLY_FINISH) {
            if (source == kInverseFromTensor)
                return launch_fused_inverse<LOGN, LOGT, kInverseFromTensor>(mode, slab, ctx, mod_base, mod_period, rows, row_period,
                                                                            row_offset, source_spec, stream);
            if (source == kInverseFromKeyMac)
                return launch_fused_inverse<LOGN, LOGT, kInverseFromKeyMac>(mode, slab, ctx, mod_base, mod_period, rows, row_period,
                                                                            row_offset, source_spec, stream);
        } else if (source != kInverseFromSlab) {
            return hipErrorInvalidValue;
        }
    }
    size_t paired_records = 0;
    if constexpr (GROUP > 1) {
        paired_records = rows <= kUngroupedBelowRows ? 0 : (rows / mod_period) / GROUP * GROUP;
        if (paired_records != 0) {
            hipError_t e = launch_inverse_kernel<LOGN, LOGT, kInverseFromSlab, GROUP>(
                mode, slab, ctx, map, paired_records / GROUP * mod_period, source_spec, stream);
            if (e != hipSuccess) return e;
        }
    }
    const size_t rest = rows - paired_records * mod_period;
    if (rest == 0) return hipSuccess;
    return launch_inverse_kernel<LOGN, LOGT, kInverseFromSlab, 1>(
        mode, slab, ctx, make_row_map(mod_base, mod_period, row_period, row_offset, static_cast<uint32_t>(paired_records)), rest,
        source_spec, stream);
}

}  // namespace

hipError_t launch_ntt_spread(const uint64_t* source, size_t poly_stride, uint32_t source_moduli, size_t polys,
                             uint64_t* spread, const DeviceContext& ks_ctx, uint32_t galois_inverse, hipStream_t stream) {
    const uint32_t period = source_moduli + 1;
    const size_t rows = polys * source_moduli * period;
    if (rows == 0) return hipSuccess;
    if (rows > (size_t(1) << 30) || ks_ctx.moduli_count < period) return hipErrorInvalidValue;
    const SpreadSource src{source, poly_stride, source_moduli, 0, galois_inverse};
    // One launch per run of key-switching moduli of one butterfly class (band_runs: e.g. 29 | 60, 60 for the reference's
    // n_8192_logq_29_60_60, whose 60-bit rows then take the fold butterflies); the usual contexts -- every modulus in
    // [2^40, 2^55) -- are one run, and a batch of one workgroup generation takes one launch either way.
    auto launch = [&](int mode, uint32_t base, uint32_t band) {
        const size_t band_total = polys * source_moduli * band;
        const uint32_t row_period = band == period ? 0 : period;
        switch (ks_ctx.log_degree) {
            case 12: return launch_forward_tiled<12, 9, kSourceSpread>(mode, spread, ks_ctx, base, band, band_total, src, stream, row_period, base);
            case 13: return launch_forward_tiled<13, 10, kSourceSpread>(mode, spread, ks_ctx, base, band, band_total, src, stream, row_period, base);
            case 14: return launch_forward_tiled<14, 10, kSourceSpread>(mode, spread, ks_ctx, base, band, band_total, src, stream, row_period, base);
            case 15:  // four interleaved sub-rows (the automorphism of a Galois key switch: the caller's unfused path)
                if (galois_inverse != 0 || kMaxFusedLoadLogDegree < 15 || !kFusedSpreadAt32768) return hipErrorNotSupported;
                return launch_interleaved_forward<2, kSourceSpread>(mode, spread, ks_ctx, make_row_map(base, band, row_period, base),
                                                                    band_total, src, stream);
            default: return hipErrorNotSupported;  // caller falls back to spread kernel + launch_ntt
        }
    };
    BandRun runs[kMaxBandRuns];
    const int count = (ks_ctx.log_degree == 12 || ks_ctx.log_degree == 13) && rows > kOneGeneration ? band_runs(ks_ctx, period, runs) : 0;
    if (count <= 1) return launch(production_mode(ks_ctx), 0, period);
    for (int k = 0; k < count; ++k)
        if (hipError_t e = launch(runs[k].mode, runs[k].base, runs[k].rows); e != hipSuccess) return e;
    return hipSuccess;
}

hipError_t launch_ntt_lift(const uint64_t* plaintexts, uint64_t plaintext_modulus, size_t polys, uint64_t* out,
                           const DeviceContext& ctx, hipStream_t stream) {
    const uint32_t period = ctx.moduli_count;
    const size_t rows = polys * period;
    if (rows == 0) return hipSuccess;
    if (rows > (size_t(1) << 30)) return hipErrorInvalidValue;
    const SpreadSource src{plaintexts, size_t(1) << ctx.log_degree, 1, plaintext_modulus, 0};
    const int mode = production_mode(ctx);
    switch (ctx.log_degree) {
        case 12: return launch_forward_tiled<12, 9, kSourceLift>(mode, out, ctx, 0, period, rows, src, stream);
        case 13: return launch_forward_tiled<13, 10, kSourceLift>(mode, out, ctx, 0, period, rows, src, stream);
        case 14: return launch_forward_tiled<14, 10, kSourceLift>(mode, out, ctx, 0, period, rows, src, stream);
        case 15:
            if (kMaxFusedLoadLogDegree < 15) return hipErrorNotSupported;
            return launch_interleaved_forward<2, kSourceLift>(mode, out, ctx, make_row_map(0, period, 0, 0), rows, src, stream);
        default: return hipErrorNotSupported;  // caller falls back to the lift kernel + launch_ntt
    }
}

const char* ntt_variant_name(uint32_t log_degree) {
    switch (log_degree) {
        case 12: return "ntt_tiled<4096, 512 lanes x 8 words>";
        case 13: return "ntt_tiled<8192, 1024 lanes x 8 words>";
        case 14: return "ntt_interleaved<16384 = 2 x 8192, 1024 lanes x 8 words x 2 sub-rows>";
        case 15: return "ntt_interleaved<32768 = 4 x 8192, 1024 lanes x 8 words x 4 sub-rows>";
        default: return "generic radix-2";
    }
}

hipError_t launch_ntt_band(bool inverse, uint64_t* slab, const DeviceContext& ctx, uint32_t mod_base, uint32_t band_rows,
                           uint32_t record_rows, uint32_t band_offset, size_t records, int mode, hipStream_t stream,
                           int source = kInverseFromSlab, const InverseSource& source_spec = {}) {
    const size_t rows = records * band_rows;
    if (rows == 0) return hipSuccess;
    if (rows > (size_t(1) << 30)) return hipErrorInvalidValue;
    switch (ctx.log_degree) {
        case 12: return launch_tiled<12, 9>(inverse, mode, slab, ctx, mod_base, band_rows, rows, stream, record_rows, band_offset, source, source_spec);
        case 13: return launch_tiled<13, 10>(inverse, mode, slab, ctx, mod_base, band_rows, rows, stream, record_rows, band_offset, source, source_spec);
        case 14: return launch_tiled<14, 10>(inverse, mode, slab, ctx, mod_base, band_rows, rows, stream, record_rows, band_offset, source, source_spec);
        case 15: {
            const RowMap map = make_row_map(mod_base, band_rows, record_rows, band_offset);
            if (kMaxFusedLoadLogDegree < 15 && inverse && source != kInverseFromSlab) return hipErrorNotSupported;
            if (inverse && source == kInverseFromTensor) return launch_interleaved_inverse<2, kInverseFromTensor>(mode, slab, ctx, map, rows, source_spec, stream);
            if constexpr (kFusedKeyMacAt32768) {  // (not instantiated otherwise)
                if (inverse && source == kInverseFromKeyMac) return launch_interleaved_inverse<2, kInverseFromKeyMac>(mode, slab, ctx, map, rows, source_spec, stream);
            }
            if (inverse && source != kInverseFromSlab) return hipErrorNotSupported;  // the key switch's fused end: not at this degree
            return launch_interleaved<2>(inverse, mode, slab, ctx, map, rows, stream);
        }
        default: return hipErrorNotSupported;
    }
}

// [Q, Bsk] records (BEHZ): the first `headroom_prefix` moduli (the ciphertext moduli, when they are the usual <= 55-bit
// primes) take the fold-free split butterflies, the 61-bit Bsk primes the [0, 8p) ones -- two launches over row bands of
// the same slab.  Falls back to one launch when the context has no such prefix or no tiled kernel.
hipError_t launch_ntt_mixed(bool inverse, uint64_t* slab, const DeviceContext& ctx, uint32_t record_rows, size_t records,
                            hipStream_t stream) {
    const bool tiled = ctx.log_degree >= 12 && ctx.log_degree <= kMaxFusedLoadLogDegree;
    BandRun runs[kMaxBandRuns];
    const int count = tiled ? band_runs(ctx, record_rows, runs) : 0;
    if (count <= 1 || records * record_rows > (size_t(1) << 30) || records * record_rows <= kOneGeneration)
        return launch_ntt(inverse, slab, ctx, 0, record_rows, records * record_rows, stream);
    for (int k = 0; k < count; ++k) {
        hipError_t e = launch_ntt_band(inverse, slab, ctx, runs[k].base, runs[k].rows, record_rows, runs[k].base, records,
                                       runs[k].mode, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The rows [first, first + count) of every record only (row r uses modulus r), one launch per run of moduli of one butterfly
// class inside that range: e.g. the Bsk rows of lifted records whose Q rows already hold their transform.
hipError_t launch_ntt_record_band(bool inverse, uint64_t* slab, const DeviceContext& ctx, uint32_t record_rows, uint32_t first,
                                  uint32_t count, size_t records, hipStream_t stream) {
    if (records == 0 || count == 0) return hipSuccess;
    const bool tiled = ctx.log_degree >= 12 && ctx.log_degree <= kMaxFusedLoadLogDegree;
    if (!tiled || first + count > record_rows || records * record_rows > (size_t(1) << 30)) return hipErrorNotSupported;
    BandRun runs[kMaxBandRuns];
    const int run_count = band_runs(ctx, record_rows, runs);
    if (run_count <= 1) return launch_ntt_band(inverse, slab, ctx, first, count, record_rows, first, records, production_mode(ctx), stream);
    for (int k = 0; k < run_count; ++k) {
        const uint32_t begin = runs[k].base > first ? runs[k].base : first;
        const uint32_t end = runs[k].base + runs[k].rows < first + count ? runs[k].base + runs[k].rows : first + count;
        if (begin >= end) continue;
        hipError_t e = launch_ntt_band(inverse, slab, ctx, begin, end - begin, record_rows, begin, records, runs[k].mode, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// Forward NTT of lifted [Q, Bsk] records whose Q rows are still where the ciphertexts lie (the lift was told not to copy
// them, rns_kernels launch_lift_q_to_qbsk_strided): the Q band is read from the source polynomials (kSourceRows) and
// written into the slab, the Bsk band is transformed in place.  hipErrorNotSupported when the context has no fold-free
// prefix of exactly source_moduli rows or no tiled kernel -- the caller then lifts with the copy and runs
// launch_ntt_mixed.
bool ntt_lifted_forward_supported(const DeviceContext& ctx, uint32_t record_rows, uint32_t source_moduli, size_t records) {
    const bool tiled = ctx.log_degree >= 12 && ctx.log_degree <= kMaxFusedLoadLogDegree;
    return tiled && source_moduli != 0 && source_moduli < record_rows && ctx.headroom_prefix == source_moduli &&
           ctx.approx_ok != 0 && ctx.forward_split_pairs != nullptr && records * record_rows > kOneGeneration &&
           records * record_rows <= (size_t(1) << 30);
}
hipError_t launch_ntt_lifted_forward(uint64_t* slab, const DeviceContext& ctx, uint32_t record_rows, size_t records,
                                     const uint64_t* base, const uint64_t* second, size_t stride, uint32_t source_moduli,
                                     hipStream_t stream) {
    if (records == 0) return hipSuccess;
    if (!ntt_lifted_forward_supported(ctx, record_rows, source_moduli, records)) return hipErrorNotSupported;
    const SpreadSource src{base, stride, source_moduli, 0, 0, second};
    const size_t rows = records * source_moduli;
    hipError_t e;
    switch (ctx.log_degree) {
        case 12: e = launch_forward_tiled<12, 9, kSourceRows>(kModeSplit, slab, ctx, 0, source_moduli, rows, src, stream, record_rows, 0); break;
        case 13: e = launch_forward_tiled<13, 10, kSourceRows>(kModeSplit, slab, ctx, 0, source_moduli, rows, src, stream, record_rows, 0); break;
        case 14: e = launch_forward_tiled<14, 10, kSourceRows>(kModeSplit, slab, ctx, 0, source_moduli, rows, src, stream, record_rows, 0); break;
        case 15: e = launch_interleaved_forward<2, kSourceRows>(kModeSplit, slab, ctx, make_row_map(0, source_moduli, record_rows, 0), rows, src, stream); break;
        default: return hipErrorNotSupported;  // (ntt_lifted_forward_supported says so first; a new degree must be named here)
    }
    if (e != hipSuccess) return e;
    return launch_ntt_band(false, slab, ctx, source_moduli, record_rows - source_moduli, record_rows, source_moduli, records,
                           kModeApprox, stream);
}

// Tensor product + inverse NTT of BEHZ multiplication in one kernel per row band: lifted [items][4][record_rows][N]
// (Eval) -> out [items][3][record_rows][N] (Coeff).  hipErrorNotSupported where no tiled kernel exists (the caller
// then runs launch_tensor + launch_ntt_mixed).
hipError_t launch_ntt_tensor_inverse(const uint64_t* lifted, uint64_t* out, const DeviceContext& ctx, uint32_t record_rows,
                                     size_t items, hipStream_t stream) {
    const bool tiled = ctx.log_degree >= 12 && ctx.log_degree <= kMaxFusedLoadLogDegree;
    const size_t records = items * 3;
    if (!tiled || records * record_rows > (size_t(1) << 30)) return hipErrorNotSupported;
    if (records == 0) return hipSuccess;
    const InverseSource spec{lifted};
    BandRun runs[kMaxBandRuns];
    // (a product of a few ciphertexts is one workgroup generation whichever butterflies it takes: one launch over all rows in
    // the mode every modulus of the context accepts, like launch_ntt_mixed -- 13.6 + 14.5 -> 15 us on one ciphertext pair,
    // profiles/r06x_small_chains.txt)
    const int count = records * record_rows <= kOneGeneration ? 0 : band_runs(ctx, record_rows, runs);
    if (count <= 1)
        return launch_ntt_band(true, out, ctx, 0, record_rows, record_rows, 0, records, production_mode(ctx), stream,
                               kInverseFromTensor, spec);
    for (int k = 0; k < count; ++k) {
        hipError_t e = launch_ntt_band(true, out, ctx, runs[k].base, runs[k].rows, record_rows, runs[k].base, records,
                                       runs[k].mode, stream, kInverseFromTensor, spec);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// Key-switching inner product + inverse NTT in one kernel (Bfv+Keys.swift:180-207): spread [polys][L][L+1][N] (Eval),
// key [top][2][top_rows][N] -> out [polys][2][L+1][N] (Coeff).  hipErrorNotSupported where no tiled kernel exists.
// The rows [first, first + count) of every (polynomial, c) record of the key-switching product, one launch per run of
// moduli of one butterfly class inside that range (band_runs over the whole key-switching context, clipped).
hipError_t launch_key_mac_runs(uint64_t* prod, const DeviceContext& ks, uint32_t first, uint32_t count, uint32_t L,
                               size_t records, int source, const InverseSource& spec, hipStream_t stream) {
    BandRun runs[kMaxBandRuns];
    const bool fold_shape = ks.log_degree == 12 || ks.log_degree == 13;
    const int run_count = fold_shape && records * count > kOneGeneration ? band_runs(ks, L + 1, runs) : 0;
    if (run_count <= 1)
        return launch_ntt_band(true, prod, ks, first, count, L + 1, first, records, production_mode(ks), stream, source, spec);
    for (int k = 0; k < run_count; ++k) {
        const uint32_t begin = runs[k].base > first ? runs[k].base : first;
        const uint32_t end = runs[k].base + runs[k].rows < first + count ? runs[k].base + runs[k].rows : first + count;
        if (begin >= end) continue;
        hipError_t e = launch_ntt_band(true, prod, ks, begin, end - begin, L + 1, begin, records, runs[k].mode, stream, source, spec);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_ntt_key_mac_inverse(const uint64_t* spread, const uint64_t* key, uint64_t* out, const DeviceContext& ks,
                                      uint32_t L, uint32_t top_rows, size_t polys, hipStream_t stream) {
    const bool tiled = ks.log_degree >= 12 && ks.log_degree <= (kFusedKeyMacAt32768 ? kMaxFusedLoadLogDegree : 14u) &&
                       (kFusedKeyMacAt16384 || ks.log_degree != 14);
    const size_t records = polys * 2;
    if (!tiled || L > 64 || records * (L + 1) > (size_t(1) << 30)) return hipErrorNotSupported;
    if (records == 0) return hipSuccess;
    return launch_key_mac_runs(out, ks, 0, L + 1, L, records, kInverseFromKeyMac,
                               InverseSource{spread, key, L, top_rows}, stream);
}

// The same with the key switch's last step applied as the rows r < L are stored (kInverseFromKeyMacFinish): first the q_ks
// row of every (polynomial, c) into `prod` (the only rows of it that are written), then the rows r < L, which read that
// row, drop the special modulus and add the update to the first `added_polys` polynomials of the ciphertext at
// ct_base + polynomial * ct_stride: out [polys][2][L][N].  hipErrorNotSupported (nothing launched) where the degree has
// no kernel that pairs the key columns; the caller then runs launch_ntt_key_mac_inverse + launch_key_switch_finish.
bool ntt_key_mac_finish_supported(const DeviceContext& ks, uint32_t L, size_t polys) {
    const bool tiled = ks.log_degree >= 12 && ks.log_degree <= 14;  // the degrees with a fused key-MAC transform
    // (a batch of up to two workgroup generations is latency-bound: there two transforms in a row cost more than one
    // transform and the small element-wise kernel -- single-query expansions lost 11-29 % with the fused end at every
    // level, and the Galois key switch crosses over between 96 and 128 ciphertexts at N = 8192, L = 4:
    // profiles/r04m_galois_fused_end_ab.txt)
    // (N = 16384: the key MAC runs as interleaved sub-rows, two workgroups per CU, and ends in the separate finish kernel --
    // kInterleavedKeyMacAt16384, measured against the 16-words-per-lane tile with the fused end)
    if (ks.log_degree == 14 && ((kInterleavedFusedLoads && kInterleavedKeyMacAt16384) || !kFusedKeyMacAt16384)) return false;
    return tiled && L >= 1 && L < 64 && ks.moduli_count == L + 1 && polys * 2 * (L + 1) > 2 * kOneGeneration &&
           polys * 2 * (L + 1) <= (size_t(1) << 30);
}
hipError_t launch_ntt_key_mac_inverse_finish(const uint64_t* spread, const uint64_t* key, uint64_t* prod,
                                             const KeySwitchEnd<uint64_t>& end, const DeviceContext& ks, uint32_t L,
                                             uint32_t top_rows, size_t polys, hipStream_t stream) {
    if (!ntt_key_mac_finish_supported(ks, L, polys)) return hipErrorNotSupported;
    if (polys == 0) return hipSuccess;
    const InverseSource spec{spread, key, L, top_rows, end.ct_base, end.ct_stride, end.out, end.added_polys,
                             end.galois_inverse, end.expand_shift, end.own_base != nullptr ? end.own_base : end.ct_base,
                             end.targets_table, end.targets_group_size == 0 ? 1 : end.targets_group_size,
                             end.targets_group_stride, end.poly_base};
    hipError_t e = launch_key_mac_runs(prod, ks, L, 1, L, polys * 2, kInverseFromKeyMac, spec, stream);
    if (e != hipSuccess) return e;
    return launch_key_mac_runs(prod, ks, 0, L, L, polys * 2, kInverseFromKeyMacFinish, spec, stream);
}

// Inverse NTT of `rows` rows read from `source` and written to the same places of `slab` (the tiled 8-words-per-lane kernels of
// N = 4096 / 8192 load their rows through source_spec.first when it is set); hipErrorNotSupported (nothing launched) elsewhere.
hipError_t launch_ntt_inverse_out_of_place(const uint64_t* source, uint64_t* slab, const DeviceContext& ctx, uint32_t mod_base,
                                           uint32_t mod_period, size_t rows, hipStream_t stream) {
    if (rows == 0) return hipSuccess;
    if (source == nullptr || ctx.scaled_inverse_degree != 0 || ctx.approx_ok == 0 || rows > (size_t(1) << 30)) return hipErrorNotSupported;
    const InverseSource spec{source};
    switch (ctx.log_degree) {
        case 12: return launch_tiled<12, 9>(true, production_mode(ctx), slab, ctx, mod_base, mod_period, rows, stream, 0, 0, kInverseFromSlab, spec);
        case 13: return launch_tiled<13, 10>(true, production_mode(ctx), slab, ctx, mod_base, mod_period, rows, stream, 0, 0, kInverseFromSlab, spec);
        default: return hipErrorNotSupported;
    }
}

hipError_t launch_ntt(bool inverse, uint64_t* slab, const DeviceContext& ctx, uint32_t mod_base, uint32_t mod_period,
                      size_t rows, hipStream_t stream, int force_variant) {
    if (rows == 0) return hipSuccess;
    // grid.x is limited to 2^31-1 workgroups; split very large batches
    constexpr size_t kMaxRowsPerLaunch = size_t(1) << 30;
    if (rows > kMaxRowsPerLaunch) {
        // keep the row -> modulus mapping intact: chunk must be a multiple of mod_period
        const size_t chunk = (kMaxRowsPerLaunch / mod_period) * mod_period;
        for (size_t done = 0; done < rows; done += chunk) {
            const size_t now = rows - done < chunk ? rows - done : chunk;
            hipError_t e = launch_ntt(inverse, slab + done * ctx.degree, ctx, mod_base, mod_period, now, stream,
                                      force_variant);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    switch (force_variant) {
        case kNttVariantAuto: case kNttVariantExact: case kNttVariantGeneric: case kNttVariantWide:
        case kNttVariantApprox: break;
        default: return hipErrorInvalidValue;
    }
    // kNttVariantExact / kNttVariantApprox pin the butterfly schedule (tests); every variant computes the same transform
    const int mode = (ctx.approx_ok == 0 || force_variant == kNttVariantExact || force_variant == kNttVariantGeneric)
                         ? kModeExact
                         : (force_variant == kNttVariantApprox ? kModeApprox : production_mode(ctx));
    // production choice (auto): 8 words per lane wherever a workgroup of <= 1024 lanes allows it.  Two rows fit the
    // CU's LDS at a time, so the waves per CU -- what hides the global/LDS latencies -- are set by the lanes per row:
    // 32 waves per CU with 8 words per lane against 16 with 16 words.
    if (force_variant == kNttVariantAuto || force_variant == kNttVariantExact || force_variant == kNttVariantApprox) {
        switch (ctx.log_degree) {
            case 12: return launch_tiled<12, 9>(inverse, mode, slab, ctx, mod_base, mod_period, rows, stream);
            case 13: return launch_tiled<13, 10>(inverse, mode, slab, ctx, mod_base, mod_period, rows, stream);
            case 14: return launch_tiled<14, 10>(inverse, mode, slab, ctx, mod_base, mod_period, rows, stream);
            case 15: return launch_interleaved<2>(inverse, mode, slab, ctx, make_row_map(mod_base, mod_period, 0, 0), rows, stream);
            default: break;
        }
    }
    if (force_variant == kNttVariantWide) {  // 16 words per lane
        switch (ctx.log_degree) {
            case 12: return launch_tiled<12, 8>(inverse, mode, slab, ctx, mod_base, mod_period, rows, stream);
            case 13: return launch_tiled<13, 9>(inverse, mode, slab, ctx, mod_base, mod_period, rows, stream);
            case 14: return launch_tiled<14, 10>(inverse, mode, slab, ctx, mod_base, mod_period, rows, stream);
            default: break;
        }
    }
    return launch_generic(inverse, slab, ctx, mod_base, mod_period, rows, stream);
}

}  // namespace heamd
