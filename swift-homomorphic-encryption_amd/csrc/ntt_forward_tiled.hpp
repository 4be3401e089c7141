// ntt_forward_tiled.hpp -- the register-tiled forward transform (one row per workgroup, or a row group) with its fused row
// sources (ntt_sources.hpp), and the selector that names it.
// Included and instantiated only by the units that compile the kernels of one row size and direction together
// (ntt_tiled_4096.hip, ntt_forward_8192.hip, ntt_inverse_8192.hip: DESIGN.md section 4.1.1).  Design notes: ntt_routing.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_context.hpp"
#include "device_math.hpp"
#include "ntt_common.hpp"
#include "ntt_policy.hpp"
#include "ntt_rows.hpp"
#include "ntt_selectors.hpp"
#include "ntt_sources.hpp"
#include "placement.hpp"

namespace heamd {

namespace {

using namespace ntt;

template <int LOGN, int LOGT, int MODE, int SPREAD = kSourceSlab, int ROWS = 1>
__global__ void __launch_bounds__(1 << LOGT, min_waves_per_simd(LOGN - LOGT, ROWS))
    ntt_forward_tiled(uint64_t* __restrict__ slab, const DeviceContext ctx, const RowMap map, const SpreadSource spread) {
    constexpr int LOGE = LOGN - LOGT;
    constexpr int E = 1 << LOGE;
    using S = Schedule<LOGN, LOGE>;
    static_assert(S::P >= 1 && S::P <= 5, "unsupported pass count");
    static_assert(ROWS == 1 || S::P >= 2, "row groups go through the LDS tile");
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
    const uint32_t tid = threadIdx.x;
    uint32_t record, within;
    size_t rows[ROWS];
    if constexpr (SPREAD != kSourceSlab && SPREAD != kSourceRows) {
        // the band_rows output rows of a record are transforms of one source row: one replica set per group of ROWS
        // consecutive records (a workgroup transforms the same band row of each of them)
        // (a launch may cover a band of the records' rows -- the moduli of one butterfly class, launch_ntt_spread)
        uint32_t group;
        locate_replica(blockIdx.x, gridDim.x / map.band_rows, map.band_rows, group, within);
        record = map.record_base + group * ROWS;
        const size_t record_rows = map.record_rows == 0 ? map.band_rows : map.record_rows;
#pragma unroll
        for (int k = 0; k < ROWS; ++k) rows[k] = size_t(record + k) * record_rows + map.band_offset + within;
    } else {
        locate_rows<ROWS>(map, blockIdx.x, rows, record, within);
    }
    const uint32_t mi = map.mod_base + within;
    const DeviceModulus mod = ctx.moduli[mi];
    const Twiddles<MODE> tw(ctx, false, mi, LOGN, 0, kLaneMajorTwiddles<LOGN, LOGT, MODE, false, true>);
    const uint64_t p = mod.p;
    uint64_t v[ROWS][E];

    if constexpr (S::P == 1) {
        const BufferResource x = make_resource(slab + (rows[0] << LOGN), 8u << LOGN);
        global_load<LOGN, LOGE, 0, LOGN>(v[0], tid, x);
        forward_pass<LOGN, LOGE, 0, LOGN, MODE, true, 1>(v, tid, tw, p, true,
                                                        forward_first_twiddle<LOGN, LOGE, 0, LOGN, MODE, true>(tw, tid));
        canonicalize_all<MODE>(v, p);
        global_store<LOGN, LOGE, 0, LOGN>(v[0], tid, x);
    } else {
        constexpr int LO0 = LOGN - LOGE;
        if constexpr (SPREAD == kSourceRows) {
#pragma unroll
            for (int k = 0; k < ROWS; ++k) {
                const size_t rec = record + k;
                const uint64_t* source;
                if (spread.second == nullptr) {
                    source = spread.base + rec * spread.stride + (static_cast<size_t>(within) << LOGN);
                } else {
                    const size_t item = rec >> 2, slot = rec & 3;
                    source = ((slot & 2) != 0 ? spread.second : spread.base) + item * spread.stride +
                             (((slot & 1) * spread.L + within) << LOGN);
                }
                global_load<LOGN, LOGE, LO0, LOGE>(v[k], tid, make_resource(source, 8u << LOGN));
            }
        } else if constexpr (SPREAD != kSourceSlab) {
            bool reduce[ROWS];  // uniform: the source row is canonical mod a larger modulus than this row's
#pragma unroll
            for (int k = 0; k < ROWS; ++k) {
                const size_t poly = (record + k) / spread.L, j = (record + k) - poly * spread.L;  // record = poly * L + j
                global_load<LOGN, LOGE, LO0, LOGE, 0>(  // cached: the other rows of this record read the same words
                    v[k], tid, make_resource(spread.base + poly * spread.stride + (j << LOGN), 8u << LOGN));
                // the split butterflies take any 64-bit multiplicand and have room for an addend below 2p, so they
                // transform a residue below 2p as it is
                reduce[k] = SPREAD == kSourceSpread && ctx.moduli[j].p > p && !(is_split(MODE) && ctx.moduli[j].p < 2 * p);
                if constexpr (SPREAD == kSourceSpread) {
                    if (spread.galois_inverse != 0) {
                        // output coefficient e takes source coefficient i = e g^-1 mod 2N, negated mod q_j when i >= N.
                        // The row sits in the tile in order; consecutive lanes read words an odd stride apart, which
                        // spreads over all banks.
                        const uint64_t source_modulus = ctx.moduli[j].p;
                        if (k > 0) __syncthreads();
#pragma unroll
                        for (int r = 0; r < E; ++r) lds[element_index<LOGN, LOGE, LO0, LOGE>(r, tid)] = v[k][r];
                        __syncthreads();
#pragma unroll
                        for (int r = 0; r < E; ++r) {
                            const uint32_t doubled = (element_index<LOGN, LOGE, LO0, LOGE>(r, tid) * spread.galois_inverse) &
                                                     ((2u << LOGN) - 1u);
                            const uint64_t x = lds[doubled & ((1u << LOGN) - 1u)];
                            v[k][r] = (doubled >> LOGN) != 0 && x != 0 ? source_modulus - x : x;
                        }
                        if (k + 1 == ROWS) __syncthreads();  // the transform's exchanges reuse the tile
                    }
                }
            }
            if constexpr (SPREAD == kSourceLift) {
                const uint64_t threshold = (spread.plaintext_modulus + 1) >> 1, increment = p - spread.plaintext_modulus;
#pragma unroll
                for (int k = 0; k < ROWS; ++k)
#pragma unroll
                    for (int r = 0; r < E; ++r) v[k][r] = v[k][r] < threshold ? v[k][r] : v[k][r] + increment;
            } else {
                bool any = false;
#pragma unroll
                for (int k = 0; k < ROWS; ++k) any |= reduce[k];
                if (any) {  // rare (moduli of very different sizes): kept out of the straight-line path
#pragma unroll
                    for (int k = 0; k < ROWS; ++k)
#pragma unroll
                        for (int r = 0; r < E; ++r)
                            v[k][r] = reduce[k] ? barrett_reduce64_uniform(v[k][r], p, mod.barrett64) : v[k][r];
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < ROWS; ++k)
                global_load<LOGN, LOGE, LO0, LOGE>(v[k], tid, make_resource(slab + (rows[k] << LOGN), 8u << LOGN));
        }
        using O = PassOrder<LOGN, LOGE, kTopPartialOrder<LOGN, LOGE, false, SPREAD == kSourceSlab>>;
        // (N = 4096, two rows per workgroup on the shift-folded products: one register short with a carried lane index)
        constexpr bool LATE = LOGN == 12 && ROWS == 2 && MODE == kModeFoldLazy;
        forward_row<LOGN, LOGE, MODE, ROWS, true, O::kTop, LATE>(v, tid, tw, p, lds);
        constexpr int LO_BEFORE_LOW = O::kTop ? O::lo(S::P - 2) : LOGN - (S::P - 1) * LOGE;
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            const BufferResource out = make_resource(slab + (rows[k] << LOGN), 8u << LOGN);
            if constexpr (kStagedStore<LOGN, LOGE, LO_BEFORE_LOW, O::LOW>) {
                global_store_staged<LOGN, LOGE, O::LOW>(v[k], tid, out, lds);
            } else {
                global_store<LOGN, LOGE, 0, O::LOW>(v[k], tid, out);
            }
        }
    }
}

}  // namespace

template <int LOGN, int LOGT, int SPREAD, int ROWS>
hipError_t launch_forward_kernel(int mode, uint64_t* slab, const DeviceContext& ctx, const RowMap& map, size_t workgroups,
                                 const SpreadSource& spread, hipStream_t stream) {
    constexpr int LOGE = LOGN - LOGT;
    constexpr size_t lds_bytes = (Schedule<LOGN, LOGE>::P > 1) ? lds_words(1u << LOGN) * sizeof(uint64_t) : 0;
    auto kernel = mode == kModeSplit    ? ntt_forward_tiled<LOGN, LOGT, kModeSplit, SPREAD, ROWS>
                  : mode == kModeApprox ? ntt_forward_tiled<LOGN, LOGT, kModeApprox, SPREAD, ROWS>
                                        : ntt_forward_tiled<LOGN, LOGT, kModeExact, SPREAD, ROWS>;
    if constexpr (kFoldLazyForward<LOGN, LOGT>) {
        // every modulus of the launch is just below a power of two: products folded by a shift, no quotient, no factors
        if (mode == kModeSplit && fold_lazy_band(ctx, map)) {
            kernel = ntt_forward_tiled<LOGN, LOGT, kModeFoldLazy, SPREAD, ROWS>;
            if constexpr (kFoldLazyForwardMode<LOGN, LOGT, SPREAD> == kModeFoldSigned) {
                // the signed form reads its own tables (PolyContext::upload builds them at N = 8192); an image without them
                // keeps the unsigned kernel
                if (ctx.forward_split_pairs_signed_lanes != nullptr) kernel = ntt_forward_tiled<LOGN, LOGT, kModeFoldSigned, SPREAD, ROWS>;
            }
        }
    }
    if constexpr (kFoldShape<LOGN, LOGT> && (SPREAD == kSourceSlab || SPREAD == kSourceSpread)) {
        if (mode == kModeApprox && ctx.forward_split_pairs != nullptr) {
            const int fold = fold_mode(ctx, map.mod_base, map.band_rows);
            if (fold == kModeFoldMinus) kernel = ntt_forward_tiled<LOGN, LOGT, kModeFoldMinus, SPREAD, ROWS>;
            if (fold == kModeFoldPlus) kernel = ntt_forward_tiled<LOGN, LOGT, kModeFoldPlus, SPREAD, ROWS>;
        }
    }
    if (hipError_t e = allow_dynamic_lds(kernel, lds_bytes); e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(workgroups)), dim3(1u << LOGT), lds_bytes, stream, slab, ctx, map,
                       spread);
    return hipGetLastError();
}

#define HEAMD_FORWARD_TILED(LOGN, LOGT, SPREAD, ROWS)                                                                        \
    template hipError_t launch_forward_kernel<LOGN, LOGT, SPREAD, ROWS>(int, uint64_t*, const DeviceContext&, const RowMap&, \
                                                                        size_t, const SpreadSource&, hipStream_t)

}  // namespace heamd
