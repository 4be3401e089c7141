// ntt_interleaved.hpp -- N = 16384 / 32768 as 2 / 4 interleaved sub-rows of 8192 words: the forward and inverse kernels, which
// share the row moves below, and the two selectors that name them.
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

// ---- interleaved rows: N = 2^(13 + LOGS) as 2^LOGS sub-rows of 8192 words --------------------------------------------
// A row of 16384 (32768) words fills the CU's LDS as one tile.  Taken as its 2 (4) sub-rows "element index mod 2^LOGS"
// it is the row group of the N = 8192 kernel: sub-row h holds the words idx = i 2^LOGS + h, and every stage on an element
// bit b >= LOGS pairs words of ONE sub-row (i and i + 2^(b - LOGS)) under a twiddle that only depends on idx >> (b + 1)
// = i >> (b - LOGS + 1) -- the same for all sub-rows, and the very index the 8192-point transform of sub-row words uses
// in its own stage: W[2^s + group] of the degree's table, s < 13, is read exactly as the smaller transform would read
// its own table.  So the first 13 forward stages are forward_row<13> over the sub-rows (one 76 KB tile in turn, every
// twiddle fetched once for all sub-rows, two workgroups per CU at N = 16384), and the remaining LOGS stages pair words
// of different sub-rows held in the same register of the same lane (cross stages, gathered twiddles).  The inverse
// mirrors it: cross stages first, then inverse_row<13> against the tail of the inverse table (which lists its stages
// from the low bit up, ntt_common.hpp inverse_twiddle: block m at N - 2m + 1, so the sub-transform's index plus
// N - 8192).  In the top-pass layout a lane's words i = r 1024 + tid of all sub-rows are 16 (32) contiguous bytes of
// the row: the forward load and the inverse store move whole lines with 16-byte accesses.
constexpr int kSubLogN = 13, kSubLogT = 10, kSubLogE = kSubLogN - kSubLogT;
// The sub-rows' 8192-point transforms read lane-major stage blocks like the N = 8192 kernels (ntt_rows.hpp kLaneMajorTwiddles,
// built by PolyContext::upload inside the degree's own tables): with the plain tables a wave's gather of one twiddle touches
// every 2^g-th entry of a run, up to 64 cache lines for 1 KiB -- made-up twiddles showed the gathers cost the inverse 19 % and
// the forward transform 8 % at N = 16384 (profiles/r06j_n16384_what_binds.txt).
template <int MODE>
constexpr int kInterleavedLaneMajor = (is_split(MODE) || is_fold(MODE)) ? 1 : 0;

// forward cross stage c (global stage 13 + c) pairs sub-row bit LOGS - 1 - c; twiddle 2^(13+c) + (idx >> (LOGS - c))
// Twiddles in flight: a cross stage's twiddles serve ONE butterfly per pair of sub-rows each (N = 16384: 8 gathers per lane, one
// butterfly between two of them), so with one request ahead every gather's L2 round trip is waited out in full -- the shift-folded
// products (4 registers per twiddle) keep kTwiddlesAhead of them in flight, the limb-wise ones (6) one.
// (measured at N = 16384, profiles/r06n_n16384_cross_stage_prefetch_ab.txt: two or three limb-wise twiddles in flight spill
// -- 16 / 40 B -- and lose 1 / 8 %; the first one requested before the row's loads: +-0)
constexpr int kCrossAheadSplit = 1;
constexpr bool kCrossEarlySplit = false;
template <int MODE>
constexpr int kCrossAhead = MODE == kModeFoldLazy ? 3 : (is_split(MODE) ? kCrossAheadSplit : 1);
// the inverse carries the finished sub-rows through its cross stages, so its third twiddle in flight costs it 20 B of scratch:
// two measure 4-5 % faster at N = 16384 and keep none (profiles/r06v_interleaved_fold_inverse_ab.txt)
template <int MODE>
constexpr int kCrossAheadInverse = MODE == kModeFoldLazy ? 2 : kCrossAhead<MODE>;
template <int LOGS, int MODE>
__device__ __forceinline__ void forward_cross_stages(uint64_t (&v)[1 << LOGS][1 << kSubLogE], uint32_t tid,
                                                     const Twiddles<MODE>& tw, uint64_t p) {
    constexpr int E = 1 << kSubLogE, R = Schedule<kSubLogN, kSubLogE>::R, AHEAD = kCrossAhead<MODE>;
    static_assert(!is_split(MODE) || 1 + ((kSubLogN + LOGS) << Lazy<MODE>::kProductLog) <= 511, "growth stays below 2^9 p");
    const uint64_t neg_p = Lazy<MODE>::reduction_constant(p);
    const uint64_t half_bound = p << Lazy<MODE>::kProductLog;
    const FoldConstants fc = mode_fold_constants<MODE>(p);
    const uint32_t lane_words = lane_part<kSubLogN, kSubLogE, 0, R>(tid);
#pragma unroll
    for (int c = 0; c < LOGS; ++c) {
        const int count = E << c;  // twiddles of the stage per lane: one per (word, upper sub-row bits)
        auto request = [&](int k) {
            const int r = k >> c, upper = k & ((1 << c) - 1);
            const uint32_t fixed = (1u << (kSubLogN + c)) + (register_part<kSubLogN, kSubLogE, 0, R>(r) << c) + upper;
            return fetch_twiddle<MODE, false>(tw, lane_words << c, fixed);
        };
        TwiddleWords ring[AHEAD];
#pragma unroll
        for (int a = 0; a < AHEAD; ++a) ring[a] = request(a < count ? a : count - 1);
#pragma unroll
        for (int k = 0; k < count; ++k) {
            const TwiddleWords w = ring[k % AHEAD];
            if (k + AHEAD < count) {
                ring[k % AHEAD] = request(k + AHEAD);
                __builtin_amdgcn_sched_barrier(0);
            }
            const int r = k >> c, upper = k & ((1 << c) - 1);
            const int span = 1 << (LOGS - 1 - c);  // sub-row distance of a pair
#pragma unroll
            for (int low = 0; low < span; ++low) {
                const int h = (upper << (LOGS - c)) | low;
                forward_butterfly<MODE>(v[h][r], v[h + span][r], w, false, neg_p, half_bound, true, fc);
            }
            if (k + AHEAD < count) __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// inverse cross stage c pairs sub-row bit c (element bit c): m = N >> (c + 1) groups, twiddle (N - 2m + 1) + (idx >> (c + 1))
// PRIOR: the words enter in the lazy range of a row whose first PRIOR stages already ran (the fused loads' [0, 5p) words)
// `head`: the first kTwiddlesAhead twiddles of stage 0, requested by the caller BEFORE it loads the row (inverse_cross_head): the
// transform opens with this stage, and its gathers then travel beside the row's loads instead of starting behind them.
template <int LOGS, int MODE>
__device__ __forceinline__ TwiddleWords inverse_cross_twiddle(const Twiddles<MODE>& tw, uint32_t lane_words, int c, int k) {
    constexpr int R = Schedule<kSubLogN, kSubLogE>::R;
    constexpr uint32_t N = 1u << (kSubLogN + LOGS);
    const uint32_t m = N >> (c + 1);
    const int upper_bits = LOGS - 1 - c;  // sub-row bits above the paired one
    const int r = k >> upper_bits, upper = k & ((1 << upper_bits) - 1);
    const uint32_t fixed = (N - 2 * m + 1) + (register_part<kSubLogN, kSubLogE, 0, R>(r) << upper_bits) + upper;
    return fetch_twiddle<MODE, false>(tw, lane_words << upper_bits, fixed);
}
template <int LOGS, int MODE>
__device__ __forceinline__ void inverse_cross_head(TwiddleWords (&head)[kCrossAheadInverse<MODE>], uint32_t tid, const Twiddles<MODE>& tw) {
    constexpr int R = Schedule<kSubLogN, kSubLogE>::R;
    const uint32_t lane_words = lane_part<kSubLogN, kSubLogE, 0, R>(tid);
#pragma unroll
    for (int a = 0; a < kCrossAheadInverse<MODE>; ++a) head[a] = inverse_cross_twiddle<LOGS, MODE>(tw, lane_words, 0, a);
}
template <int LOGS, int MODE, int PRIOR = 0>
__device__ __forceinline__ void inverse_cross_stages(uint64_t (&v)[1 << LOGS][1 << kSubLogE], uint32_t tid,
                                                     const Twiddles<MODE>& tw, uint64_t p,
                                                     const TwiddleWords (&head)[kCrossAheadInverse<MODE>]) {
    constexpr int E = 1 << kSubLogE, R = Schedule<kSubLogN, kSubLogE>::R, H = Lazy<MODE>::kInverseCapLog, AHEAD = kCrossAheadInverse<MODE>;
    static_assert(AHEAD <= E, "the head twiddles are all of stage 0");
    const uint64_t neg_p = Lazy<MODE>::reduction_constant(p);
    const FoldConstants fc = mode_fold_constants<MODE>(p);
    const uint32_t lane_words = lane_part<kSubLogN, kSubLogE, 0, R>(tid);
#pragma unroll
    for (int c = 0; c < LOGS; ++c) {
        const int in_shift = inverse_in_shift<MODE>(c + PRIOR);
        const uint64_t bound = p << in_shift;
        const bool fold = in_shift + 1 > H;
        const int upper_bits = LOGS - 1 - c;  // sub-row bits above the paired one
        const int count = E << upper_bits;
        TwiddleWords ring[AHEAD];
#pragma unroll
        for (int a = 0; a < AHEAD; ++a)
            ring[a] = c == 0 ? head[a] : inverse_cross_twiddle<LOGS, MODE>(tw, lane_words, c, a < count ? a : count - 1);
#pragma unroll
        for (int k = 0; k < count; ++k) {
            const TwiddleWords w = ring[k % AHEAD];
            if (k + AHEAD < count) {
                ring[k % AHEAD] = inverse_cross_twiddle<LOGS, MODE>(tw, lane_words, c, k + AHEAD);
                __builtin_amdgcn_sched_barrier(0);
            }
            const int upper = k & ((1 << upper_bits) - 1), r = k >> upper_bits;
            const int span = 1 << c;
#pragma unroll
            for (int low = 0; low < span; ++low) {
                const int h = (upper << (c + 1)) | low;
                inverse_butterfly<MODE>(v[h][r], v[h + span][r], w, false, p, neg_p, bound, fold, fc, split_signed_bias(p));
            }
            if (k + AHEAD < count) __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// Words i = r 1024 + tid (top-pass layout of the sub-rows) of all sub-rows: 8 2^LOGS contiguous bytes of the row per lane.
template <int LOGS, bool STORE, int POLICY = row_policy<kSubLogN + LOGS>()>
__device__ __forceinline__ void interleaved_top_words(uint64_t (&v)[1 << LOGS][1 << kSubLogE], uint32_t tid, BufferResource row) {
    constexpr int ROWS = 1 << LOGS;
    const uint32_t lane_bytes = tid << (3 + LOGS);
#pragma unroll
    for (int r = 0; r < (1 << kSubLogE); ++r) {
#pragma unroll
        for (int h = 0; h < ROWS; h += 2) {
            const uint32_t fixed = (static_cast<uint32_t>(r) << (kSubLogT + 3 + LOGS)) + h * 8;
            if constexpr (STORE) {
                const Dwordx4 words = {lo32(v[h][r]), hi32(v[h][r]), lo32(v[h + 1][r]), hi32(v[h + 1][r])};
                __builtin_amdgcn_raw_buffer_store_b128(words, row, lane_bytes, fixed, POLICY);
            } else {
                const Dwordx4 words = __builtin_amdgcn_raw_buffer_load_b128(row, lane_bytes, fixed, POLICY);
                v[h][r] = pack64(words.x, words.y);
                v[h + 1][r] = pack64(words.z, words.w);
            }
        }
    }
}
// Words of the low-pass layout of the sub-rows (element_index<13, 3, 0, 1>: runs of 2 words of a sub-row per lane, i.e.
// runs of 2^(LOGS + 1) words of the row) of all sub-rows: 16-byte accesses as the words lie.
template <int LOGS, bool STORE>
__device__ __forceinline__ void interleaved_low_words(uint64_t (&v)[1 << LOGS][1 << kSubLogE], uint32_t tid, BufferResource row) {
    constexpr int ROWS = 1 << LOGS, R = Schedule<kSubLogN, kSubLogE>::R, POLICY = row_policy<kSubLogN + LOGS>();
    const uint32_t lane_bytes = lane_part<kSubLogN, kSubLogE, 0, R>(tid) << (3 + LOGS);
#pragma unroll
    for (int r = 0; r < (1 << kSubLogE); ++r) {
#pragma unroll
        for (int h = 0; h < ROWS; h += 2) {
            const uint32_t fixed = (register_part<kSubLogN, kSubLogE, 0, R>(r) << (3 + LOGS)) + h * 8;
            if constexpr (STORE) {
                const Dwordx4 words = {lo32(v[h][r]), hi32(v[h][r]), lo32(v[h + 1][r]), hi32(v[h + 1][r])};
                __builtin_amdgcn_raw_buffer_store_b128(words, row, lane_bytes, fixed, POLICY);
            } else {
                const Dwordx4 words = __builtin_amdgcn_raw_buffer_load_b128(row, lane_bytes, fixed, POLICY);
                v[h][r] = pack64(words.x, words.y);
                v[h + 1][r] = pack64(words.z, words.w);
            }
        }
    }
}

// The same words in whole cache lines (ntt_common.hpp global_store_staged / global_load_staged): a lane's run is 2^(LOGS+1)
// contiguous words of the row, i.e. C = 2^LOGS 16-byte chunks; the wave's block of 64 C chunks per run goes through the
// wave's own 592-slot slice of the tile (free on both occasions: the exchange next to the low pass never leaves the
// wave) and crosses the memory interface in lane order, 1 KiB per instruction.
constexpr bool kInterleavedStaged = true;
template <int LOGS, bool STORE>
__device__ __forceinline__ void interleaved_low_words_staged(uint64_t (&v)[1 << LOGS][1 << kSubLogE], uint32_t tid,
                                                             BufferResource row, uint64_t* lds) {
    constexpr int ROWS = 1 << LOGS, C = ROWS, R = Schedule<kSubLogN, kSubLogE>::R, POLICY = row_policy<kSubLogN + LOGS>();
    static_assert(R == 1 && C * 64 * 16 <= 592 * 8, "runs of two sub-row words; the block fits the wave's slice");
    const uint32_t lane = tid & 63u;
    const uint32_t swizzle = (lane >> (4 - LOGS)) & (C - 1);
    char* const block = reinterpret_cast<char*>(lds + (tid >> 6) * 592u);
#pragma unroll
    for (int run = 0; run < (1 << (kSubLogE - R)); ++run) {
        const uint32_t first = (lane_part<kSubLogN, kSubLogE, 0, R>(tid & ~63u) | register_part<kSubLogN, kSubLogE, 0, R>(run << R))
                               << LOGS;  // row word the wave's block starts at
        if constexpr (STORE) {
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const int b = j / (ROWS / 2), h = (j % (ROWS / 2)) * 2;
                *reinterpret_cast<U64x2*>(block + ((lane * C + (j ^ swizzle)) << 4)) = U64x2{v[h][(run << R) + b], v[h + 1][(run << R) + b]};
            }
        }
        U64x2 picked[C];
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const uint32_t chunk = j * 64 + lane, owner = chunk / C, slot = chunk % C;
            const uint32_t owner_swizzle = (owner >> (4 - LOGS)) & (C - 1);
            char* const at = block + ((owner * C + (slot ^ owner_swizzle)) << 4);
            if constexpr (STORE) {
                const U64x2 pair = *reinterpret_cast<const U64x2*>(at);
                const Dwordx4 words = {lo32(pair.x), hi32(pair.x), lo32(pair.y), hi32(pair.y)};
                __builtin_amdgcn_raw_buffer_store_b128(words, row, (first << 3) + (lane << 4), j << 10, POLICY);
            } else {
                const Dwordx4 words = __builtin_amdgcn_raw_buffer_load_b128(row, (first << 3) + (lane << 4), j << 10, POLICY);
                picked[j] = U64x2{pack64(words.x, words.y), pack64(words.z, words.w)};
            }
        }
        if constexpr (!STORE) {
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const uint32_t chunk = j * 64 + lane, owner = chunk / C, slot = chunk % C;
                const uint32_t owner_swizzle = (owner >> (4 - LOGS)) & (C - 1);
                *reinterpret_cast<U64x2*>(block + ((owner * C + (slot ^ owner_swizzle)) << 4)) = picked[j];
            }
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const int b = j / (ROWS / 2), h = (j % (ROWS / 2)) * 2;
                const U64x2 pair = *reinterpret_cast<const U64x2*>(block + ((lane * C + (j ^ swizzle)) << 4));
                v[h][(run << R) + b] = pair.x;
                v[h + 1][(run << R) + b] = pair.y;
            }
        }
    }
}

// SPREAD: the row sources of ntt_forward_tiled (kSourceSpread without the automorphism, kSourceLift, kSourceRows) -- the step
// that would otherwise write the slab is applied to the words as they are loaded, in the top-pass layout of the sub-rows
// (a lane's words of all sub-rows are contiguous bytes of the SOURCE row too).
template <int LOGS, int MODE, int SPREAD = kSourceSlab>
__global__ void __launch_bounds__(1 << kSubLogT, min_waves_per_simd(kSubLogE, 1 << LOGS))
    ntt_forward_interleaved(uint64_t* __restrict__ slab, const DeviceContext ctx, const RowMap map, const SpreadSource spread) {
    constexpr int ROWS = 1 << LOGS, LOGD = kSubLogN + LOGS, E = 1 << kSubLogE;
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
    const uint32_t tid = threadIdx.x;
    uint32_t record, within;
    size_t rows[1];
    if constexpr (SPREAD == kSourceSpread || SPREAD == kSourceLift) {
        // the band_rows output rows of a record are transforms of one source row: one replica set per record
        uint32_t group;
        locate_replica(blockIdx.x, gridDim.x / map.band_rows, map.band_rows, group, within);
        record = map.record_base + group;
        rows[0] = size_t(record) * (map.record_rows == 0 ? map.band_rows : map.record_rows) + map.band_offset + within;
    } else {
        locate_rows<1>(map, blockIdx.x, rows, record, within);
    }
    const uint32_t mi = map.mod_base + within;
    const DeviceModulus mod = ctx.moduli[mi];
    const uint64_t p = mod.p;
    const Twiddles<MODE> tw(ctx, false, mi, LOGD, 0, kInterleavedLaneMajor<MODE>);  // (the cross stages' block is not permuted)
    const BufferResource row = make_resource(slab + (rows[0] << LOGD), 8u << LOGD);
    uint64_t v[ROWS][E];
    if constexpr (SPREAD == kSourceRows) {
        const uint64_t* source;
        if (spread.second == nullptr) {
            source = spread.base + size_t(record) * spread.stride + (static_cast<size_t>(within) << LOGD);
        } else {
            const size_t item = record >> 2, slot = record & 3;
            source = ((slot & 2) != 0 ? spread.second : spread.base) + item * spread.stride + (((slot & 1) * spread.L + within) << LOGD);
        }
        interleaved_top_words<LOGS, false>(v, tid, make_uniform_resource(source, 8u << LOGD));
    } else if constexpr (SPREAD != kSourceSlab) {
        const size_t poly = record / spread.L, j = record - poly * spread.L;  // record = poly * L + j
        // cached: the other rows of this record read the same words
        interleaved_top_words<LOGS, false, 0>(v, tid, make_uniform_resource(spread.base + poly * spread.stride + (j << LOGD), 8u << LOGD));
        if constexpr (SPREAD == kSourceLift) {
            const uint64_t threshold = (spread.plaintext_modulus + 1) >> 1, increment = p - spread.plaintext_modulus;
#pragma unroll
            for (int h = 0; h < ROWS; ++h)
#pragma unroll
                for (int r = 0; r < E; ++r) v[h][r] = v[h][r] < threshold ? v[h][r] : v[h][r] + increment;
        } else {
            // rare (moduli of very different sizes; ntt_forward_tiled): the source row is canonical mod a larger modulus
            const bool reduce = ctx.moduli[j].p > p && !(is_split(MODE) && ctx.moduli[j].p < 2 * p);  // wave-uniform
            if (reduce) {
#pragma unroll
                for (int h = 0; h < ROWS; ++h)
#pragma unroll
                    for (int r = 0; r < E; ++r) v[h][r] = reduce ? barrett_reduce64_uniform(v[h][r], p, mod.barrett64) : v[h][r];
            }
        }
    } else {
        interleaved_top_words<LOGS, false>(v, tid, row);
    }
    forward_row<kSubLogN, kSubLogE, MODE, ROWS, false>(v, tid, tw, p, lds);
    forward_cross_stages<LOGS, MODE>(v, tid, tw, p);
    canonicalize_all<MODE>(v, p);
    // (the store's lane addresses are derived from an opaque copy of the lane index: the compiler otherwise computes them
    // at the top of the kernel and carries them through every pass in scratch)
    if constexpr (kInterleavedStaged) interleaved_low_words_staged<LOGS, true>(v, opaque32(tid), row, lds);
    else interleaved_low_words<LOGS, true>(v, tid, row);
}

// SOURCE: kInverseFromSlab, or the fused loads of ntt_inverse_tiled -- kInverseFromTensor (the BEHZ tensor product) and
// kInverseFromKeyMac (the lazy inner product with the key-switching key) -- formed in the low-pass layout of the sub-rows: the
// words (element i, sub-rows h, h + 1) are 16 contiguous bytes of every source row.
template <int LOGS, int MODE, bool SCALED, int SOURCE = kInverseFromSlab>
__global__ void __launch_bounds__(1 << kSubLogT, min_waves_per_simd(kSubLogE, 1 << LOGS))
    ntt_inverse_interleaved(uint64_t* __restrict__ slab, const DeviceContext ctx, const RowMap map, const InverseSource source_spec) {
    constexpr int ROWS = 1 << LOGS, LOGD = kSubLogN + LOGS, E = 1 << kSubLogE, R = Schedule<kSubLogN, kSubLogE>::R;
    constexpr bool TENSOR = SOURCE == kInverseFromTensor, KEYMAC = SOURCE == kInverseFromKeyMac;
    static_assert(SOURCE == kInverseFromSlab || TENSOR || KEYMAC, "the key switch's end stays with the tiled kernel");
    static_assert(!TENSOR || SCALED, "the fused tensor load belongs to dropExtendedBase (t N^-1)");
    constexpr int INPUT_STAGES = (TENSOR || KEYMAC) && kLazyTransformInput<MODE> ? kLazyInputStages : 0;
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
    const uint32_t tid = threadIdx.x;
    uint32_t record, within;
    size_t rows[1];
    if constexpr (TENSOR || KEYMAC) {
        constexpr uint32_t REPLICAS = TENSOR ? 3 : 2;  // records (item, c) of one item read the same source rows
        uint32_t set, c, group;
        locate_replica(blockIdx.x, gridDim.x / REPLICAS, REPLICAS, set, c);
        locate(map, set, group, within);
        record = (map.record_base + group) * REPLICAS + c;
        rows[0] = size_t(record) * map.record_rows + map.band_offset + within;
    } else {
        locate_rows<1>(map, blockIdx.x, rows, record, within);
    }
    const uint32_t mi = map.mod_base + within;
    const DeviceModulus mod = ctx.moduli[mi];
    const Twiddles<MODE> cross(ctx, true, mi, LOGD);
    const Twiddles<MODE> tail(ctx, true, mi, LOGD, (1u << LOGD) - (1u << kSubLogN), kInterleavedLaneMajor<MODE>);
    const BufferResource row = make_resource(slab + (rows[0] << LOGD), 8u << LOGD);
    // (before the row's loads where the registers allow it: the plain slab on the shift-folded products -- a fused load needs
    // them for its operands, a limb-wise twiddle is 6 registers)
    constexpr bool EARLY_HEAD = SOURCE == kInverseFromSlab && (MODE == kModeFoldLazy || kCrossEarlySplit);
    TwiddleWords cross_head[kCrossAheadInverse<MODE>];
    if constexpr (EARLY_HEAD) inverse_cross_head<LOGS, MODE>(cross_head, tid, cross);
    uint64_t v[ROWS][E];
    if constexpr (TENSOR) {
        const size_t item = record / 3;
        const uint32_t c = static_cast<uint32_t>(record - item * 3);  // wave-uniform
        const size_t poly_words = static_cast<size_t>(map.record_rows) << LOGD;
        const uint64_t* const source = source_spec.first + item * 4 * poly_words + (static_cast<size_t>(map.band_offset + within) << LOGD);
        const uint32_t lane_words = lane_part<kSubLogN, kSubLogE, 0, R>(tid) << LOGS;
        auto reduce = [&](const ProductSum& sum) {
            if constexpr (kLazyTransformInput<MODE>) return reduce_product_sum_bounded_lazy(sum, mod);
            else return mod.wide_shift != 0 ? reduce_product_sum_bounded(sum, mod) : reduce_product_sum(sum, mod);  // wave-uniform
        };
#pragma unroll
        for (int r = 0; r < E; ++r) {
#pragma unroll
            for (int h = 0; h < ROWS; h += 2) {
                const size_t at = (register_part<kSubLogN, kSubLogE, 0, R>(r) << LOGS) + lane_words + h;
                if (c != 1) {
                    const U64x2 a = *reinterpret_cast<const U64x2*>(source + (c == 0 ? 0 : 1) * poly_words + at);
                    const U64x2 b = *reinterpret_cast<const U64x2*>(source + (c == 0 ? 2 : 3) * poly_words + at);
                    if constexpr (kLazyTransformInput<MODE>) {
                        v[h][r] = reduce_product_sum_bounded_lazy(product_sum_first(a.x, b.x), mod);
                        v[h + 1][r] = reduce_product_sum_bounded_lazy(product_sum_first(a.y, b.y), mod);
                    } else {
                        v[h][r] = barrett_mul(a.x, b.x, mod.p, mod.product_factor, static_cast<int>(mod.product_shift));
                        v[h + 1][r] = barrett_mul(a.y, b.y, mod.p, mod.product_factor, static_cast<int>(mod.product_shift));
                    }
                } else {
                    const U64x2 a0 = *reinterpret_cast<const U64x2*>(source + at);
                    const U64x2 a1 = *reinterpret_cast<const U64x2*>(source + poly_words + at);
                    const U64x2 b0 = *reinterpret_cast<const U64x2*>(source + 2 * poly_words + at);
                    const U64x2 b1 = *reinterpret_cast<const U64x2*>(source + 3 * poly_words + at);
                    ProductSum cross0 = product_sum_first(a0.x, b1.x), cross1 = product_sum_first(a0.y, b1.y);
                    product_sum_add(cross0, a1.x, b0.x);
                    product_sum_add(cross1, a1.y, b0.y);
                    v[h][r] = reduce(cross0);
                    v[h + 1][r] = reduce(cross1);
                }
            }
        }
    } else if constexpr (KEYMAC) {
        const size_t poly = record >> 1, c = record & 1;  // record = poly * 2 + c
        const uint32_t L = source_spec.L, top_rows = source_spec.top_rows;
        const uint32_t band_row = map.band_offset + within;
        const uint32_t key_row = (band_row == L) ? top_rows - 1 : band_row;  // Bfv+Keys.swift:153
        const uint32_t lane_words = lane_part<kSubLogN, kSubLogE, 0, R>(tid) << LOGS;
        const bool bounded = kKeyMacBoundedReduce && mod.wide_shift != 0 && L <= 8 && uint64_t(L) * mod.p < (uint64_t(1) << 63);  // wave-uniform
#pragma unroll
        for (int r = 0; r < E; ++r) {
#pragma unroll
            for (int h = 0; h < ROWS; h += 2) {
                const uint32_t at = (register_part<kSubLogN, kSubLogE, 0, R>(r) << LOGS) + h;
                // the words of term j + 1 are requested before term j is accumulated (ntt_inverse_tiled)
                const uint64_t* const flat_spread = source_spec.first + ((poly * L * (L + 1) + band_row) << LOGD) + lane_words + at;
                const uint64_t* const flat_key = source_spec.second + ((c * top_rows + key_row) << LOGD) + lane_words + at;
                U64x2 xs = *reinterpret_cast<const U64x2*>(flat_spread);
                U64x2 ks = *reinterpret_cast<const U64x2*>(flat_key);
                ProductSum acc0 = product_sum_zero(), acc1 = product_sum_zero();
                for (uint32_t j = 0; j < L; ++j) {
                    const uint32_t ahead = j + 1 < L ? j + 1 : j;
                    const U64x2 xn = *reinterpret_cast<const U64x2*>(flat_spread + ((size_t(ahead) * (L + 1)) << LOGD));
                    const U64x2 kn = *reinterpret_cast<const U64x2*>(flat_key + ((size_t(ahead) * 2 * top_rows) << LOGD));
                    product_sum_add_one<is_split(MODE)>(acc0, xs.x, ks.x);
                    product_sum_add_one<is_split(MODE)>(acc1, xs.y, ks.y);
                    xs = xn;
                    ks = kn;
                }
                if (bounded) {
                    if constexpr (kLazyTransformInput<MODE>) {
                        v[h][r] = reduce_product_sum_bounded_lazy(acc0, mod);
                        v[h + 1][r] = reduce_product_sum_bounded_lazy(acc1, mod);
                    } else {
                        v[h][r] = reduce_product_sum_bounded(acc0, mod);
                        v[h + 1][r] = reduce_product_sum_bounded(acc1, mod);
                    }
                } else {
                    v[h][r] = reduce_product_sum(acc0, mod);
                    v[h + 1][r] = reduce_product_sum(acc1, mod);
                }
            }
        }
    } else {
        if constexpr (kInterleavedStaged) interleaved_low_words_staged<LOGS, false>(v, tid, row, lds);
        else interleaved_low_words<LOGS, false>(v, tid, row);
    }
    if constexpr (!EARLY_HEAD) inverse_cross_head<LOGS, MODE>(cross_head, tid, cross);
    inverse_cross_stages<LOGS, MODE, INPUT_STAGES>(v, tid, cross, mod.p, cross_head);
    TwiddleWords head[1];
    inverse_row_head<kSubLogN, kSubLogE, MODE, false, 1>(head, tail, tid);
    // (two sub-rows on the shift-folded products: every step re-derives the lane index, as the key-MAC transforms -- step_lane)
    constexpr bool LATE = ROWS == 2 && MODE == kModeFoldLazy;
    inverse_row<kSubLogN, kSubLogE, MODE, ROWS, SCALED, LOGS + INPUT_STAGES, LOGD, false, 1, LATE>(v, tid, tail, mod, lds, head);
    interleaved_top_words<LOGS, true>(v, LATE ? late_lane(tid) : tid, row);
}

// (four sub-rows -- N = 32768, one workgroup per CU at 128 registers -- go through two tiles side by side like the row groups
// of behz_kernels.hip: ntt_rows.hpp kGroupTiles)
template <int LOGS>
constexpr size_t kInterleavedLdsBytes = kGroupTiles<(1 << LOGS)> * lds_words(1u << kSubLogN) * sizeof(uint64_t);

}  // namespace

template <int LOGS, int SPREAD>
hipError_t launch_interleaved_forward(int mode, uint64_t* slab, const DeviceContext& ctx, const RowMap& map, size_t rows,
                                      const SpreadSource& spread, hipStream_t stream) {
    auto kernel = mode == kModeSplit    ? ntt_forward_interleaved<LOGS, kModeSplit, SPREAD>
                  : mode == kModeApprox ? ntt_forward_interleaved<LOGS, kModeApprox, SPREAD>
                                        : ntt_forward_interleaved<LOGS, kModeExact, SPREAD>;
    if constexpr (kFoldLazyInterleaved) {
        if (mode == kModeSplit && fold_lazy_band(ctx, map)) kernel = ntt_forward_interleaved<LOGS, kModeFoldLazy, SPREAD>;
    }
    if constexpr (kFoldPlusInterleaved && SPREAD == kSourceSlab) {
        // the BEHZ primes 2^60 + e (the Bsk band of a lifted record, transformed in place) on the fold butterflies, as at N = 8192
        if (mode == kModeApprox && ctx.forward_split_pairs != nullptr && fold_mode(ctx, map.mod_base, map.band_rows) == kModeFoldPlus)
            kernel = ntt_forward_interleaved<LOGS, kModeFoldPlus, SPREAD>;
    }
    if (hipError_t e = allow_dynamic_lds(kernel, kInterleavedLdsBytes<LOGS>); e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(rows)), dim3(1u << kSubLogT), kInterleavedLdsBytes<LOGS>, stream, slab, ctx, map,
                       spread);
    return hipGetLastError();
}
template <int LOGS, int SOURCE>
hipError_t launch_interleaved_inverse(int mode, uint64_t* slab, const DeviceContext& ctx, const RowMap& map, size_t rows,
                                      const InverseSource& source_spec, hipStream_t stream) {
    using Kernel = void (*)(uint64_t*, const DeviceContext, const RowMap, const InverseSource);
    Kernel kernel;
    if constexpr (SOURCE == kInverseFromTensor) {
        if (ctx.scaled_inverse_degree == 0) return hipErrorInvalidValue;  // the fused tensor load belongs to dropExtendedBase
        kernel = mode == kModeSplit    ? ntt_inverse_interleaved<LOGS, kInterleavedInverseSplit, true, SOURCE>
                 : mode == kModeApprox ? ntt_inverse_interleaved<LOGS, kModeApprox, true, SOURCE>
                                       : ntt_inverse_interleaved<LOGS, kModeExact, true, SOURCE>;
    } else if constexpr (SOURCE == kInverseFromKeyMac) {
        if (ctx.scaled_inverse_degree != 0) return hipErrorInvalidValue;  // the key-switching contexts are never scaled
        kernel = mode == kModeSplit    ? ntt_inverse_interleaved<LOGS, kInterleavedInverseSplit, false, SOURCE>
                 : mode == kModeApprox ? ntt_inverse_interleaved<LOGS, kModeApprox, false, SOURCE>
                                       : ntt_inverse_interleaved<LOGS, kModeExact, false, SOURCE>;
    } else if (ctx.scaled_inverse_degree != 0) {
        kernel = mode == kModeSplit    ? ntt_inverse_interleaved<LOGS, kInterleavedInverseSplit, true, SOURCE>
                 : mode == kModeApprox ? ntt_inverse_interleaved<LOGS, kModeApprox, true, SOURCE>
                                       : ntt_inverse_interleaved<LOGS, kModeExact, true, SOURCE>;
    } else {
        kernel = mode == kModeSplit    ? ntt_inverse_interleaved<LOGS, kInterleavedInverseSplit, false, SOURCE>
                 : mode == kModeApprox ? ntt_inverse_interleaved<LOGS, kModeApprox, false, SOURCE>
                                       : ntt_inverse_interleaved<LOGS, kModeExact, false, SOURCE>;
    }
    if constexpr (kFoldLazyInterleaved) {
        if (mode == kModeSplit && fold_lazy_band(ctx, map)) {
            constexpr bool ALWAYS_SCALED = SOURCE == kInverseFromTensor, NEVER_SCALED = SOURCE == kInverseFromKeyMac;
            if constexpr (ALWAYS_SCALED) kernel = ntt_inverse_interleaved<LOGS, kModeFoldLazy, true, SOURCE>;
            else if constexpr (NEVER_SCALED) kernel = ntt_inverse_interleaved<LOGS, kModeFoldLazy, false, SOURCE>;
            else kernel = ctx.scaled_inverse_degree != 0 ? ntt_inverse_interleaved<LOGS, kModeFoldLazy, true, SOURCE>
                                                         : ntt_inverse_interleaved<LOGS, kModeFoldLazy, false, SOURCE>;
        }
    }
    if constexpr (kFoldPlusInterleaved && (SOURCE == kInverseFromSlab || SOURCE == kInverseFromTensor)) {
        if (mode == kModeApprox && ctx.forward_split_pairs != nullptr && fold_mode(ctx, map.mod_base, map.band_rows) == kModeFoldPlus) {
            if constexpr (SOURCE == kInverseFromTensor) kernel = ntt_inverse_interleaved<LOGS, kModeFoldPlus, true, SOURCE>;
            else kernel = ctx.scaled_inverse_degree != 0 ? ntt_inverse_interleaved<LOGS, kModeFoldPlus, true, SOURCE>
                                                         : ntt_inverse_interleaved<LOGS, kModeFoldPlus, false, SOURCE>;
        }
    }
    if (hipError_t e = allow_dynamic_lds(kernel, kInterleavedLdsBytes<LOGS>); e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(rows)), dim3(1u << kSubLogT), kInterleavedLdsBytes<LOGS>, stream, slab, ctx, map,
                       source_spec);
    return hipGetLastError();
}

#define HEAMD_INTERLEAVED_FORWARD(LOGS, SPREAD)                                                                                \
    template hipError_t launch_interleaved_forward<LOGS, SPREAD>(int, uint64_t*, const DeviceContext&, const RowMap&, size_t, \
                                                                 const SpreadSource&, hipStream_t)
#define HEAMD_INTERLEAVED_INVERSE(LOGS, SOURCE)                                                                                \
    template hipError_t launch_interleaved_inverse<LOGS, SOURCE>(int, uint64_t*, const DeviceContext&, const RowMap&, size_t, \
                                                                 const InverseSource&, hipStream_t)

}  // namespace heamd
