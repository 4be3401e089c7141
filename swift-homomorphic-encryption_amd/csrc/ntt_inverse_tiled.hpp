// ntt_inverse_tiled.hpp -- the register-tiled inverse transform with its fused loads and the key switch's fused end
// (ntt_sources.hpp), and the selector that names it.
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

// Byte offset of argument INDEX of a kernel in its kernel-argument segment (arguments in order, each at its natural
// alignment), from the kernel's own type; the number of arguments.
template <size_t INDEX, typename... Args>
constexpr size_t kernarg_offset(void (*)(Args...)) {
    constexpr size_t sizes[] = {sizeof(Args)...}, aligns[] = {alignof(Args)...};
    size_t at = 0;
    for (size_t k = 0; k <= INDEX; ++k) {
        at = (at + aligns[k] - 1) / aligns[k] * aligns[k];
        if (k < INDEX) at += sizes[k];
    }
    return at;
}
template <typename... Args>
constexpr size_t kernarg_count(void (*)(Args...)) { return sizeof...(Args); }

template <int LOGN, int LOGT, int MODE, int SOURCE = kInverseFromSlab, int ROWS = 1>
__global__ void __launch_bounds__(1 << LOGT, min_waves_per_simd(LOGN - LOGT, ROWS))
    ntt_inverse_tiled(uint64_t* __restrict__ slab, const DeviceContext ctx, const RowMap map,
                      const InverseSource source_spec) {
    constexpr bool TENSOR = SOURCE == kInverseFromTensor;
    constexpr bool SCALED = SOURCE == kInverseFromTensor || SOURCE == kInverseFromSlabScaled;
    constexpr bool FROM_SLAB = SOURCE == kInverseFromSlab || SOURCE == kInverseFromSlabScaled;
    constexpr bool KEYMAC = is_key_mac(SOURCE), FINISH = SOURCE == kInverseFromKeyMacFinish;
    constexpr int INPUT_STAGES = (TENSOR || KEYMAC) && kLazyTransformInput<MODE> ? kLazyInputStages : 0;
    constexpr bool LATE = KEYMAC && ROWS == 2;  // (ntt_rows.hpp step_lane)
    static_assert(ROWS == 1 || SOURCE != kInverseFromSlabScaled, "scaled plain slabs go one row per workgroup");
    const uint64_t* __restrict__ tensor_source = source_spec.first;
    constexpr int LOGE = LOGN - LOGT;
    constexpr int E = 1 << LOGE;
    using S = Schedule<LOGN, LOGE>;
    using O = PassOrder<LOGN, LOGE, kTopPartialOrder<LOGN, LOGE, true, FROM_SLAB>>;
    constexpr int LOW = O::LOW;  // the width of the pass on the low bits: the layout the rows are loaded in
    static_assert(S::P >= 1 && S::P <= 5, "unsupported pass count");
    extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
    const uint32_t tid = threadIdx.x;
    uint32_t record, within;
    size_t rows[ROWS];
    if constexpr (!FROM_SLAB) {
        // records (item, c) of one item read the same source rows: one replica set per (group of ROWS consecutive
        // items, band row); the workgroup transforms record (item + k, c) for k < ROWS
        constexpr uint32_t REPLICAS = TENSOR ? 3 : 2;
        uint32_t set, c, group;
        locate_replica(blockIdx.x, gridDim.x / REPLICAS, REPLICAS, set, c);
        locate(map, set, group, within);
        record = (map.record_base + group * ROWS) * REPLICAS + c;  // of the first item; record_base counts items here
#pragma unroll
        for (int k = 0; k < ROWS; ++k)
            rows[k] = size_t(record + k * REPLICAS) * map.record_rows + map.band_offset + within;
    } else {
        locate_rows<ROWS>(map, blockIdx.x, rows, record, within);
    }
    const uint32_t mi = map.mod_base + within;
    const DeviceModulus mod = ctx.moduli[mi];
    const Twiddles<MODE> tw(ctx, true, mi, LOGN, 0, kLaneMajorTwiddles<LOGN, LOGT, MODE, true, FROM_SLAB>);
    uint64_t v[ROWS][E];

    if constexpr (S::P == 1) {
        const BufferResource x = make_resource(slab + (rows[0] << LOGN), 8u << LOGN);
        global_load<LOGN, LOGE, 0, LOGN>(v[0], tid, x);
        const TwiddleWords head[1] = {inverse_first_twiddle<LOGN, LOGE, 0, LOGN, MODE, false>(tw, tid)};
        inverse_pass<LOGN, LOGE, 0, LOGN, MODE, false, 1, SCALED, 0, LOGN, 0, 1>(v, tid, tw, mod, true, head);
        global_store<LOGN, LOGE, 0, LOGN>(v[0], tid, x);
    } else {
        // every transpose but the last one (into the top pass) stays inside a wave
        constexpr int HEAD = kInverseHeadTwiddles<LOGN, LOGE, MODE, SOURCE, ROWS>;
        TwiddleWords head[HEAD];
        if constexpr (HEAD > 1) inverse_row_head<LOGN, LOGE, MODE, O::kTop, HEAD>(head, tw, tid);
        if constexpr (TENSOR) {
            const size_t first_item = record / 3;
            const uint32_t c = static_cast<uint32_t>(record - first_item * 3);  // wave-uniform
            const size_t poly_words = static_cast<size_t>(map.record_rows) << LOGN;
            const uint64_t p = mod.p, factor = mod.product_factor;
            const int shift = static_cast<int>(mod.product_shift);
            const uint32_t lane_words = lane_part<LOGN, LOGE, 0, LOW>(tid);
#pragma unroll
            for (int k = 0; k < ROWS; ++k) {
                const uint64_t* const source = tensor_source + (first_item + k) * 4 * poly_words +
                                               (static_cast<size_t>(map.band_offset + within) << LOGN);
#pragma unroll
                for (int r = 0; r < E; r += 2) {
                    const size_t at = register_part<LOGN, LOGE, 0, LOW>(r) + lane_words;
                    if (c != 1) {
                        const U64x2 a = *reinterpret_cast<const U64x2*>(source + (c == 0 ? 0 : 1) * poly_words + at);
                        const U64x2 b = *reinterpret_cast<const U64x2*>(source + (c == 0 ? 2 : 3) * poly_words + at);
                        if constexpr (kLazyTransformInput<MODE>) {
                            // (these moduli are 41 .. 61 bits: wide_shift != 0, p^2 inside the bounded reduction's range)
                            v[k][r] = reduce_product_sum_bounded_lazy(product_sum_first(a.x, b.x), mod);
                            v[k][r + 1] = reduce_product_sum_bounded_lazy(product_sum_first(a.y, b.y), mod);
                        } else {
                            v[k][r] = barrett_mul(a.x, b.x, p, factor, shift);
                            v[k][r + 1] = barrett_mul(a.y, b.y, p, factor, shift);
                        }
                    } else {
                        const U64x2 a0 = *reinterpret_cast<const U64x2*>(source + at);
                        const U64x2 a1 = *reinterpret_cast<const U64x2*>(source + poly_words + at);
                        const U64x2 b0 = *reinterpret_cast<const U64x2*>(source + 2 * poly_words + at);
                        const U64x2 b1 = *reinterpret_cast<const U64x2*>(source + 3 * poly_words + at);
                        // a0 b1 + a1 b0 as one exact 128-bit sum and one reduction (two products < 2^125); below 2^61 the
                        // sum 2 p^2 is inside the one-word-quotient Barrett's bound 2^(64 + wide_shift)
                        ProductSum cross0 = product_sum_first(a0.x, b1.x), cross1 = product_sum_first(a0.y, b1.y);
                        product_sum_add(cross0, a1.x, b0.x);
                        product_sum_add(cross1, a1.y, b0.y);
                        if constexpr (kLazyTransformInput<MODE>) {
                            v[k][r] = reduce_product_sum_bounded_lazy(cross0, mod);
                            v[k][r + 1] = reduce_product_sum_bounded_lazy(cross1, mod);
                        } else if (mod.wide_shift != 0) {  // wave-uniform
                            v[k][r] = reduce_product_sum_bounded(cross0, mod);
                            v[k][r + 1] = reduce_product_sum_bounded(cross1, mod);
                        } else {
                            v[k][r] = reduce_product_sum(cross0, mod);
                            v[k][r + 1] = reduce_product_sum(cross1, mod);
                        }
                    }
                }
            }
        } else if constexpr (KEYMAC) {
            const size_t first_poly = record >> 1, c = record & 1;  // record = poly * 2 + c
            const uint32_t L = source_spec.L, top_rows = source_spec.top_rows;
            const uint32_t r = map.band_offset + within;
            const uint32_t key_row = (r == L) ? top_rows - 1 : r;  // Bfv+Keys.swift:153
            // (flat 64-bit addresses: the same loads through scalar buffer descriptors with a scalar offset per term --
            // no address arithmetic on the vector ALU -- measured 1.4 % slower, profiles/r04j_keymac_loads_and_column_words_ab.txt)
            const uint32_t lane_words = lane_part<LOGN, LOGE, 0, LOW>(tid);
#pragma unroll
            for (int k = 0; k < ROWS; ++k) {
#pragma unroll
                for (int q = 0; q < E; q += 2) {
                    const uint32_t at = register_part<LOGN, LOGE, 0, LOW>(q);
                    // the words of term j + 1 are requested before term j is accumulated (the count L is a run-time
                    // value: the loop is not unrolled, and without the request ahead every term would wait out its own
                    // L2 round trip); past the last term the request repeats it -- a load behind a branch would drain
                    // the queue
                    const uint64_t* const flat_spread =
                        source_spec.first + (((first_poly + k) * L * (L + 1) + r) << LOGN) + lane_words + at;  // + j (L+1) N
                    const uint64_t* const flat_key =
                        source_spec.second + ((c * top_rows + key_row) << LOGN) + lane_words + at;          // + j 2 top_rows N
                    U64x2 xs = *reinterpret_cast<const U64x2*>(flat_spread);
                    U64x2 ks = *reinterpret_cast<const U64x2*>(flat_key);
                    ProductSum acc0 = product_sum_zero(), acc1 = product_sum_zero();
                    for (uint32_t j = 0; j < L; ++j) {
                        const uint32_t ahead = j + 1 < L ? j + 1 : j;
                        const U64x2 xn = *reinterpret_cast<const U64x2*>(flat_spread + ((size_t(ahead) * (L + 1)) << LOGN));
                        const U64x2 kn = *reinterpret_cast<const U64x2*>(flat_key + ((size_t(ahead) * 2 * top_rows) << LOGN));
                        // (limb-wise schedule = every modulus below 2^55: canonical operands keep the middle column of a
                        // sum from wrapping for 127 products, so its carry counts are not kept -- 5 instructions per
                        // product instead of 7; L <= 64 terms stay inside kNarrowProductSumCadence)
                        product_sum_add_one<is_split(MODE)>(acc0, xs.x, ks.x);
                        product_sum_add_one<is_split(MODE)>(acc1, xs.y, ks.y);
                        xs = xn;
                        ks = kn;
                    }
                    // (the one-word-quotient Barrett where the sum allows it: L products of canonical words stay below
                    // L p^2 < 2^(64 + wide_shift) = 2^(63 + bits(p)) whenever L p < 2^63)
                    if (kKeyMacBoundedReduce && mod.wide_shift != 0 && L <= 8 && uint64_t(L) * mod.p < (uint64_t(1) << 63)) {  // wave-uniform
                        if constexpr (kLazyTransformInput<MODE>) {
                            v[k][q] = reduce_product_sum_bounded_lazy(acc0, mod);
                            v[k][q + 1] = reduce_product_sum_bounded_lazy(acc1, mod);
                        } else {
                            v[k][q] = reduce_product_sum_bounded(acc0, mod);
                            v[k][q + 1] = reduce_product_sum_bounded(acc1, mod);
                        }
                    } else {
                        v[k][q] = reduce_product_sum(acc0, mod);
                        v[k][q + 1] = reduce_product_sum(acc1, mod);
                    }
                }
            }
        } else {
            [[maybe_unused]] const uint64_t p = mod.p;
            // (plain slabs may be transformed OUT OF PLACE: rows read from source_spec.first, laid out like the slab, when it is set)
            const uint64_t* load_base = slab;
            if constexpr (SOURCE == kInverseFromSlab) load_base = tensor_source != nullptr ? tensor_source : slab;
#pragma unroll
            for (int k = 0; k < ROWS; ++k) {
                const BufferResource in = make_resource(load_base + (rows[k] << LOGN), 8u << LOGN);
                if constexpr (kStagedLoad<LOGN, LOGE, LOW>) {
                    global_load_staged<LOGN, LOGE, LOW>(v[k], tid, in, lds);
                } else {
                    global_load<LOGN, LOGE, 0, LOW>(v[k], tid, in);
                }
            }
        }
        if constexpr (HEAD == 1) inverse_row_head<LOGN, LOGE, MODE, O::kTop, HEAD>(head, tw, tid);
        constexpr int LOL = LOGN - LOGE;
        if constexpr (FINISH) {
            // key_switch_finish_kernel's arithmetic (rns_kernels.hip) on each row as its last pass completes: with x_ks the
            // q_ks word of the coefficient and c its centred representative, out = (x - c) q_ks^-1 mod q_r (+ the ciphertext
            // word).  |c| <= q_ks / 2 needs a reduction mod q_r only where q_r is the smaller one (`wide`, wave-uniform: the
            // 29-bit modulus next to the 60-bit ones of the reference's n_8192_logq_29_60_60); the word loop exists in both
            // forms.
            // The end's parameters are read from the kernel-argument segment WHERE THEY ARE USED (scalar loads off the segment's
            // base), not as kernel arguments: those are all loaded in the entry block, and this kernel then parks them in
            // vector-register lanes across the whole transform -- two of its 64 registers, paid for in scratch.
            struct KernelArguments {
                uint64_t* slab;
                DeviceContext ctx;
                RowMap map;
                InverseSource source_spec;
            };
            // The AMDGPU kernel-argument segment lays the arguments out in order, each at its natural alignment -- the rule
            // of a C++ struct with the same members.  kernarg_offset derives the offset of argument 3 from THIS kernel's own
            // parameter list: adding, removing or reordering a parameter without touching the mirror fails here, not at run
            // time with garbage in out / ct_base / poly_base.
            using ThisKernel = decltype(&ntt_inverse_tiled<LOGN, LOGT, MODE, SOURCE, ROWS>);
            static_assert(kernarg_offset<3>(static_cast<ThisKernel>(nullptr)) == offsetof(KernelArguments, source_spec) &&
                              kernarg_count(static_cast<ThisKernel>(nullptr)) == 4,
                          "KernelArguments must mirror ntt_inverse_tiled's parameter list");
            static_assert(std::is_trivially_copyable<InverseSource>::value && std::is_standard_layout<KernelArguments>::value,
                          "kernel arguments are copied byte for byte into the segment");
            using ConstSpec = const __attribute__((address_space(4))) InverseSource;
            using ConstByte = const __attribute__((address_space(4))) char;
            ConstSpec* const end_spec = (ConstSpec*)((ConstByte*)__builtin_amdgcn_kernarg_segment_ptr() +
                                                     offsetof(KernelArguments, source_spec));
            const uint32_t L = source_spec.L, r = map.band_offset + within;
            const uint64_t p = mod.p, q_last = ctx.moduli[L].p, half = q_last >> 1;
            const U64x2 inverse_q_last = load_twiddle(ctx.inverse_q_last + size_t(L) * ctx.moduli_stride + r);
            const bool wide = half >= p;
            constexpr int kEndPlain = 0, kEndGalois = 1, kEndExpand = 2;
            auto finish = [&](int k, uint64_t (&row)[E]) {
                const uint32_t lane = step_lane<MODE, LATE>(tid);
                const uint32_t lane_words = lane_part<LOGN, LOGE, LOL, LOGE>(lane), lane_bytes = lane_words << 3;
                constexpr int CHUNK = 4;  // words in flight: the q_ks and ciphertext words of a chunk are requested together
                auto word = [](Dwordx2 w) { return pack64(w.x, w.y); };
                const size_t pc = record + 2 * k;  // polynomial * 2 + c (the rows are the same column of consecutive polynomials)
                const size_t poly = end_spec->poly_base + (pc >> 1);  // in the ciphertext / output slabs
                const uint32_t c = static_cast<uint32_t>(pc & 1);
                const BufferResource last_row = make_resource(slab + ((pc * (L + 1) + L) << LOGN), 8u << LOGN);
                const uint32_t galois_inverse = end_spec->galois_inverse, expand_shift = end_spec->expand_shift;
                // polynomial c of the ciphertext: added as it lies (relinearize), or -- c0 under an automorphism -- gathered
                const bool gathered = galois_inverse != 0 && c == 0;
                const bool add = galois_inverse != 0 ? gathered : c < end_spec->added_polys;  // wave-uniform
                const BufferResource added_row =
                    add ? make_resource(end_spec->ct_base + poly * end_spec->ct_stride + ((size_t(c) * L + r) << LOGN), 8u << LOGN)
                        : last_row;  // (without an addend the q_ks row is read twice)
                auto words_of_row = [&](auto reduce_magnitude, auto end_tag) {
                    constexpr int END = decltype(end_tag)::value;
                    // where the row goes: polynomial c of ciphertext `poly`, or -- an expand step -- of its two children.  The
                    // descriptors are built inside the end that uses them: held across all three they cost scalar registers
                    // that this kernel parks in vector-register lanes
                    size_t first_ct = poly, second_ct = 0;
                    [[maybe_unused]] bool first_doubled = false, second_doubled = false;
                    if constexpr (END == kEndExpand) {
                        first_ct = 2 * poly;
                        second_ct = 2 * poly + 1;
                        if (end_spec->targets_table != nullptr) {
                            using ConstWord = const __attribute__((address_space(4))) uint32_t;
                            const size_t group = poly / end_spec->targets_group_size, parent = poly - group * end_spec->targets_group_size;
                            const uint32_t first = *(ConstWord*)(end_spec->targets_table + 4 * parent + 1);
                            const uint32_t second = *(ConstWord*)(end_spec->targets_table + 4 * parent + 3);
                            first_ct = group * end_spec->targets_group_stride + (first >> 1);
                            second_ct = group * end_spec->targets_group_stride + (second >> 1);
                            first_doubled = (first & 1u) != 0;
                            second_doubled = (second & 1u) != 0;
                        }
                    }
                    const BufferResource out_row = make_uniform_resource(end_spec->out + (((first_ct * 2 + c) * L + r) << LOGN), 8u << LOGN);
                    [[maybe_unused]] BufferResource moved_row = out_row, own_row = last_row;
                    if constexpr (END == kEndExpand) {
                        moved_row = make_uniform_resource(end_spec->out + (((second_ct * 2 + c) * L + r) << LOGN), 8u << LOGN);
                        own_row = make_resource(end_spec->own_base + poly * end_spec->ct_stride + ((size_t(c) * L + r) << LOGN), 8u << LOGN);
                    }
#pragma unroll
                    for (int base = 0; base < E; base += CHUNK) {
                        uint64_t last[CHUNK], added[CHUNK];
                        [[maybe_unused]] uint64_t own[CHUNK];
                        [[maybe_unused]] bool negate[CHUNK];
#pragma unroll
                        for (int e = 0; e < CHUNK; ++e) {
                            const uint32_t at = register_part<LOGN, LOGE, LOL, LOGE>(base + e) << 3;
                            last[e] = word(__builtin_amdgcn_raw_buffer_load_b64(last_row, lane_bytes, at, row_load_policy<LOGN>()));
                            if constexpr (END == kEndPlain) {
                                added[e] = word(__builtin_amdgcn_raw_buffer_load_b64(added_row, lane_bytes, at, row_load_policy<LOGN>()));
                            } else {
                                // coefficient idx of galois(c0) = -+ coefficient idx g^-1 mod 2N of c0 (row c = 1: not used)
                                const uint32_t idx = register_part<LOGN, LOGE, LOL, LOGE>(base + e) | lane_words;
                                const uint32_t doubled = (idx * galois_inverse) & ((2u << LOGN) - 1u);
                                negate[e] = (doubled >> LOGN) != 0;
                                added[e] = word(__builtin_amdgcn_raw_buffer_load_b64(added_row, (doubled & ((1u << LOGN) - 1u)) << 3, 0, 0));
                                if constexpr (END == kEndExpand)
                                    own[e] = word(__builtin_amdgcn_raw_buffer_load_b64(own_row, lane_bytes, at, row_load_policy<LOGN>()));
                            }
                        }
#pragma unroll
                        for (int e = 0; e < CHUNK; ++e) {
                            const uint32_t at = register_part<LOGN, LOGE, LOL, LOGE>(base + e) << 3;
                            // straight-line: x - c = x + (c < 0 ? |c| : p - |c|) mod p, an absent addend is zero
                            const uint64_t shifted = add_mod_uniform(last[e], half, q_last);
                            const bool negative = shifted < half;
                            uint64_t t = negative ? half - shifted : shifted - half;
                            if constexpr (decltype(reduce_magnitude)::value) t = barrett_reduce64_uniform(t, p, mod.barrett64);
                            const uint64_t difference = csub_uniform(row[base + e] + (negative ? t : p - t), p);
                            const uint64_t update = shoup_mul_uniform(difference, inverse_q_last.x, inverse_q_last.y, p);
                            uint64_t addend = add ? added[e] : 0;
                            if constexpr (END != kEndPlain) addend = negate[e] && addend != 0 ? p - addend : addend;
                            const uint64_t result = csub_uniform(addend + update, p);  // c' (or ct + update)
                            if constexpr (END != kEndExpand) {
                                const Dwordx2 words = {lo32(result), hi32(result)};
                                __builtin_amdgcn_raw_buffer_store_b64(words, out_row, lane_bytes, at, row_policy<LOGN>());
                            } else {
                                // children own + c' and (own - c') x^shift: the second one lands at idx + shift mod 2N,
                                // negated past N
                                uint64_t sum = csub_uniform(own[e] + result, p);
                                if (first_doubled) sum = csub_uniform(sum + sum, p);
                                const Dwordx2 first_words = {lo32(sum), hi32(sum)};
                                __builtin_amdgcn_raw_buffer_store_b64(first_words, out_row, lane_bytes, at, row_policy<LOGN>());
                                const uint32_t idx = register_part<LOGN, LOGE, LOL, LOGE>(base + e) | lane_words;
                                const uint32_t landed = (idx + expand_shift) & ((2u << LOGN) - 1u);
                                uint64_t moved = csub_uniform(own[e] + (p - result), p);
                                moved = (landed >> LOGN) != 0 && moved != 0 ? p - moved : moved;
                                if (second_doubled) moved = csub_uniform(moved + moved, p);
                                const Dwordx2 moved_words = {lo32(moved), hi32(moved)};
                                __builtin_amdgcn_raw_buffer_store_b64(moved_words, moved_row, (landed & ((1u << LOGN) - 1u)) << 3, 0,
                                                                      row_policy<LOGN>());
                            }
                        }
                    }
                };
                auto with_end = [&](auto reduce_magnitude) {
                    if (expand_shift != 0) words_of_row(reduce_magnitude, std::integral_constant<int, kEndExpand>{});
                    else if (galois_inverse != 0) words_of_row(reduce_magnitude, std::integral_constant<int, kEndGalois>{});
                    else words_of_row(reduce_magnitude, std::integral_constant<int, kEndPlain>{});
                };
                if (wide) with_end(std::true_type{});
                else with_end(std::false_type{});
            };
            inverse_row<LOGN, LOGE, MODE, ROWS, SCALED, INPUT_STAGES, LOGN, O::kTop, HEAD, LATE>(v, tid, tw, mod, lds, head, finish);
        } else {
            inverse_row<LOGN, LOGE, MODE, ROWS, SCALED, INPUT_STAGES, LOGN, O::kTop, HEAD, LATE>(v, tid, tw, mod, lds, head);
            const uint32_t store_lane = step_lane<MODE, LATE>(tid);
#pragma unroll
            for (int k = 0; k < ROWS; ++k)
                global_store<LOGN, LOGE, LOL, LOGE>(v[k], store_lane, make_resource(slab + (rows[k] << LOGN), 8u << LOGN));
        }
    }
}

}  // namespace

template <int LOGN, int LOGT, int SOURCE, int ROWS>
hipError_t launch_inverse_kernel(int mode, uint64_t* slab, const DeviceContext& ctx, const RowMap& map, size_t workgroups,
                                 const InverseSource& source_spec, hipStream_t stream) {
    constexpr int LOGE = LOGN - LOGT;
    constexpr size_t lds_bytes = (Schedule<LOGN, LOGE>::P > 1) ? lds_words(1u << LOGN) * sizeof(uint64_t) : 0;
    // (the limb-wise inverse in its signed form wherever that measured faster: ntt_common.hpp kModeSplitSigned)
    constexpr int SPLIT = kSignedInverse<LOGN, SOURCE> ? kModeSplitSigned : kModeSplit;
    auto kernel = mode == kModeSplit    ? ntt_inverse_tiled<LOGN, LOGT, SPLIT, SOURCE, ROWS>
                  : mode == kModeApprox ? ntt_inverse_tiled<LOGN, LOGT, kModeApprox, SOURCE, ROWS>
                                        : ntt_inverse_tiled<LOGN, LOGT, kModeExact, SOURCE, ROWS>;
    if constexpr (kFoldLazyInverse<LOGN, LOGT, SOURCE>) {
        if (mode == kModeSplit && fold_lazy_band(ctx, map)) {
            kernel = ntt_inverse_tiled<LOGN, LOGT, kModeFoldLazy, SOURCE, ROWS>;
            if constexpr (kFoldLazyInverseMode<LOGN, LOGT, SOURCE> == kModeFoldSigned) {
                if (ctx.inverse_split_pairs_signed_lanes_top != nullptr) kernel = ntt_inverse_tiled<LOGN, LOGT, kModeFoldSigned, SOURCE, ROWS>;
            }
        }
    }
    if constexpr (kFoldShape<LOGN, LOGT>) {
        if (mode == kModeApprox && ctx.forward_split_pairs != nullptr) {
            const int fold = fold_mode(ctx, map.mod_base, map.band_rows);
            if (fold == kModeFoldMinus) kernel = ntt_inverse_tiled<LOGN, LOGT, kModeFoldMinus, SOURCE, ROWS>;
            if (fold == kModeFoldPlus) kernel = ntt_inverse_tiled<LOGN, LOGT, kModeFoldPlus, SOURCE, ROWS>;
        }
    }
    if (hipError_t e = allow_dynamic_lds(kernel, lds_bytes); e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(workgroups)), dim3(1u << LOGT), lds_bytes, stream, slab, ctx, map,
                       source_spec);
    return hipGetLastError();
}

#define HEAMD_INVERSE_TILED(LOGN, LOGT, SOURCE, ROWS)                                                                        \
    template hipError_t launch_inverse_kernel<LOGN, LOGT, SOURCE, ROWS>(int, uint64_t*, const DeviceContext&, const RowMap&, \
                                                                        size_t, const InverseSource&, hipStream_t)

}  // namespace heamd
