// bfv_api.cpp -- B3 entry points: Context<Bfv<UInt64>> and the HeScheme operations on the hot path
// (reference Sources/HomomorphicEncryption/Bfv/*.swift).  Each operation is a short pipeline of HIP kernels on the
// caller's stream; nothing here touches the data on the host.
#include <cmath>
#include <limits>
#include <memory>
#include <mutex>
#include <type_traits>
#include <vector>

#include "api_internal.hpp"
#include "bfv_context.hpp"
#include "decrypt_kernels.hpp"
#include "kernels.hpp"
#include "rns_kernels.hpp"
#include "side_lane.hpp"
#include "word_layer.hpp"

using heamd::as_stream;
using heamd::BfvContext;
using heamd::DeviceContext;
using heamd::DeviceImage;
using heamd::invalid_argument;
using heamd::PolyContext;
using heamd::RnsToolLevel;
using heamd::Scratch;
using heamd::SideLane;

struct he_bfv_context {
    std::unique_ptr<BfvContext> impl;
    // non-owning he_poly_context views handed out by he_bfv_*_context(), index = ciphertext moduli count
    std::vector<std::unique_ptr<he_poly_context>> ciphertext, key_switching, qbsk;
    mutable heamd::ExpandPlanCache expand_plans;  // PirUtil.expand shapes seen so far (api_internal.hpp)
    mutable heamd::LanePool lanes;                 // side_lane.hpp: streams for work of one call that runs beside its neighbour
};

namespace heamd {
ExpandPlanCache& expand_plans(const he_bfv_context* ctx) { return ctx->expand_plans; }
const BfvContext& bfv_impl(const he_bfv_context* ctx) { return *ctx->impl; }
LanePool& lane_pool(const he_bfv_context* ctx) { return ctx->lanes; }
}  // namespace heamd

namespace {

int bfv_create(uint32_t degree, uint64_t t, const uint64_t* q, uint32_t count, bool host_only, he_bfv_context** out,
               int word_bits = 64) {
    if (out == nullptr) return invalid_argument("null out");
    *out = nullptr;
    std::unique_ptr<BfvContext> impl;
    const int status = BfvContext::create(degree, t, q, count, impl, host_only, word_bits);
    if (status != HE_OK) {
        if (status != HE_ERR_DEVICE) heamd::set_last_error(std::string("Context.init: ") + he_status_string(status));
        return status;
    }
    auto* handle = new he_bfv_context{};
    const uint32_t L = impl->top_level();
    handle->ciphertext.resize(L + 1);
    handle->key_switching.resize(L + 1);
    handle->qbsk.resize(L + 1);
    for (uint32_t k = 1; k <= L; ++k) {
        handle->ciphertext[k].reset(new he_poly_context{const_cast<PolyContext*>(impl->ciphertext(k)), false});
        if (impl->key_switching(k) != nullptr)
            handle->key_switching[k].reset(new he_poly_context{const_cast<PolyContext*>(impl->key_switching(k)), false});
        handle->qbsk[k].reset(new he_poly_context{impl->tool(k)->qbsk.get(), false});
    }
    handle->impl = std::move(impl);
    *out = handle;
    return HE_OK;
}

// Common argument checks; returns the level's tool on success.  word_bytes 4: the slabs are packed [UInt32], the same kernels
// run on 4-byte words (widened in registers) and the context must come from he_bfv_context_create_u32.
// `slabs(n)`: the entry's pointer contract (api_internal.hpp check_slabs over its slabs, n the degree).  It is an argument check
// like the two before it, so it comes ahead of the device: an overlap is refused on a host-only context too, and before anything
// is enqueued.  Null slabs and empty batches overlap nothing, so every status the entry had keeps its place.
template <typename SlabCheck>
int check_level(const he_bfv_context* ctx, uint32_t moduli_count, const RnsToolLevel** tool, size_t word_bytes, SlabCheck slabs) {
    if (ctx == nullptr) return invalid_argument("null context");
    if (!ctx->impl->valid(moduli_count)) return invalid_argument("moduli_count out of range");
    HEAMD_TRY_STATUS(slabs(size_t(ctx->impl->degree())));
    if (ctx->impl->host_only()) return heamd::host_only_refusal();
    const int status = ctx->impl->ciphertext(moduli_count)->check_device();
    if (status != HE_OK) return status;
    *tool = ctx->impl->tool(moduli_count);
    if ((*tool)->device.L > heamd::rns_max_supported_moduli()) {
        heamd::set_last_error("more than 16 ciphertext moduli are not supported by the BEHZ kernels");
        return HE_ERR_UNSUPPORTED;
    }
    if (word_bytes == 4 && ctx->impl->word_bits() != 32) return invalid_argument("4-byte slabs need a Bfv<UInt32> context");
    return HE_OK;
}
int check_level(const he_bfv_context* ctx, uint32_t moduli_count, const RnsToolLevel** tool, size_t word_bytes = 8) {
    return check_level(ctx, moduli_count, tool, word_bytes, [](size_t) { return HE_OK; });
}

size_t qbsk_poly_words(const BfvContext& ctx, uint32_t L) { return size_t(2 * L + 1) * ctx.degree(); }

// Resolves caller workspace vs stream-ordered scratch.
int resolve_workspace(void* workspace, size_t workspace_bytes, size_t needed, Scratch& scratch, uint64_t** out) {
    if (workspace != nullptr) {
        if (workspace_bytes < needed) return invalid_argument("workspace too small");
        *out = static_cast<uint64_t*>(workspace);
        return HE_OK;
    }
    HEAMD_HIP_TRY(scratch.allocate(needed));
    *out = static_cast<uint64_t*>(scratch.get());
    return HE_OK;
}

// Eval form over [Q, Bsk] -> Coeff over Q: (x t) -> inverse NTT -> floorQBskToQ  (Bfv+Multiply.swift:31-48)
template <typename W>
int drop_extended_base(const RnsToolLevel& tool, W* eval_qbsk, W* out, size_t polys, hipStream_t stream) {
    DeviceContext scaled = tool.qbsk->device_context();
    scaled.moduli = tool.qbsk_moduli_scaled_by_t;  // folds the multiplication by t into N^-1
    scaled.scaled_inverse_degree = 1;
    const uint32_t rows = tool.qbsk->moduli_count();
    HEAMD_HIP_TRY(ntt_records(true, eval_qbsk, *tool.qbsk, scaled, rows, polys, stream));
    HEAMD_HIP_TRY(heamd::launch_floor_qbsk_to_q(eval_qbsk, out, tool.device, polys, stream));
    return HE_OK;
}

// The five helpers below try a transform with the step before or after it fused into its load or store, and on
// hipErrorNotSupported (nothing launched) run the unfused kernels.  Each takes its image from word_image and hands on the
// status it gave; through the C ABI none but HE_OK is reached there: context creation has validated the moduli, and check_level
// the device and the word size.

// tensor product (Bfv+Multiply.swift:80-82) and dropExtendedBase's inverse NTT: one kernel where the degree has a tiled
// transform (the products are formed as the inverse transform loads its row), else the tensor product alone
template <typename W>
int tensor_and_inverse(const RnsToolLevel& tool, W* lifted, W* tensor, size_t batch, hipStream_t stream, bool* in_coeff_form) {
    DeviceContext scaled = tool.qbsk->device_context();
    scaled.moduli = tool.qbsk_moduli_scaled_by_t;  // folds the multiplication by t into N^-1
    scaled.scaled_inverse_degree = 1;
    const uint32_t rows = tool.qbsk->moduli_count();
    DeviceImage<W> image{};
    HEAMD_TRY_STATUS(heamd::word_image<W>(*tool.qbsk, scaled, rows, image));
    const hipError_t fused = heamd::launch_ntt_tensor_inverse(lifted, tensor, image, rows, batch, stream);
    if (fused == hipErrorNotSupported) {
        (void)hipGetLastError();
        HEAMD_HIP_TRY(heamd::launch_tensor(lifted, tensor, tool.qbsk->device_context(), batch, stream));
        *in_coeff_form = false;
        return HE_OK;
    }
    HEAMD_HIP_TRY(fused);
    *in_coeff_form = true;
    return HE_OK;
}

// computeBehzPolys (Bfv+Multiply.swift:51-57) for `items` pairs of two-polynomial ciphertexts: lift each of the four
// polynomials into lifted[item][0..3] (lhs -> slots 0, 1; rhs -> slots 2, 3), then forward NTT over [Q, Bsk].  Rows
// [0, L) of a lifted polynomial are the input itself (RnsTool.swift:329-330): where the tiled transform can read them
// from the ciphertexts, the lift does not write the copy.
template <typename W>
int lift_pairs_to_eval(const RnsToolLevel& tool, uint32_t L, size_t n, size_t ext, const W* lhs, const W* rhs, W* lifted,
                       size_t items, hipStream_t stream) {
    const DeviceContext qbsk = tool.qbsk->device_context();
    const uint32_t rows = 2 * L + 1;
    DeviceImage<W> image{};
    HEAMD_TRY_STATUS(heamd::word_image<W>(*tool.qbsk, qbsk, rows, image));
    const bool from_source = heamd::ntt_lifted_forward_supported(image, rows, L, items * 4);
    HEAMD_HIP_TRY(heamd::launch_lift_pair_q_to_qbsk_strided(lhs, rhs, lifted, tool.device, items, 2, 2 * L * n, 4 * ext, 0, 2 * ext,
                                                            stream, !from_source));
    if (from_source) HEAMD_HIP_TRY(heamd::launch_ntt_lifted_forward(lifted, image, rows, items * 4, lhs, rhs, 2 * L * n, L, stream));
    else HEAMD_HIP_TRY(ntt_records(false, lifted, *tool.qbsk, qbsk, rows, items * 4, stream));
    return HE_OK;
}

// multiplyWithoutScaling's transforms and tensor product and dropExtendedBase's inverse transforms row by row
// (behz_kernels.hip): the lift writes the Bsk rows of the four operands, then ONE kernel per row band takes every
// (item, [Q, Bsk] row) from its four Coeff rows to its three scaled Coeff product rows -- the Eval rows never reach HBM.
// *fused = false (nothing launched): the degree or the batch has no such kernel; the caller runs the unfused pipeline.
constexpr bool kBehzRowsFused = true;
constexpr bool kBehzCiphertextRowsBesideLift = true;
constexpr size_t kBehzFloorParts = 2;  // <= SideLane::kStages + 1
constexpr size_t kBehzFirstPartEighths = 4;  // two parts: the first one's share of the batch, in eighths
int mul_rows_fused(const he_bfv_context* ctx, const RnsToolLevel& tool, uint32_t L, size_t n, size_t ext, const uint64_t* lhs,
                   const uint64_t* rhs, uint64_t* lifted, uint64_t* tensor, uint64_t* out, size_t batch, hipStream_t stream,
                   bool* fused, bool* floored) {
    *floored = false;
    *fused = false;
    if (!kBehzRowsFused) return HE_OK;
    DeviceContext scaled = tool.qbsk->device_context();
    scaled.moduli = tool.qbsk_moduli_scaled_by_t;  // folds dropExtendedBase's multiplication by t into N^-1
    scaled.scaled_inverse_degree = 1;
    const uint32_t rows = 2 * L + 1;
    if (!heamd::behz_rows_fused_supported(scaled, rows, L, batch)) return HE_OK;
    *fused = true;
    // (the fold butterflies of the Bsk band take the lift's rows as its reduction leaves them, below 5p)
    const bool lazy = heamd::behz_lifted_rows_may_be_lazy(scaled, rows, L);
    // The row bands that read the ciphertexts themselves (the Q rows) do not depend on the lift: on the context's side lane they
    // run beside it -- a 128-register row-fused workgroup leaves room on its CU for the lift's 256-lane workgroups of 40
    // registers (ct x ct +2.6 %, profiles/r05v_behz_q_band_beside_lift_ab.txt).  From four workgroup generations of Q rows up;
    // not while the caller's stream is being captured into a graph, nor when every lane of the context is leased
    // (side_lane.hpp).
    if (kBehzCiphertextRowsBesideLift && batch * L >= 1024) {
        heamd::LaneLease lease(heamd::lane_pool(ctx), stream);
        if (lease.lane != nullptr) {
            SideLane& lane = *lease.lane;
            hipError_t e = hipEventRecord(lane.forked, stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(lane.stream, lane.forked, 0);
            if (e == hipSuccess)
                e = heamd::launch_behz_rows_fused(lhs, rhs, 2 * L * n, lifted, tensor, scaled, rows, L, batch, lane.stream,
                                                  heamd::kBehzCiphertextRows);
            if (e == hipSuccess)
                e = heamd::launch_lift_pair_q_to_qbsk_strided(lhs, rhs, lifted, tool.device, batch, 2, 2 * L * n, 4 * ext, 0, 2 * ext, stream, false, lazy);
            // The Bsk band and the floor in kBehzFloorParts parts of the batch: a part's floor -- 256-lane workgroups of 41
            // registers -- follows the Q band on the lane and runs beside the NEXT part's Bsk band on the caller's stream;
            // only the last part's floor is left to run on its own.
            const size_t parts = (kBehzFloorParts > 1 && batch >= 256 * kBehzFloorParts) ? kBehzFloorParts : 1;
            // (two parts: the first one larger -- its floor has the whole of the second part's Bsk band to run beside, and the
            // second part's floor is what is left exposed)
            size_t bounds[SideLane::kStages + 2] = {0};
            for (size_t k = 1; k <= parts; ++k) bounds[k] = batch * k / parts;
            if (parts == 2) bounds[1] = batch * kBehzFirstPartEighths / 8;
            for (size_t k = 0; k < parts; ++k) {
                const size_t first = bounds[k], items = bounds[k + 1] - first;
                if (items == 0) continue;
                if (e == hipSuccess)
                    e = heamd::launch_behz_rows_fused(lhs + first * 2 * L * n, rhs + first * 2 * L * n, 2 * L * n, lifted + first * 4 * ext,
                                                      tensor + first * 3 * ext, scaled, rows, L, items, stream, heamd::kBehzLiftedRows);
                if (k + 1 < parts) {
                    if (e == hipSuccess) e = hipEventRecord(lane.stage[k], stream);
                    if (e == hipSuccess) e = hipStreamWaitEvent(lane.stream, lane.stage[k], 0);
                    if (e == hipSuccess)
                        e = heamd::launch_floor_qbsk_to_q(tensor + first * 3 * ext, out + first * 3 * L * n, tool.device, items * 3, lane.stream);
                }
            }
            // the join is enqueued whatever happened in between: the caller's stream never runs ahead of the lane's work
            const hipError_t recorded = hipEventRecord(lane.joined, lane.stream);
            const hipError_t waited = recorded == hipSuccess ? hipStreamWaitEvent(stream, lane.joined, 0) : recorded;
            HEAMD_HIP_TRY(e);
            HEAMD_HIP_TRY(waited);
            if (parts > 1) {  // the last part's floor, behind the join (it reads the Q band's rows too)
                const size_t first = bounds[parts - 1];
                HEAMD_HIP_TRY(heamd::launch_floor_qbsk_to_q(tensor + first * 3 * ext, out + first * 3 * L * n, tool.device,
                                                            (batch - first) * 3, stream));
                *floored = true;
            }
            return HE_OK;
        }
    }
    HEAMD_HIP_TRY(heamd::launch_lift_pair_q_to_qbsk_strided(lhs, rhs, lifted, tool.device, batch, 2, 2 * L * n, 4 * ext, 0, 2 * ext, stream, false, lazy));
    HEAMD_HIP_TRY(heamd::launch_behz_rows_fused(lhs, rhs, 2 * L * n, lifted, tensor, scaled, rows, L, batch, stream));
    return HE_OK;
}

// Bfv.mulAssign(ct, ct) (Bfv/Bfv+Multiply.swift:18-85) on slabs of W
template <typename W>
int mul_pipeline(const he_bfv_context* ctx, const RnsToolLevel* tool, uint32_t L, const W* lhs, const W* rhs, W* out,
                 size_t batch, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const size_t n = ctx->impl->degree(), ext = qbsk_poly_words(*ctx->impl, L);
    Scratch scratch(stream);
    uint64_t* raw = nullptr;
    int status = resolve_workspace(workspace, workspace_bytes, batch * 7 * ext * sizeof(W), scratch, &raw);
    if (status != HE_OK) return status;
    W* ws = reinterpret_cast<W*>(raw);
    W* lifted = ws;                   // [batch][4][2L+1][N]  (a0, a1, b0, b1)
    W* tensor = ws + batch * 4 * ext; // [batch][3][2L+1][N]
    if constexpr (std::is_same<W, uint64_t>::value) {
        bool fused = false;
        bool floored = false;
        status = mul_rows_fused(ctx, *tool, L, n, ext, lhs, rhs, lifted, tensor, out, batch, stream, &fused, &floored);
        if (status != HE_OK) return status;
        if (fused) {
            if (!floored) HEAMD_HIP_TRY(heamd::launch_floor_qbsk_to_q(tensor, out, tool->device, batch * 3, stream));
            return HE_OK;
        }
    }
    HEAMD_TRY_STATUS(lift_pairs_to_eval(*tool, L, n, ext, lhs, rhs, lifted, batch, stream));
    bool in_coeff_form = false;
    status = tensor_and_inverse(*tool, lifted, tensor, batch, stream, &in_coeff_form);
    if (status != HE_OK) return status;
    if (!in_coeff_form) return drop_extended_base(*tool, tensor, out, batch * 3, stream);
    HEAMD_HIP_TRY(heamd::launch_floor_qbsk_to_q(tensor, out, tool->device, batch * 3, stream));
    return HE_OK;
}

// Bfv+Keys.swift:165-179: decompose the target over q_0..q_{L-1}, lift each piece to every key-switching modulus
// and take it to Eval.  One fused kernel where the degree has a tiled NTT, two launches otherwise.
template <typename W>
int spread_to_eval(const W* target, size_t target_stride, W* spread, const PolyContext& ks_ctx, uint32_t L, size_t polys,
                   hipStream_t stream) {
    const DeviceContext ks = ks_ctx.device_context();
    DeviceImage<W> image{};
    HEAMD_TRY_STATUS(heamd::word_image<W>(ks_ctx, ks, L + 1, image));
    const hipError_t fused = heamd::launch_ntt_spread(target, target_stride, L, polys, spread, image, 0, stream);
    if (fused != hipErrorNotSupported) {
        HEAMD_HIP_TRY(fused);
        return HE_OK;
    }
    (void)hipGetLastError();
    HEAMD_HIP_TRY(heamd::launch_key_switch_spread(target, target_stride, spread, ks, L, polys, stream));
    HEAMD_HIP_TRY(ntt_rows(false, spread, ks_ctx, ks, L + 1, polys * L * (L + 1), stream));
    return HE_OK;
}
// Bfv+Keys.swift:180-207: the lazy inner product of the decomposed target with the key, then back to Coeff.  One
// kernel where the degree has a tiled NTT (the sums are formed as the inverse transform loads its row).
template <typename W>
int key_mac_to_coeff(const W* spread, const W* key, W* prod, const PolyContext& ks_ctx, uint32_t L, uint32_t top_rows,
                     size_t polys, hipStream_t stream) {
    const DeviceContext ks = ks_ctx.device_context();
    DeviceImage<W> image{};
    HEAMD_TRY_STATUS(heamd::word_image<W>(ks_ctx, ks, L + 1, image));
    const hipError_t fused = heamd::launch_ntt_key_mac_inverse(spread, key, prod, image, L, top_rows, polys, stream);
    if (fused != hipErrorNotSupported) {
        HEAMD_HIP_TRY(fused);
        return HE_OK;
    }
    (void)hipGetLastError();
    HEAMD_HIP_TRY(heamd::launch_key_switch_mac(spread, key, prod, ks, L, top_rows, polys, stream));
    HEAMD_HIP_TRY(ntt_rows(true, prod, ks_ctx, ks, L + 1, polys * 2 * (L + 1), stream));
    return HE_OK;
}

// The inner product with the key, the inverse transforms and the key switch's last step (`end`: relinearize, added_polys = 2)
// in two launches of one kernel where the degree and the batch have it (ntt_sources.hpp kInverseFromKeyMacFinish,
// ntt_word32.hip kSource32KeyMacFinish); *finished = false otherwise (nothing launched).
template <typename W>
int key_mac_and_finish(const W* spread, const W* key, W* prod, const heamd::KeySwitchEnd<W>& end, const PolyContext& ks_ctx,
                       uint32_t L, uint32_t top_rows, size_t polys, hipStream_t stream, bool* finished) {
    DeviceImage<W> image{};
    HEAMD_TRY_STATUS(heamd::word_image<W>(ks_ctx, ks_ctx.device_context(), L + 1, image));
    const hipError_t fused = heamd::launch_ntt_key_mac_inverse_finish(spread, key, prod, end, image, L, top_rows, polys, stream);
    *finished = fused != hipErrorNotSupported;
    if (*finished) HEAMD_HIP_TRY(fused);
    return HE_OK;
}

// _computeKeySwitchingUpdate (Bfv+Keys.swift:123-208) on polynomial `target` of every item, then
// out[item][c] = (c < added_polys ? ct[item][c] : 0) + update[item][c]  (relinearize: added 2; applyGalois: added 1)
// One key per group of `group_size` consecutive items (ciphertexts of different clients in one batch): one decomposition
// over the whole batch, then the inner product with the key per run of equal keys -- through the key switch's last step where
// the run has that kernel, otherwise to Coeff, and the last step follows in one launch over every stretch of such runs.
template <typename W>
int key_switch_pipeline_grouped(const he_bfv_context* ctx, uint32_t L, const W* target, size_t target_stride,
                                const W* ct_base, size_t ct_stride, const W* const* keys, size_t groups, size_t group_size,
                                W* out, uint32_t added_polys, W* spread, W* prod, hipStream_t stream) {
    const PolyContext* ks_ctx = ctx->impl->key_switching(L);
    const size_t n = ctx->impl->degree(), batch = groups * group_size;
    const uint32_t top_rows = ctx->impl->top_level() + 1;
    HEAMD_TRY_STATUS(spread_to_eval(target, target_stride, spread, *ks_ctx, L, batch, stream));
    auto finish = [&](size_t first, size_t end) {  // the last step for the items [first, end) left in Coeff form
        if (first == end) return hipSuccess;
        return heamd::launch_key_switch_finish(static_cast<const W*>(prod) + first * 2 * (L + 1) * n,
                                               ct_base + first * ct_stride, ct_stride, out + first * 2 * L * n,
                                               ks_ctx->device_context(), L, end - first, added_polys, stream);
    };
    size_t unfinished = 0;  // the first item whose last step is still to come
    for (size_t g = 0; g < groups;) {
        size_t run = 1;
        while (g + run < groups && keys[g + run] == keys[g]) ++run;
        const size_t first = g * group_size, polys = run * group_size;
        const W* run_spread = static_cast<const W*>(spread) + first * L * (L + 1) * n;
        W* run_prod = prod + first * 2 * (L + 1) * n;
        const heamd::KeySwitchEnd<W> end{ct_base + first * ct_stride, ct_stride, out + first * 2 * L * n, added_polys};
        bool finished = false;
        HEAMD_TRY_STATUS(key_mac_and_finish(run_spread, keys[g], run_prod, end, *ks_ctx, L, top_rows, polys, stream, &finished));
        if (!finished) {
            HEAMD_TRY_STATUS(key_mac_to_coeff(run_spread, keys[g], run_prod, *ks_ctx, L, top_rows, polys, stream));
        } else {
            HEAMD_HIP_TRY(finish(unfinished, first));
            unfinished = first + polys;
        }
        g += run;
    }
    HEAMD_HIP_TRY(finish(unfinished, batch));
    return HE_OK;
}

// g^-1 mod 2N for odd g (Newton iteration doubles the correct low bits)
uint32_t inverse_mod_power_of_two(uint64_t g, uint64_t modulus) {
    uint64_t x = g;  // correct to 3 bits
    for (int k = 0; k < 6; ++k) x *= 2 - g * x;
    return static_cast<uint32_t>(x & (modulus - 1));
}

// Bfv.applyGalois (Bfv.swift:174-198) without a rotated copy of the ciphertext: the automorphism of c1 happens as the
// decomposition's transform loads its rows, that of c0 as the last kernel adds it to the update; expand_shift != 0
// turns that last kernel into one step of PirUtil.expand (rns_kernels.hpp, launch_galois_finish).  One key per group of
// `group_size` consecutive ciphertexts.  *fused = false (nothing launched): the degree has no tiled transform.
// `own` (expand steps): the ciphertexts the children are formed with when they are not `ct` (launch_galois_finish).
int galois_switch_fused(const he_bfv_context* ctx, uint32_t L, const uint64_t* ct, uint32_t galois_inverse,
                        const uint64_t* const* keys, size_t groups, size_t group_size, uint64_t* out, uint32_t expand_shift,
                        const heamd::ExpandTargets& targets, uint64_t* spread, uint64_t* prod, hipStream_t stream, bool* fused,
                        const uint64_t* own = nullptr) {
    *fused = false;
    const PolyContext* ks_ctx = ctx->impl->key_switching(L);
    const DeviceContext ks = ks_ctx->device_context();
    const size_t n = ctx->impl->degree(), batch = groups * group_size, ct_stride = 2 * size_t(L) * n;
    const hipError_t spread_status = heamd::launch_ntt_spread(ct + size_t(L) * n, ct_stride, L, batch, spread, ks, galois_inverse, stream);
    if (spread_status == hipErrorNotSupported) {
        (void)hipGetLastError();
        return HE_OK;
    }
    HEAMD_HIP_TRY(spread_status);
    *fused = true;
    // the key switch's end (galois(c0) + update0 | update1, or the two children of an expand step) in the key-MAC
    // transform's store where the degree has that kernel; the separate finish kernel otherwise
    // -- decided on the smallest run of queries with one key: every run is two launches of its own there, against one
    // key-MAC launch per run and ONE finish kernel over the whole batch (profiles/r04m_galois_fused_end_ab.txt)
    size_t smallest_run = groups;
    for (size_t g = 0; g < groups;) {
        size_t run = 1;
        while (g + run < groups && keys[g + run] == keys[g]) ++run;
        smallest_run = run < smallest_run ? run : smallest_run;
        g += run;
    }
    const bool fused_end = heamd::ntt_key_mac_finish_supported(ks, L, smallest_run * group_size);
    for (size_t g = 0; g < groups;) {
        size_t run = 1;
        while (g + run < groups && keys[g + run] == keys[g]) ++run;
        const size_t first = g * group_size, polys = run * group_size;
        const uint64_t* const run_spread = static_cast<const uint64_t*>(spread) + first * L * (L + 1) * n;
        uint64_t* const run_prod = prod + first * 2 * (L + 1) * n;
        if (fused_end) {
            heamd::KeySwitchEnd<uint64_t> end{ct, ct_stride, out, 1u};
            end.galois_inverse = galois_inverse;
            end.expand_shift = expand_shift;
            end.own_base = own;
            end.targets_table = targets.table;
            end.targets_group_size = targets.group_size;
            end.targets_group_stride = targets.group_stride;
            end.poly_base = first;
            HEAMD_HIP_TRY(heamd::launch_ntt_key_mac_inverse_finish(run_spread, keys[g], run_prod, end, ks, L,
                                                                   ctx->impl->top_level() + 1, polys, stream));
        } else {
            HEAMD_TRY_STATUS(key_mac_to_coeff(run_spread, keys[g], run_prod, *ks_ctx, L, ctx->impl->top_level() + 1, polys, stream));
        }
        g += run;
    }
    if (fused_end) return HE_OK;
    HEAMD_HIP_TRY(heamd::launch_galois_finish(static_cast<const uint64_t*>(prod), ct, ct_stride, out, ks, L, batch, galois_inverse,
                                              expand_shift, targets, stream, own));
    return HE_OK;
}

template <typename W>
int relinearize_pipeline(const he_bfv_context* ctx, uint32_t L, const W* ct3, const W* key, W* out, size_t batch,
                         void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const size_t n = ctx->impl->degree();
    Scratch scratch(stream);
    uint64_t* raw = nullptr;
    const size_t words = batch * (size_t(L) * (L + 1) + 2 * (L + 1)) * n;
    int status = resolve_workspace(workspace, workspace_bytes, words * sizeof(W), scratch, &raw);
    if (status != HE_OK) return status;
    W* spread = reinterpret_cast<W*>(raw);                // [batch][L][L+1][N]
    W* prod = spread + batch * L * (L + 1) * n;           // [batch][2][L+1][N]
    const size_t ct_stride = 3 * size_t(L) * n;
    return key_switch_pipeline_grouped(ctx, L, ct3 + 2 * size_t(L) * n, ct_stride, ct3, ct_stride, &key, 1, batch, out, 2,
                                       spread, prod, stream);
}

}  // namespace

namespace heamd {
// One level of PirUtil.expand (PirUtil.swift:204-236) for parents whose Galois element has its own key: the children
// (parent + applyGalois(parent), (parent - applyGalois(parent)) x^shift) leave the key switch's last kernel directly.
// leaf_table != nullptr: the children are leaves and go to their output slots in `next` = the expansion's output
// (rns_kernels.hpp, ExpandTargets; leaf_stride = outputs per query).
// Returns kExpandStepUnavailable when the degree has no tiled transform (the caller composes the step from
// he_bfv_apply_galois_grouped_device and the expand-step kernel instead).
int bfv_expand_step_fused(const he_bfv_context* ctx, uint32_t L, const uint64_t* parents, uint64_t element,
                          const uint64_t* const* keys, size_t groups, size_t group_size, uint64_t* next, uint32_t shift,
                          const uint32_t* leaf_table, size_t leaf_stride, void* workspace, size_t workspace_bytes,
                          hipStream_t stream, const uint64_t* rotated) {
    const size_t n = ctx->impl->degree(), batch = groups * group_size;
    if (batch == 0) return HE_OK;
    if (workspace_bytes < he_bfv_apply_galois_workspace_bytes(ctx, L, batch)) return invalid_argument("workspace too small");
    uint64_t* spread = static_cast<uint64_t*>(workspace);    // [batch][L][L+1][N]
    uint64_t* prod = spread + batch * L * (L + 1) * n;       // [batch][2][L+1][N]
    bool fused = false;
    HEAMD_TRY_STATUS(galois_switch_fused(ctx, L, rotated != nullptr ? rotated : parents, inverse_mod_power_of_two(element, 2 * n),
                                         keys, groups, group_size, next, shift,
                                         heamd::ExpandTargets{leaf_table, group_size, leaf_stride}, spread, prod, stream, &fused,
                                         rotated != nullptr ? parents : nullptr));
    return fused ? HE_OK : kExpandStepUnavailable;
}
}  // namespace heamd

extern "C" {

int he_bfv_context_create(uint32_t degree, uint64_t plaintext_modulus, const uint64_t* coefficient_moduli,
                          uint32_t moduli_count, he_bfv_context** out) {
    return bfv_create(degree, plaintext_modulus, coefficient_moduli, moduli_count, false, out);
}
int he_bfv_context_create_host_only(uint32_t degree, uint64_t plaintext_modulus, const uint64_t* coefficient_moduli,
                                    uint32_t moduli_count, he_bfv_context** out) {
    return bfv_create(degree, plaintext_modulus, coefficient_moduli, moduli_count, true, out);
}
int he_bfv_context_create_u32(uint32_t degree, uint64_t plaintext_modulus, const uint64_t* coefficient_moduli,
                              uint32_t moduli_count, he_bfv_context** out) {
    return bfv_create(degree, plaintext_modulus, coefficient_moduli, moduli_count, false, out, 32);
}
int he_bfv_context_create_u32_host_only(uint32_t degree, uint64_t plaintext_modulus, const uint64_t* coefficient_moduli,
                                        uint32_t moduli_count, he_bfv_context** out) {
    return bfv_create(degree, plaintext_modulus, coefficient_moduli, moduli_count, true, out, 32);
}
void he_bfv_context_destroy(he_bfv_context* ctx) {
    heamd::RelaxedCapture relaxed;  // (api_internal.hpp: safe beside another thread's -- or this thread's -- graph capture)
    delete ctx;
}
uint32_t he_bfv_ciphertext_moduli_count(const he_bfv_context* ctx) { return ctx ? ctx->impl->top_level() : 0; }
const he_poly_context* he_bfv_ciphertext_context(const he_bfv_context* ctx, uint32_t k) {
    return (ctx && ctx->impl->valid(k)) ? ctx->ciphertext[k].get() : nullptr;
}
const he_poly_context* he_bfv_key_switching_context(const he_bfv_context* ctx, uint32_t k) {
    return (ctx && ctx->impl->valid(k)) ? ctx->key_switching[k].get() : nullptr;
}
const he_poly_context* he_bfv_qbsk_context(const he_bfv_context* ctx, uint32_t k) {
    return (ctx && ctx->impl->valid(k)) ? ctx->qbsk[k].get() : nullptr;
}
int he_bfv_copy_bsk_moduli(const he_bfv_context* ctx, uint64_t* out_bsk) {
    if (ctx == nullptr || out_bsk == nullptr) return invalid_argument("null pointer");
    const auto& list = ctx->impl->bsk_mtilde();
    for (size_t i = 0; i + 1 < list.size(); ++i) out_bsk[i] = list[i];
    return HE_OK;
}

extern "C++" {
namespace {
// RnsTool.liftQToQBsk (`lift`) / floorQBskToQ on whole polynomials
template <typename W>
int rns_base_change(const he_bfv_context* ctx, uint32_t moduli_count, bool lift, const W* in, W* out, size_t batch, he_stream s) {
    const RnsToolLevel* tool = nullptr;
    // a polynomial's L rows and its 2L + 1 rows lie at different strides: in place, polynomials store over one another's input
    int status = check_level(ctx, moduli_count, &tool, sizeof(W), [&](size_t n) {
        const size_t q_bytes = batch * moduli_count * n * sizeof(W), qbsk_bytes = batch * (2 * moduli_count + 1) * n * sizeof(W);
        return heamd::check_slabs(lift ? "liftQToQBsk" : "floorQBskToQ", {{"out", out, lift ? qbsk_bytes : q_bytes, true},
                                                                         {"in", in, lift ? q_bytes : qbsk_bytes, false}});
    });
    if (status != HE_OK) return status;
    if (batch == 0) return HE_OK;
    if (in == nullptr || out == nullptr) return invalid_argument("null slab");
    if (lift) HEAMD_HIP_TRY(heamd::launch_lift_q_to_qbsk(in, out, tool->device, batch, as_stream(s)));
    else HEAMD_HIP_TRY(heamd::launch_floor_qbsk_to_q(in, out, tool->device, batch, as_stream(s)));
    return HE_OK;
}
}  // namespace
}  // extern "C++"

int he_rns_lift_q_to_qbsk_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* in, uint64_t* out,
                                 size_t batch, he_stream s) {
    return rns_base_change(ctx, moduli_count, true, in, out, batch, s);
}
int he_rns_lift_q_to_qbsk_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* in, uint32_t* out,
                                     size_t batch, he_stream s) {
    return rns_base_change(ctx, moduli_count, true, in, out, batch, s);
}
int he_rns_floor_qbsk_to_q_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* in, uint64_t* out,
                                  size_t batch, he_stream s) {
    return rns_base_change(ctx, moduli_count, false, in, out, batch, s);
}
int he_rns_floor_qbsk_to_q_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* in,
                                      uint32_t* out, size_t batch, he_stream s) {
    return rns_base_change(ctx, moduli_count, false, in, out, batch, s);
}

// ------------------------------------------------------------------------------------------ ct x ct
size_t he_bfv_mul_workspace_bytes(const he_bfv_context* ctx, uint32_t moduli_count, size_t batch) {
    if (ctx == nullptr || !ctx->impl->valid(moduli_count)) return 0;
    return batch * 7 * qbsk_poly_words(*ctx->impl, moduli_count) * sizeof(uint64_t);  // 4 lifted + 3 tensor polys
}

extern "C++" {
namespace {
template <typename W>
int mul_entry(const he_bfv_context* ctx, uint32_t moduli_count, const W* lhs, const W* rhs, W* out, size_t batch,
              void* workspace, size_t workspace_bytes, he_stream s) {
    const RnsToolLevel* tool = nullptr;
    // out must not overlap lhs or rhs: with the batch in parts, one part's floor stores its products while another
    // part's row band still reads the operands -- whether that happens depends on the batch size and the moduli, so an
    // overlap would be right for some shapes and silently wrong for others.  lhs and rhs are only read: they may be one
    // ciphertext (a square).
    int status = check_level(ctx, moduli_count, &tool, sizeof(W), [&](size_t n) {
        const size_t poly_bytes = batch * moduli_count * n * sizeof(W);
        return heamd::check_slabs("ct x ct", {{"out", out, 3 * poly_bytes, true},
                                              {"workspace", workspace, workspace_bytes, true},
                                              {"lhs", lhs, 2 * poly_bytes, false},
                                              {"rhs", rhs, 2 * poly_bytes, false}});
    });
    if (status != HE_OK) return status;
    if (batch == 0) return HE_OK;
    if (lhs == nullptr || rhs == nullptr || out == nullptr) return invalid_argument("null ciphertext");
    return mul_pipeline(ctx, tool, moduli_count, lhs, rhs, out, batch, workspace, workspace_bytes, as_stream(s));
}
}  // namespace
}  // extern "C++"

int he_bfv_mul_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* lhs, const uint64_t* rhs,
                      uint64_t* out, size_t batch, void* workspace, size_t workspace_bytes, he_stream s) {
    return mul_entry(ctx, moduli_count, lhs, rhs, out, batch, workspace, workspace_bytes, s);
}
int he_bfv_mul_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* lhs, const uint32_t* rhs,
                          uint32_t* out, size_t batch, void* workspace, size_t workspace_bytes, he_stream s) {
    return mul_entry(ctx, moduli_count, lhs, rhs, out, batch, workspace, workspace_bytes, s);
}

// ------------------------------------------------------------------------------------------ relinearize
size_t he_bfv_relinearize_workspace_bytes(const he_bfv_context* ctx, uint32_t moduli_count, size_t batch) {
    if (ctx == nullptr || !ctx->impl->valid(moduli_count)) return 0;
    const size_t L = moduli_count, n = ctx->impl->degree();
    return batch * (L * (L + 1) + 2 * (L + 1)) * n * sizeof(uint64_t);
}

extern "C++" {
template <typename W>
int heamd::bfv_relinearize(const he_bfv_context* ctx, uint32_t moduli_count, const W* ct3, const W* key, W* out, size_t batch,
                           void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const RnsToolLevel* tool = nullptr;
    // out must not overlap ct3: the last kernel adds the update to (c0, c1) of one item while it stores another item's
    // result (items are 3 L N words apart in ct3 and 2 L N apart in out), in no particular order -- and which kernel
    // that is depends on the batch size, so an overlap would be right for some batches and silently wrong for others.
    // The one overlap that is word-for-word in place -- a single ciphertext relinearized onto its own (c0, c1) -- is
    // allowed: it takes the element-wise finish kernel (a batch of one is never fused).
    int status = check_level(ctx, moduli_count, &tool, sizeof(W), [&](size_t n) {
        const size_t poly_bytes = batch * moduli_count * n * sizeof(W), top = ctx->impl->top_level();
        if (batch == 0) return int(HE_OK);  // (nothing is read or written, the key and the workspace included)
        return heamd::check_slabs("relinearize", {{"out", out, 2 * poly_bytes, true},
                                                  {"ct3", ct3, 3 * poly_bytes, false},
                                                  {"workspace", workspace, workspace_bytes, true},
                                                  {"key", key, top * 2 * (top + 1) * n * sizeof(W), false}},
                                  batch == 1 ? std::pair<int, int>{0, 1} : std::pair<int, int>{-1, -1});
    });
    if (status != HE_OK) return status;
    if (key == nullptr || !ctx->impl->has_key_switching()) {
        heamd::set_last_error("no relinearization key");
        return HE_ERR_MISSING_RELINEARIZATION_KEY;  // Bfv.swift:208-210
    }
    if (batch == 0) return HE_OK;
    if (ct3 == nullptr || out == nullptr) return invalid_argument("null ciphertext");
    return relinearize_pipeline(ctx, moduli_count, ct3, key, out, batch, workspace, workspace_bytes, stream);
}
template int heamd::bfv_relinearize(const he_bfv_context*, uint32_t, const uint64_t*, const uint64_t*, uint64_t*, size_t, void*,
                                    size_t, hipStream_t);
template int heamd::bfv_relinearize(const he_bfv_context*, uint32_t, const uint32_t*, const uint32_t*, uint32_t*, size_t, void*,
                                    size_t, hipStream_t);
}  // extern "C++"

int he_bfv_relinearize_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* ct3,
                              const uint64_t* key, uint64_t* out, size_t batch, void* workspace,
                              size_t workspace_bytes, he_stream s) {
    return heamd::bfv_relinearize(ctx, moduli_count, ct3, key, out, batch, workspace, workspace_bytes, as_stream(s));
}
int he_bfv_relinearize_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* ct3,
                                  const uint32_t* key, uint32_t* out, size_t batch, void* workspace,
                                  size_t workspace_bytes, he_stream s) {
    return heamd::bfv_relinearize(ctx, moduli_count, ct3, key, out, batch, workspace, workspace_bytes, as_stream(s));
}

// ------------------------------------------------------------------------------------------ Galois automorphism
extern "C++" {
namespace {
bool is_valid_galois_element(uint64_t element, uint64_t degree) {  // Galois.swift:100-105
    return degree != 0 && (degree & (degree - 1)) == 0 && (element & 1) == 1 && element < (degree << 1) && element > 1;
}
}  // namespace
}  // extern "C++"

// GaloisElement.swappingRows(degree:) / rotatingColumns(by:degree:) (PolyRq/Galois.swift:174-212): the elements that
// Bfv.swapRows / rotateColumns pass to applyGalois (HeScheme.swift:1047-1094)
int he_galois_element_swapping_rows(uint64_t degree, uint64_t* out_element) {
    if (out_element == nullptr) return invalid_argument("null out");
    *out_element = (degree << 1) - 1;
    return HE_OK;
}
int he_galois_element_rotating_columns(int64_t step, uint64_t degree, uint64_t* out_element) {
    if (out_element == nullptr) return invalid_argument("null out");
    if (degree == 0 || (degree & (degree - 1)) != 0) return HE_ERR_INVALID_DEGREE;
    uint64_t positive = static_cast<uint64_t>(step < 0 ? -step : step);
    if (!(positive < (degree >> 1) && positive > 0)) return invalid_argument("rotation step out of range");  // invalidRotationStep
    positive &= (degree << 1) - 1;
    if (step > 0) positive = (degree >> 1) - positive;
    // GaloisElementGenerator.value = 3, to the power `positive` mod 2N
    const uint64_t modulus = degree << 1;
    uint64_t result = 1, base = 3 % modulus;
    for (uint64_t e = positive; e != 0; e >>= 1) {
        if (e & 1) result = result * base % modulus;
        base = base * base % modulus;
    }
    *out_element = result;
    return HE_OK;
}

size_t he_bfv_apply_galois_workspace_bytes(const he_bfv_context* ctx, uint32_t moduli_count, size_t batch) {
    if (ctx == nullptr || !ctx->impl->valid(moduli_count)) return 0;
    const size_t L = moduli_count, n = ctx->impl->degree();
    return batch * (2 * L + L * (L + 1) + 2 * (L + 1)) * n * sizeof(uint64_t);
}

extern "C++" {
namespace heamd {
// Bfv.applyGalois (Bfv.swift:174-198) on groups * group_size ciphertexts, group g under keys[g]: the checks of the three
// entries below in their order, the fused key switch where the words and the degree have it, else the rotated copy and
// key_switch_pipeline_grouped.
template <typename W>
int bfv_apply_galois_grouped(const he_bfv_context* ctx, uint32_t L, const W* ct, uint64_t element, const W* const* keys,
                             size_t groups, size_t group_size, W* out, void* workspace, size_t workspace_bytes,
                             hipStream_t stream) {
    const RnsToolLevel* tool = nullptr;
    // out may be ct itself: the whole of ct goes through the permutation into the workspace before the first word of out is
    // stored (the fused kernels, which read ct to the end, are not taken then).  Any other overlap is refused.
    int status = check_level(ctx, L, &tool, sizeof(W), [&](size_t n) {
        const size_t ct_bytes = groups * group_size * 2 * L * n * sizeof(W), top = ctx->impl->top_level();
        if (ct_bytes == 0) return int(HE_OK);  // (nothing is read or written, the keys and the workspace included)
        HEAMD_TRY_STATUS(heamd::check_slabs("applyGalois", {{"out", out, ct_bytes, true},
                                                            {"ct", ct, ct_bytes, false},
                                                            {"workspace", workspace, workspace_bytes, true}},
                                            {0, 1}));
        for (size_t g = 0; keys != nullptr && g < groups; ++g)
            HEAMD_TRY_STATUS(heamd::check_slabs("applyGalois", {{"out", out, ct_bytes, true},
                                                                {"workspace", workspace, workspace_bytes, true},
                                                                {"galois_key", keys[g], top * 2 * (top + 1) * n * sizeof(W), false}}));
        return int(HE_OK);
    });
    if (status != HE_OK) return status;
    bool missing = keys == nullptr || !ctx->impl->has_key_switching();
    for (size_t g = 0; !missing && g < groups; ++g) missing = keys[g] == nullptr;
    if (missing) {
        heamd::set_last_error("no Galois key for this element");
        return HE_ERR_MISSING_GALOIS_KEY;  // Bfv.swift:184-189
    }
    if (!is_valid_galois_element(element, ctx->impl->degree())) return invalid_argument("invalid Galois element");
    const size_t batch = groups * group_size;
    if (batch == 0) return HE_OK;
    if (ct == nullptr || out == nullptr) return invalid_argument("null ciphertext");
    const size_t n = ctx->impl->degree();
    Scratch scratch(stream);
    uint64_t* raw = nullptr;
    const size_t words = batch * (2 * size_t(L) + size_t(L) * (L + 1) + 2 * (L + 1)) * n;
    status = resolve_workspace(workspace, workspace_bytes, words * sizeof(W), scratch, &raw);
    if (status != HE_OK) return status;
    W* rotated = reinterpret_cast<W*>(raw);                // [batch][2][L][N]
    W* spread = rotated + batch * 2 * L * n;               // [batch][L][L+1][N]
    W* prod = spread + batch * L * (L + 1) * n;            // [batch][2][L+1][N]
    const size_t ct_stride = 2 * size_t(L) * n;
    // Bfv.swift:190-196: c0' = galois(c0) + update0, c1' = update1, update = keySwitch(galois(c1))
    const uint32_t galois_inverse = inverse_mod_power_of_two(element, 2 * n);
    if constexpr (sizeof(W) == 8) {
        if (ct != out) {  // the fused kernels read ct to the end
            bool fused = false;
            HEAMD_TRY_STATUS(galois_switch_fused(ctx, L, ct, galois_inverse, keys, groups, group_size, out, 0,
                                                 heamd::ExpandTargets{nullptr, 1, 0}, spread, prod, stream, &fused));
            if (fused) return HE_OK;
        }
    }
    const PolyContext* q_ctx = ctx->impl->ciphertext(L);
    HEAMD_HIP_TRY(heamd::launch_galois_coeff(ct, rotated, q_ctx->device_context(L), galois_inverse, batch * 2 * L, stream));
    return key_switch_pipeline_grouped<W>(ctx, L, rotated + size_t(L) * n, ct_stride, rotated, ct_stride, keys, groups,
                                          group_size, out, 1, spread, prod, stream);
}
template int bfv_apply_galois_grouped(const he_bfv_context*, uint32_t, const uint64_t*, uint64_t, const uint64_t* const*, size_t,
                                      size_t, uint64_t*, void*, size_t, hipStream_t);
template int bfv_apply_galois_grouped(const he_bfv_context*, uint32_t, const uint32_t*, uint64_t, const uint32_t* const*, size_t,
                                      size_t, uint32_t*, void*, size_t, hipStream_t);
}  // namespace heamd
}  // extern "C++"

int he_bfv_apply_galois_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* ct, uint64_t element,
                               const uint64_t* galois_key, uint64_t* out, size_t batch, void* workspace,
                               size_t workspace_bytes, he_stream s) {
    return heamd::bfv_apply_galois_grouped(ctx, moduli_count, ct, element, &galois_key, 1, batch, out, workspace,
                                           workspace_bytes, as_stream(s));
}
int he_bfv_apply_galois_grouped_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* ct,
                                       uint64_t element, const uint64_t* const* galois_keys, size_t groups,
                                       size_t group_size, uint64_t* out, void* workspace, size_t workspace_bytes,
                                       he_stream s) {
    return heamd::bfv_apply_galois_grouped(ctx, moduli_count, ct, element, galois_keys, groups, group_size, out, workspace,
                                           workspace_bytes, as_stream(s));
}
int he_bfv_apply_galois_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* ct, uint64_t element,
                                   const uint32_t* galois_key, uint32_t* out, size_t batch, void* workspace,
                                   size_t workspace_bytes, he_stream s) {
    return heamd::bfv_apply_galois_grouped(ctx, moduli_count, ct, element, &galois_key, 1, batch, out, workspace,
                                           workspace_bytes, as_stream(s));
}

// ------------------------------------------------------------------------------------------ scaleAndRound
extern "C++" {
namespace {
template <typename W>
int scale_and_round(const he_bfv_context* ctx, uint32_t moduli_count, const W* in, uint64_t scaling_factor, W* out, size_t batch,
                    he_stream s) {
    const RnsToolLevel* tool = nullptr;
    int status = check_level(ctx, moduli_count, &tool, sizeof(W), [&](size_t n) {  // L rows in, one row out per polynomial
        return heamd::check_slabs("scaleAndRound", {{"out", out, batch * n * sizeof(W), true},
                                                    {"in", in, batch * moduli_count * n * sizeof(W), false}});
    });
    if (status != HE_OK) return status;
    if (batch == 0) return HE_OK;
    if (in == nullptr || out == nullptr) return invalid_argument("null polynomial");
    const uint64_t t = ctx->impl->plaintext_modulus();
    if (scaling_factor >= t) return invalid_argument("scaling factor not reduced mod t");
    // inverseGammaModT.multiplyMod(scalingFactor) (RnsTool.swift:298)
    const uint64_t scaled = heamd::mul_mod(tool->device.inv_gamma_mod_t, scaling_factor, t);
    const heamd::U64x2 final_scale{scaled, heamd::shoup_factor(scaled, t)};
    HEAMD_HIP_TRY(heamd::launch_scale_and_round(in, out, tool->device, final_scale, batch, as_stream(s)));
    return HE_OK;
}
}  // namespace
}  // extern "C++"

int he_rns_scale_and_round_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* in,
                                  uint64_t scaling_factor, uint64_t* out, size_t batch, he_stream s) {
    return scale_and_round(ctx, moduli_count, in, scaling_factor, out, batch, s);
}
int he_rns_scale_and_round_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* in,
                                      uint64_t scaling_factor, uint32_t* out, size_t batch, he_stream s) {
    return scale_and_round(ctx, moduli_count, in, scaling_factor, out, batch, s);
}

// ------------------------------------------------------------------------------------------ decrypt, noise budget
extern "C++" {
namespace {

using heamd::NoiseNormTables;
using heamd::u64;

// the checks the entries with void* slabs share, in this order: the word, the level (check_level), the polynomial count
// `result`: the slab the entry writes, its size as bytes per coefficient (the degree is the context's, which may still be null
// here) plus result_fixed_bytes; it, the ciphertexts, the secret key and a caller's workspace go through check_slabs
int check_decrypt_arguments(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, uint32_t poly_count,
                            const RnsToolLevel** tool, const char* what, const void* cts, const void* secret_key, size_t batch,
                            heamd::Slab result, size_t result_fixed_bytes, const void* workspace, size_t workspace_bytes) {
    HEAMD_TRY_STATUS(heamd::check_word_bits(word_bits));
    HEAMD_TRY_STATUS(check_level(ctx, moduli_count, tool, word_bits / 8, [&](size_t n) {
        const size_t poly_bytes = size_t(moduli_count) * n * (word_bits / 8);
        if (batch == 0) return int(HE_OK);  // (nothing is read or written, the secret key and the workspace included)
        // (a polynomial count the entry is about to refuse says nothing about where the ciphertexts end)
        if (poly_count < 1 || poly_count > heamd::kMaxDecryptPolys) return int(HE_OK);
        result.bytes *= n;  // (given per coefficient)
        result.bytes += result_fixed_bytes;
        return heamd::check_slabs(what, {result,
                                         {"workspace", workspace, workspace_bytes, true},
                                         {"cts", cts, batch * poly_count * poly_bytes, false},
                                         {"secret_key", secret_key, poly_bytes, false}});
    }));
    if (poly_count < 1 || poly_count > heamd::kMaxDecryptPolys) {
        heamd::set_last_error("a ciphertext has 1..3 polynomials");
        return HE_ERR_UNSUPPORTED;
    }
    return HE_OK;
}

// Of Coeff-form ciphertexts the polynomials behind the first are transformed in a copy (the caller's slab is const); c0 is
// added in Coeff form after the inverse transform -- the transform is linear -- and is neither copied nor transformed
size_t decrypt_copy_words(const BfvContext& bfv, uint32_t moduli_count, uint32_t poly_count, bool is_eval, size_t batch) {
    return is_eval || poly_count == 1 ? 0 : batch * (poly_count - 1) * moduli_count * bfv.degree();
}
size_t decrypt_dot_words(const BfvContext& bfv, uint32_t moduli_count, size_t batch) {
    return batch * moduli_count * bfv.degree();
}

// Bfv.dotProduct (Bfv+Decrypt.swift:188-204): out [batch][L][N] Coeff.  eval_copy: decrypt_copy_words words.
template <typename W>
int secret_dot_product(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, bool is_eval, const W* cts,
                       const W* secret_key, W* out, size_t batch, W* eval_copy, hipStream_t stream) {
    const PolyContext* pc = ctx->impl->ciphertext(moduli_count);
    const DeviceContext dc = pc->device_context();
    const size_t poly_words = size_t(moduli_count) * ctx->impl->degree();
    if (!is_eval && poly_count == 1) {  // the dot product is c0: its two transforms cancel
        HEAMD_HIP_TRY(hipMemcpyAsync(out, cts, batch * poly_words * sizeof(W), hipMemcpyDeviceToDevice, stream));
        return HE_OK;
    }
    if (is_eval) {
        HEAMD_HIP_TRY(heamd::launch_secret_dot_product(cts, secret_key, out, dc, poly_count, true, batch, stream));
        HEAMD_HIP_TRY(ntt_rows(true, out, *pc, dc, moduli_count, batch * moduli_count, stream));
        return HE_OK;
    }
    const size_t tail_bytes = (poly_count - 1) * poly_words * sizeof(W);  // c1.. of one ciphertext
    HEAMD_HIP_TRY(hipMemcpy2DAsync(eval_copy, tail_bytes, cts + poly_words, poly_count * poly_words * sizeof(W), tail_bytes, batch,
                                   hipMemcpyDeviceToDevice, stream));
    HEAMD_HIP_TRY(ntt_rows(false, eval_copy, *pc, dc, moduli_count, batch * (poly_count - 1) * moduli_count, stream));
    HEAMD_HIP_TRY(heamd::launch_secret_dot_product(eval_copy, secret_key, out, dc, poly_count, false, batch, stream));
    HEAMD_HIP_TRY(ntt_rows(true, out, *pc, dc, moduli_count, batch * moduli_count, stream));
    HEAMD_HIP_TRY(heamd::launch_add_first_polynomial(cts, out, dc, poly_count, batch, stream));
    return HE_OK;
}

// The dot product of a batch into `dot` (the caller's slab, or the head of the workspace when dot == nullptr), with the checks
// every entry below makes.  HE_OK with *dot_out == nullptr: nothing to do (batch 0).
template <typename W>
int decrypt_dot(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, int is_eval, const void* cts,
                const void* secret_key, void* dot, size_t batch, void* workspace, size_t workspace_bytes, Scratch& scratch,
                hipStream_t stream, W** dot_out) {
    *dot_out = nullptr;
    if (batch == 0) return HE_OK;
    if (cts == nullptr || secret_key == nullptr) return invalid_argument("null ciphertexts or secret key");
    const BfvContext& bfv = *ctx->impl;
    // A caller's workspace holds what he_bfv_decrypt_workspace_bytes reports, whichever entry this is (he_amd.h): the dot
    // product, which leaves its result in the caller's slab, uses less of it, and still refuses a shorter one.
    if (workspace != nullptr &&
        workspace_bytes < he_bfv_decrypt_workspace_bytes(ctx, 8 * sizeof(W), moduli_count, poly_count, is_eval, batch))
        return invalid_argument("workspace too small");
    const size_t copy_words = decrypt_copy_words(bfv, moduli_count, poly_count, is_eval != 0, batch);
    const size_t dot_words = dot == nullptr ? decrypt_dot_words(bfv, moduli_count, batch) : 0;
    uint64_t* base = nullptr;
    if (copy_words + dot_words != 0)
        HEAMD_TRY_STATUS(resolve_workspace(workspace, workspace_bytes, (copy_words + dot_words) * sizeof(W), scratch, &base));
    W* words = reinterpret_cast<W*>(base);
    W* out = dot != nullptr ? static_cast<W*>(dot) : words;
    HEAMD_TRY_STATUS(secret_dot_product(ctx, moduli_count, poly_count, is_eval != 0, static_cast<const W*>(cts),
                                        static_cast<const W*>(secret_key), out, batch, words + dot_words, stream));
    *dot_out = out;
    return HE_OK;
}

template <typename W>
int decrypt_words(const he_bfv_context* ctx, const RnsToolLevel& tool, uint32_t moduli_count, uint32_t poly_count, int is_eval,
                  const void* cts, const void* secret_key, u64 scaling_factor, void* out_plaintexts, size_t batch,
                  void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (batch != 0 && out_plaintexts == nullptr) return invalid_argument("null plaintexts");
    Scratch scratch(stream);
    W* dot = nullptr;
    HEAMD_TRY_STATUS(decrypt_dot<W>(ctx, moduli_count, poly_count, is_eval, cts, secret_key, nullptr, batch, workspace,
                                    workspace_bytes, scratch, stream, &dot));
    if (dot == nullptr) return HE_OK;
    const u64 t = ctx->impl->plaintext_modulus();
    const u64 scaled = heamd::mul_mod(tool.device.inv_gamma_mod_t, scaling_factor, t);  // RnsTool.swift:298
    const heamd::U64x2 final_scale{scaled, heamd::shoup_factor(scaled, t)};
    HEAMD_HIP_TRY(heamd::launch_scale_and_round(dot, static_cast<W*>(out_plaintexts), tool.device, final_scale, batch, stream));
    return HE_OK;
}

// Q = q_0 .. q_{L-1} as little-endian 64-bit limbs, without leading zero limbs
std::vector<u64> modulus_product_limbs(const std::vector<u64>& moduli) {
    std::vector<u64> limbs{1};
    for (u64 q : moduli) {
        u64 carry = 0;
        for (u64& limb : limbs) {
            const heamd::u128 product = static_cast<heamd::u128>(limb) * q + carry;
            limb = static_cast<u64>(product);
            carry = static_cast<u64>(product >> 64);
        }
        if (carry != 0) limbs.push_back(carry);
    }
    return limbs;
}

// t mod q_i, and (Q + 1) >> 1 in the norm kernel's mixed radix (decrypt_kernels.hpp).  Q is odd -- every q_i is an NTT
// modulus --, so (Q + 1) >> 1 is the inverse of 2 mod Q and its residue mod q_i is (q_i + 1) / 2; Garner's digits follow from
// the residues with the q_j^-1 mod q_i the context holds for divideAndRoundQLast.
void noise_norm_tables(const BfvContext& bfv, uint32_t moduli_count, NoiseNormTables& tables) {
    const PolyContext& pc = *bfv.ciphertext(moduli_count);
    const std::vector<u64>& q = pc.moduli();
    u64 residue[heamd::kMaxNoiseModuli];
    for (uint32_t i = 0; i < moduli_count; ++i) {
        const u64 t = bfv.plaintext_modulus() % q[i];
        tables.t_mod_q[i] = heamd::U64x2{t, heamd::shoup_factor(t, q[i])};
        residue[i] = (q[i] + 1) / 2;
    }
    for (uint32_t j = moduli_count; j-- > 0;) {
        tables.half_digits[j] = residue[j];
        const heamd::U64x2* inverse_q_j = pc.host_inverse_q_last(j);
        for (uint32_t i = 0; i < j; ++i) {
            const u64 difference = (residue[i] + q[i] - residue[j] % q[i]) % q[i];  // (moduli are below 2^62)
            residue[i] = heamd::mul_mod(difference, inverse_q_j[i].x, q[i]);
        }
    }
    tables.limbs = static_cast<uint32_t>(modulus_product_limbs(q).size());
}

template <typename W>
int noise_norm_words(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, int is_eval, const void* cts,
                     const void* secret_key, uint64_t* out_limbs, size_t batch, void* workspace, size_t workspace_bytes,
                     hipStream_t stream) {
    if (batch != 0 && out_limbs == nullptr) return invalid_argument("null limbs");
    Scratch scratch(stream);
    W* dot = nullptr;
    HEAMD_TRY_STATUS(decrypt_dot<W>(ctx, moduli_count, poly_count, is_eval, cts, secret_key, nullptr, batch, workspace,
                                    workspace_bytes, scratch, stream, &dot));
    if (dot == nullptr) return HE_OK;
    NoiseNormTables tables{};
    noise_norm_tables(*ctx->impl, moduli_count, tables);
    const DeviceContext dc = ctx->impl->ciphertext(moduli_count)->device_context();
    HEAMD_HIP_TRY(heamd::launch_noise_norm(dot, out_limbs, dc, tables, batch, stream));
    return HE_OK;
}

// Double(norm) for a multi-limb integer, rounded to nearest, ties to even: the top 64 bits with every lower bit folded into
// the lowest of them (far below the 53 bits a double keeps), converted by the hardware's own rounding, then scaled exactly
double limbs_to_double(const uint64_t* limbs, uint32_t count) {
    while (count != 0 && limbs[count - 1] == 0) --count;
    if (count == 0) return 0.0;
    if (count == 1) return static_cast<double>(limbs[0]);
    const int shift = 64 * static_cast<int>(count - 2) + heamd::bit_length(limbs[count - 1]);  // bits below the top 64
    const uint32_t word = static_cast<uint32_t>(shift / 64), offset = static_cast<uint32_t>(shift % 64);
    uint64_t top = limbs[word] >> offset;
    if (offset != 0) top |= limbs[word + 1] << (64 - offset);
    bool sticky = offset != 0 && (limbs[word] & ((uint64_t(1) << offset) - 1)) != 0;
    for (uint32_t i = 0; i < word; ++i) sticky = sticky || limbs[i] != 0;
    return std::ldexp(static_cast<double>(top | (sticky ? 1 : 0)), shift);
}

}  // namespace
// word_layer.hpp
int heamd::check_word_and_context(const he_bfv_context* ctx, uint32_t word_bits) {
    HEAMD_TRY_STATUS(check_word_bits(word_bits));
    if (ctx == nullptr) return invalid_argument("null context");
    if (word_bits == 32 && ctx->impl->word_bits() != 32) return invalid_argument("4-byte slabs need a Bfv<UInt32> context");
    return HE_OK;
}
int heamd::bfv_decrypt_check_device(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count) {
    HEAMD_TRY_STATUS(check_word_bits(word_bits));
    const RnsToolLevel* tool = nullptr;
    return check_level(ctx, moduli_count, &tool, word_bits / 8);
}
}  // extern "C++"

size_t he_bfv_decrypt_workspace_bytes(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, uint32_t poly_count,
                                      int is_eval, size_t batch) {
    if (ctx == nullptr || !ctx->impl->valid(moduli_count) || (word_bits != 32 && word_bits != 64) || poly_count < 1 ||
        poly_count > heamd::kMaxDecryptPolys)
        return 0;
    const BfvContext& bfv = *ctx->impl;
    return (decrypt_dot_words(bfv, moduli_count, batch) + decrypt_copy_words(bfv, moduli_count, poly_count, is_eval != 0, batch)) *
           (word_bits / 8);
}

int he_bfv_secret_dot_product_device(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, uint32_t poly_count,
                                     int is_eval, const void* cts, const void* secret_key, void* out, size_t batch,
                                     void* workspace, size_t workspace_bytes, he_stream s) {
    const RnsToolLevel* tool = nullptr;
    HEAMD_TRY_STATUS(check_decrypt_arguments(ctx, word_bits, moduli_count, poly_count, &tool, "dotProduct", cts, secret_key, batch,
                                             {"out", out, batch * moduli_count * (word_bits / 8), true}, 0, workspace,
                                             workspace_bytes));
    if (batch != 0 && out == nullptr) return invalid_argument("null dot product");
    Scratch scratch(as_stream(s));
    return heamd::with_word(word_bits, [&](auto word) {
        decltype(word)* dot = nullptr;
        return decrypt_dot(ctx, moduli_count, poly_count, is_eval, cts, secret_key, out, batch, workspace, workspace_bytes, scratch,
                           as_stream(s), &dot);
    });
}

int he_bfv_decrypt_device(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, uint32_t poly_count, int is_eval,
                          const void* cts, const void* secret_key, uint64_t correction_factor, void* out_plaintexts,
                          size_t batch, void* workspace, size_t workspace_bytes, he_stream s) {
    const RnsToolLevel* tool = nullptr;
    HEAMD_TRY_STATUS(check_decrypt_arguments(ctx, word_bits, moduli_count, poly_count, &tool, "decrypt", cts, secret_key, batch,
                                             {"out_plaintexts", out_plaintexts, batch * (word_bits / 8), true}, 0, workspace,
                                             workspace_bytes));
    const u64 t = ctx->impl->plaintext_modulus();
    if (correction_factor >= t) return invalid_argument("correction factor not reduced mod t");
    u64 scaling_factor = 0;  // correctionFactor.inverseMod(modulus: t) (Bfv+Decrypt.swift:34)
    if (!heamd::inverse_mod(correction_factor, t, scaling_factor)) {
        heamd::set_last_error("the correction factor has no inverse mod t");
        return HE_ERR_NOT_INVERTIBLE;
    }
    return heamd::with_word(word_bits, [&](auto word) {
        return decrypt_words<decltype(word)>(ctx, *tool, moduli_count, poly_count, is_eval, cts, secret_key, scaling_factor,
                                             out_plaintexts, batch, workspace, workspace_bytes, as_stream(s));
    });
}

int he_bfv_noise_norm_device(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, uint32_t poly_count,
                             int is_eval, const void* cts, const void* secret_key, uint64_t* out_limbs, size_t batch,
                             void* workspace, size_t workspace_bytes, he_stream s) {
    const RnsToolLevel* tool = nullptr;
    HEAMD_TRY_STATUS(check_decrypt_arguments(ctx, word_bits, moduli_count, poly_count, &tool, "noiseNorm", cts, secret_key, batch,
                                             {"out_limbs", out_limbs, 0, true},
                                             batch * he_bfv_noise_norm_limbs(ctx, moduli_count) * sizeof(uint64_t), workspace,
                                             workspace_bytes));
    return heamd::with_word(word_bits, [&](auto word) {
        return noise_norm_words<decltype(word)>(ctx, moduli_count, poly_count, is_eval, cts, secret_key, out_limbs, batch, workspace,
                                                workspace_bytes, as_stream(s));
    });
}

int he_bfv_is_transparent_device(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, uint32_t poly_count,
                                 const void* cts, uint8_t* out_flags, size_t batch, he_stream s) {
    const RnsToolLevel* tool = nullptr;
    HEAMD_TRY_STATUS(check_decrypt_arguments(ctx, word_bits, moduli_count, poly_count, &tool, "isTransparent", cts, nullptr, batch,
                                             {"out_flags", out_flags, 0, true}, batch, nullptr, 0));
    if (batch == 0) return HE_OK;
    if (cts == nullptr || out_flags == nullptr) return invalid_argument("null ciphertexts or flags");
    const uint32_t log_degree = tool->device.log_degree;
    return heamd::with_word(word_bits, [&](auto word) {
        HEAMD_HIP_TRY(heamd::launch_is_transparent(static_cast<const decltype(word)*>(cts), out_flags, log_degree, moduli_count,
                                                   poly_count, batch, as_stream(s)));
        return int(HE_OK);
    });
}

uint32_t he_bfv_noise_norm_limbs(const he_bfv_context* ctx, uint32_t moduli_count) {
    if (ctx == nullptr || !ctx->impl->valid(moduli_count)) return 0;
    return static_cast<uint32_t>(modulus_product_limbs(ctx->impl->ciphertext(moduli_count)->moduli()).size());
}

int he_bfv_noise_budget_from_norm(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, const uint64_t* limbs,
                                  int variable_time, double* out) {
    if (ctx == nullptr) return invalid_argument("null context");
    if (word_bits != 32 && word_bits != 64) return invalid_argument("word_bits must be 32 or 64");
    if (!ctx->impl->valid(moduli_count)) return invalid_argument("moduli_count out of range");
    if (limbs == nullptr || out == nullptr) return invalid_argument("null limbs or result");
    const std::vector<u64>& q = ctx->impl->ciphertext(moduli_count)->moduli();
    double q_double = 1.0;
    for (u64 modulus : q) q_double *= static_cast<double>(modulus);
    // the reference composes in the narrowest of T, T.DoubleWidth, ... that holds crtComposeMaxIntermediateValue
    // (CrtComposer.swift:54-61), and anything wider than T is precondition(variableTime) (Bfv+Decrypt.swift:151-173)
    const double t_max = word_bits == 32 ? static_cast<double>(UINT32_MAX) : static_cast<double>(UINT64_MAX);
    const double crt_max = q.size() == 1 ? static_cast<double>(q[0]) : 2.0 * q_double;
    if (!(crt_max < std::pow(t_max, 32))) return invalid_argument("crtComposeMaxIntermediateValue too large");
    if (!(crt_max < t_max) && variable_time == 0)
        return invalid_argument("the composed coefficients are wider than a word: variable_time must be set");
    const double norm = limbs_to_double(limbs, he_bfv_noise_norm_limbs(ctx, moduli_count));
    *out = norm == 0.0 ? std::numeric_limits<double>::infinity() : std::log2(q_double / (2.0 * norm));
    return HE_OK;
}

// ------------------------------------------------------------------------------------------ plaintext <-> Eval
extern "C++" {
template <typename W>
int heamd::bfv_plaintext_to_eval(const he_bfv_context* ctx, uint32_t moduli_count, const W* plaintext, W* out, size_t batch,
                                 hipStream_t stream) {
    const RnsToolLevel* tool = nullptr;
    int status = check_level(ctx, moduli_count, &tool, sizeof(W), [&](size_t n) {  // one row in, L rows out per plaintext
        return heamd::check_slabs("convertToEvalFormat", {{"out", out, batch * moduli_count * n * sizeof(W), true},
                                                          {"plaintext", plaintext, batch * n * sizeof(W), false}});
    });
    if (status != HE_OK) return status;
    if (batch == 0) return HE_OK;
    if (plaintext == nullptr || out == nullptr) return invalid_argument("null plaintext");
    const PolyContext* q_ctx = ctx->impl->ciphertext(moduli_count);
    const DeviceContext dc = q_ctx->device_context(moduli_count);
    // Plaintext.convertToEvalFormat (Plaintext.swift:149-170): centered lift, then forwardNtt -- for 8-byte words one kernel
    // where the degree has a tiled NTT (the lift rides the transform's load), two launches otherwise
    if constexpr (sizeof(W) == 8) {
        hipError_t fused = heamd::launch_ntt_lift(plaintext, ctx->impl->plaintext_modulus(), batch, out, dc, stream);
        if (fused != hipErrorNotSupported) {
            HEAMD_HIP_TRY(fused);
            return HE_OK;
        }
        (void)hipGetLastError();
    }
    HEAMD_HIP_TRY(heamd::launch_plaintext_lift(plaintext, out, dc, ctx->impl->plaintext_modulus(), batch, stream));
    HEAMD_HIP_TRY(ntt_rows(false, out, *q_ctx, dc, moduli_count, batch * moduli_count, stream));
    return HE_OK;
}
template int heamd::bfv_plaintext_to_eval(const he_bfv_context*, uint32_t, const uint64_t*, uint64_t*, size_t, hipStream_t);
template int heamd::bfv_plaintext_to_eval(const he_bfv_context*, uint32_t, const uint32_t*, uint32_t*, size_t, hipStream_t);

namespace {
template <typename W>
int plaintext_to_coeff(const he_bfv_context* ctx, uint32_t moduli_count, const W* plaintext_eval, W* out, size_t batch,
                       he_stream s) {
    const RnsToolLevel* tool = nullptr;
    int status = check_level(ctx, moduli_count, &tool, sizeof(W), [&](size_t n) {  // L rows in, one row out per plaintext
        return heamd::check_slabs("convertToCoeffFormat", {{"out", out, batch * n * sizeof(W), true},
                                                           {"plaintext_eval", plaintext_eval, batch * moduli_count * n * sizeof(W), false}});
    });
    if (status != HE_OK) return status;
    if (batch == 0) return HE_OK;
    if (plaintext_eval == nullptr || out == nullptr) return invalid_argument("null plaintext");
    hipStream_t stream = as_stream(s);
    const PolyContext* q_ctx = ctx->impl->ciphertext(moduli_count);
    const DeviceContext dc = q_ctx->device_context(moduli_count);
    const size_t n = ctx->impl->degree();
    // Plaintext.convertToCoeffFormat (Plaintext.swift:176-191) keeps residue row 0 only and rows are independent
    // under the inverse NTT, so only row 0 is transformed
    HEAMD_HIP_TRY(heamd::launch_first_rows(plaintext_eval, out, dc, batch, stream));
    HEAMD_HIP_TRY(ntt_rows(true, out, *q_ctx, dc, 1, batch, stream));  // (not ntt_records: its 8-byte schedule is the [Q, Bsk] one)
    HEAMD_HIP_TRY(heamd::launch_plaintext_unlift(out, q_ctx->moduli()[0], ctx->impl->plaintext_modulus(), batch * n,
                                                 stream));
    return HE_OK;
}
}  // namespace
}  // extern "C++"

int he_bfv_plaintext_to_eval_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* plaintext,
                                    uint64_t* out, size_t batch, he_stream s) {
    return heamd::bfv_plaintext_to_eval(ctx, moduli_count, plaintext, out, batch, as_stream(s));
}
int he_bfv_plaintext_to_eval_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* plaintext,
                                        uint32_t* out, size_t batch, he_stream s) {
    return heamd::bfv_plaintext_to_eval(ctx, moduli_count, plaintext, out, batch, as_stream(s));
}
int he_bfv_plaintext_to_coeff_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* plaintext_eval,
                                     uint64_t* out, size_t batch, he_stream s) {
    return plaintext_to_coeff(ctx, moduli_count, plaintext_eval, out, batch, s);
}
int he_bfv_plaintext_to_coeff_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* plaintext_eval,
                                         uint32_t* out, size_t batch, he_stream s) {
    return plaintext_to_coeff(ctx, moduli_count, plaintext_eval, out, batch, s);
}

// ------------------------------------------------------------------------------------------ mod switch, ct x pt
extern "C++" {
namespace {
template <typename W>
int mod_switch_down(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, const W* in, W* out, size_t batch,
                    he_stream s) {
    const RnsToolLevel* tool = nullptr;
    int status = check_level(ctx, moduli_count, &tool, sizeof(W), [&](size_t n) {  // as he_poly_divide_and_round_q_last_device
        const size_t row = batch * poly_count * n * sizeof(W);
        return heamd::check_slabs("modSwitchDown", {{"out", out, row * (moduli_count - 1), true}, {"in", in, row * moduli_count, false}});
    });
    if (status != HE_OK) return status;
    if (moduli_count < 2) return HE_ERR_INVALID_POLY_CONTEXT;  // PolyRq.swift:366-368
    if (batch == 0 || poly_count == 0) return HE_OK;
    if (in == nullptr || out == nullptr) return invalid_argument("null ciphertext");
    HEAMD_HIP_TRY(divide_and_round_q_last(in, out, *ctx->impl->ciphertext(moduli_count), moduli_count, batch * poly_count,
                                          as_stream(s)));
    return HE_OK;
}

template <typename W>
int mul_plain_entry(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, W* ct, const W* pt, size_t batch,
                    he_stream s) {
    const RnsToolLevel* tool = nullptr;
    // a lane reads word k of plaintext b and updates word k of every polynomial of ciphertext b: pt may be ct itself where no
    // lane reads what another writes -- one polynomial per ciphertext (a square), or one ciphertext (times its own c0)
    int status = check_level(ctx, moduli_count, &tool, sizeof(W), [&](size_t n) {
        const size_t poly_bytes = batch * moduli_count * n * sizeof(W);
        return heamd::check_slabs("ct x pt", {{"ct", ct, poly_count * poly_bytes, true}, {"pt", pt, poly_bytes, false}},
                                  batch == 1 || poly_count == 1 ? std::pair<int, int>{0, 1} : std::pair<int, int>{-1, -1});
    });
    if (status != HE_OK) return status;
    if (batch == 0 || poly_count == 0) return HE_OK;
    if (ct == nullptr || pt == nullptr) return invalid_argument("null operand");
    const PolyContext* pc = ctx->impl->ciphertext(moduli_count);
    HEAMD_HIP_TRY(mul_plain(ct, pt, pc->device_context(), poly_count, batch, as_stream(s)));
    return HE_OK;
}

// Bfv.addAssignCoeff / subAssignCoeff(_: inout CoeffCiphertext, _: CoeffPlaintext) (Bfv/Bfv.swift:110-117) =
// plaintextTranslate (Bfv/Bfv+Encrypt.swift:75-140)
template <typename W>
int plaintext_translate(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, W* ct, const W* plaintexts,
                        bool subtract, size_t batch, he_stream s) {
    const RnsToolLevel* tool = nullptr;
    const int status = check_level(ctx, moduli_count, &tool, sizeof(W), [&](size_t n) {  // one plaintext row spreads over L rows
        return heamd::check_slabs(subtract ? "ct - pt" : "ct + pt",
                                  {{"ct", ct, batch * poly_count * moduli_count * n * sizeof(W), true},
                                   {"plaintexts", plaintexts, batch * n * sizeof(W), false}});
    });
    if (status != HE_OK) return status;
    if (poly_count == 0) return invalid_argument("a ciphertext has at least one polynomial");
    if (batch == 0) return HE_OK;
    if (ct == nullptr || plaintexts == nullptr) return invalid_argument("null operand");
    HEAMD_HIP_TRY(heamd::launch_plaintext_translate(ct, plaintexts, tool->device, poly_count, subtract, batch, as_stream(s)));
    return HE_OK;
}
}  // namespace

// Ciphertext.modSwitchDownToSingle (Bfv.swift:163-171): moduli_count -> 1 moduli
template <typename W>
int heamd::bfv_mod_switch_down_to_single(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, const W* in,
                                         W* out, size_t batch, hipStream_t stream) {
    const RnsToolLevel* tool = nullptr;
    // at one modulus the ciphertext is already there: out == in is the no-op it always was; any other overlap, and every
    // overlap at more moduli (rows L p .. read, row p written), is refused
    int status = check_level(ctx, moduli_count, &tool, sizeof(W), [&](size_t n) {
        const size_t row = batch * poly_count * n * sizeof(W);
        return heamd::check_slabs("modSwitchDownToSingle", {{"out", out, row, true}, {"in", in, row * moduli_count, false}},
                                  moduli_count == 1 ? std::pair<int, int>{0, 1} : std::pair<int, int>{-1, -1});
    });
    if (status != HE_OK) return status;
    if (batch == 0 || poly_count == 0) return HE_OK;
    if (in == nullptr || out == nullptr) return invalid_argument("null ciphertext");
    const size_t polys = batch * poly_count, n = ctx->impl->degree();
    if (moduli_count == 1) {  // already there
        if (in != out) HEAMD_HIP_TRY(hipMemcpyAsync(out, in, polys * n * sizeof(W), hipMemcpyDeviceToDevice, stream));
        return HE_OK;
    }
    if constexpr (sizeof(W) == 8) {  // one kernel for 2..8 moduli
        const PolyContext* pc = ctx->impl->ciphertext(moduli_count);
        hipError_t e = heamd::launch_mod_switch_down_to_single(in, out, pc->device_context(), moduli_count, polys, stream);
        if (e != hipErrorNotSupported) {
            HEAMD_HIP_TRY(e);
            return HE_OK;
        }
        (void)hipGetLastError();
    }
    // step by step; the levels between the first and the last alternate between two scratch slabs
    Scratch level_mem(stream);
    const size_t level_words = polys * size_t(moduli_count - 1) * n;
    if (moduli_count > 2) HEAMD_HIP_TRY(level_mem.allocate(2 * level_words * sizeof(W)));
    W* ping = static_cast<W*>(level_mem.get());
    W* pong = ping != nullptr ? ping + level_words : nullptr;
    const W* current = in;
    for (uint32_t level = moduli_count; level > 1; --level) {
        W* target = level == 2 ? out : (current == ping ? pong : ping);
        HEAMD_HIP_TRY(divide_and_round_q_last(current, target, *ctx->impl->ciphertext(level), level, polys, stream));
        current = target;
    }
    return HE_OK;
}
template int heamd::bfv_mod_switch_down_to_single(const he_bfv_context*, uint32_t, uint32_t, const uint64_t*, uint64_t*, size_t,
                                                  hipStream_t);
template int heamd::bfv_mod_switch_down_to_single(const he_bfv_context*, uint32_t, uint32_t, const uint32_t*, uint32_t*, size_t,
                                                  hipStream_t);
}  // extern "C++"

int he_bfv_mod_switch_down_device(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count,
                                  const uint64_t* in, uint64_t* out, size_t batch, he_stream s) {
    return mod_switch_down(ctx, moduli_count, poly_count, in, out, batch, s);
}
int he_bfv_mod_switch_down_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count,
                                      const uint32_t* in, uint32_t* out, size_t batch, he_stream s) {
    return mod_switch_down(ctx, moduli_count, poly_count, in, out, batch, s);
}
// (there is no 4-byte twin in the C ABI: the 4-byte PNNS and PIR responses call the body)
int he_bfv_mod_switch_down_to_single_device(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count,
                                            const uint64_t* in, uint64_t* out, size_t batch, he_stream s) {
    return heamd::bfv_mod_switch_down_to_single(ctx, moduli_count, poly_count, in, out, batch, as_stream(s));
}

int he_bfv_mul_plain_device(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, uint64_t* ct,
                            const uint64_t* pt, size_t batch, he_stream s) {
    return mul_plain_entry(ctx, moduli_count, poly_count, ct, pt, batch, s);
}
int he_bfv_mul_plain_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, uint32_t* ct,
                                const uint32_t* pt, size_t batch, he_stream s) {
    return mul_plain_entry(ctx, moduli_count, poly_count, ct, pt, batch, s);
}
int he_bfv_add_plain_device(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, uint64_t* ct,
                            const uint64_t* plaintexts, size_t batch, he_stream s) {
    return plaintext_translate(ctx, moduli_count, poly_count, ct, plaintexts, false, batch, s);
}
int he_bfv_add_plain_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, uint32_t* ct,
                                const uint32_t* plaintexts, size_t batch, he_stream s) {
    return plaintext_translate(ctx, moduli_count, poly_count, ct, plaintexts, false, batch, s);
}
int he_bfv_sub_plain_device(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, uint64_t* ct,
                            const uint64_t* plaintexts, size_t batch, he_stream s) {
    return plaintext_translate(ctx, moduli_count, poly_count, ct, plaintexts, true, batch, s);
}
int he_bfv_sub_plain_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, uint32_t* ct,
                                const uint32_t* plaintexts, size_t batch, he_stream s) {
    return plaintext_translate(ctx, moduli_count, poly_count, ct, plaintexts, true, batch, s);
}

extern "C++" {
namespace {
// Bfv.innerProduct(ciphertexts:plaintexts:) (Bfv/Bfv.swift:476-505) with the nil-plaintext mask resident on the device
template <typename W>
int inner_product_plain(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, const W* cts, const W* pts,
                        const uint8_t* present_device, size_t count, size_t columns, W* out, hipStream_t stream) {
    const PolyContext* pc = ctx->impl->ciphertext(moduli_count);
    const heamd::AccumulatorCadence lazy = heamd::accumulator_cadence(*pc, moduli_count);
    HEAMD_HIP_TRY(heamd::launch_inner_product_plain(cts, pts, present_device, out, pc->device_context(), poly_count,
                                                    count, columns, lazy.max_lazy, lazy.cadence, lazy.narrow_moduli, stream));
    return HE_OK;
}
// (the resident entry looks at the word size before the level, unlike every other 4-byte entry;
// tests/test_word_twin_status.py pins the order)
// plaintext_bytes(n): the bytes of one plaintext in pts (L rows of words, or packed); present_device: the device mask or null
template <typename PlaintextBytes>
int check_inner_product_plain(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, const void* cts,
                              const void* pts, const void* present_device, size_t count, size_t columns, const void* out,
                              bool* nothing_to_do, size_t word_bytes, PlaintextBytes plaintext_bytes) {
    if (word_bytes == 4 && ctx != nullptr && ctx->impl->word_bits() != 32)
        return invalid_argument("4-byte slabs need a Bfv<UInt32> context");
    const RnsToolLevel* tool = nullptr;
    int status = check_level(ctx, moduli_count, &tool, 8, [&](size_t n) {
        const size_t ct_bytes = size_t(poly_count) * moduli_count * n * word_bytes;
        return heamd::check_slabs("innerProduct", {{"out", out, columns * ct_bytes, true},
                                                   {"cts", cts, count * ct_bytes, false},
                                                   {"pts", pts, columns * count * plaintext_bytes(n), false},
                                                   {"present_device", present_device, columns * count, false}});
    });
    if (status != HE_OK) return status;
    *nothing_to_do = false;
    if (count == 0) return invalid_argument("empty ciphertext vector");  // precondition, Bfv.swift:481-483
    if (columns == 0) {
        *nothing_to_do = true;
        return HE_OK;
    }
    if (cts == nullptr || pts == nullptr || out == nullptr) return invalid_argument("null operand");
    if (poly_count < 1 || poly_count > 8 || poly_count == 5 || poly_count == 7)
        return invalid_argument("poly_count must be 1, 2, 3, 4, 6 or 8");
    return HE_OK;
}
}  // namespace
template <typename W>
int heamd::bfv_inner_product_plain_resident(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, const W* cts,
                                            const W* pts, const uint8_t* present_device, size_t count, size_t columns, W* out,
                                            hipStream_t stream) {
    bool nothing = false;
    int status = check_inner_product_plain(ctx, moduli_count, poly_count, cts, pts, present_device, count, columns, out, &nothing,
                                           sizeof(W), [&](size_t n) { return moduli_count * n * sizeof(W); });
    if (status != HE_OK || nothing) return status;
    return inner_product_plain(ctx, moduli_count, poly_count, cts, pts, present_device, count, columns, out, stream);
}
template int heamd::bfv_inner_product_plain_resident(const he_bfv_context*, uint32_t, uint32_t, const uint64_t*, const uint64_t*,
                                                     const uint8_t*, size_t, size_t, uint64_t*, hipStream_t);
template int heamd::bfv_inner_product_plain_resident(const he_bfv_context*, uint32_t, uint32_t, const uint32_t*, const uint32_t*,
                                                     const uint8_t*, size_t, size_t, uint32_t*, hipStream_t);

heamd::AccumulatorCadence heamd::accumulator_cadence(const PolyContext& pc, uint32_t level) {
    AccumulatorCadence lazy{pc.max_lazy_product_accumulation_count(level), 0, true};
    // the carry-counting accumulator's reduction wants sums below 2^127: at most 2^127 / (p_max - 1)^2 products
    lazy.cadence = lazy.max_lazy;
    for (uint32_t i = 0; i < level; ++i) {
        lazy.narrow_moduli = lazy.narrow_moduli && (pc.moduli()[i] >> 56) == 0;
        const unsigned __int128 below = pc.moduli()[i] - 1;
        if (below == 0) continue;
        // a window starts from the previous window's folded residue (< p), so cadence (p - 1)^2 + p - 1 must stay
        // below 2^127
        const unsigned __int128 limit = ((static_cast<unsigned __int128>(1) << 127) - pc.moduli()[i]) / (below * below);
        if (limit < lazy.cadence) lazy.cadence = static_cast<uint64_t>(limit);
    }
    return lazy;
}
}  // extern "C++"

int he_bfv_inner_product_plain_device(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count,
                                      const uint64_t* cts, const uint64_t* pts, const uint8_t* present, size_t count,
                                      size_t columns, uint64_t* out, he_stream s) {
    bool nothing = false;
    int status = check_inner_product_plain(ctx, moduli_count, poly_count, cts, pts, nullptr, count, columns, out, &nothing, 8,
                                           [&](size_t n) { return moduli_count * n * sizeof(uint64_t); });
    if (status != HE_OK || nothing) return status;
    hipStream_t stream = as_stream(s);
    Scratch scratch(stream);
    const uint8_t* present_device = nullptr;
    if (present != nullptr) {
        HEAMD_HIP_TRY(scratch.allocate(count * columns));
        HEAMD_HIP_TRY(hipMemcpyAsync(scratch.get(), present, count * columns, hipMemcpyHostToDevice, stream));
        HEAMD_HIP_TRY(hipStreamSynchronize(stream));  // `present` is a borrowed pageable host buffer
        present_device = static_cast<const uint8_t*>(scratch.get());
    }
    return inner_product_plain(ctx, moduli_count, poly_count, cts, pts, present_device, count, columns, out, stream);
}

int he_bfv_inner_product_plain_resident_device(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count,
                                               const uint64_t* cts, const uint64_t* pts, const uint8_t* present_device,
                                               size_t count, size_t columns, uint64_t* out, he_stream s) {
    return heamd::bfv_inner_product_plain_resident(ctx, moduli_count, poly_count, cts, pts, present_device, count, columns, out,
                                                   as_stream(s));
}
int he_bfv_inner_product_plain_resident_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count,
                                                   const uint32_t* cts, const uint32_t* pts,
                                                   const uint8_t* present_device, size_t count, size_t columns,
                                                   uint32_t* out, he_stream s) {
    return heamd::bfv_inner_product_plain_resident(ctx, moduli_count, poly_count, cts, pts, present_device, count, columns, out,
                                                   as_stream(s));
}

// ------------------------------------------------------------------------------------------ packed plaintexts
extern "C++" {
namespace {
// 8-byte words of one packed plaintext over pc: what packed_layout lays out, without looking at the device (the pointer contract
// of the packed entries is checked on host-only contexts too)
size_t packed_plaintext_words(const PolyContext& pc) {
    size_t words = 0;
    for (uint64_t q : pc.moduli()) words += pc.degree() / 64 * static_cast<size_t>(64 - __builtin_clzll(q));
    return words;
}

// bits(q_r) per word, rows in whole 8-byte words (degree a multiple of 64)
int packed_layout(const he_bfv_context* ctx, uint32_t moduli_count, heamd::PackedLayout& layout) {
    const RnsToolLevel* tool = nullptr;
    int status = check_level(ctx, moduli_count, &tool);
    if (status != HE_OK) return status;
    const PolyContext* pc = ctx->impl->ciphertext(moduli_count);
    if (moduli_count > heamd::kMaxPackedRows || pc->degree() < 256) {
        heamd::set_last_error("packed plaintexts need degree >= 256 and at most 8 moduli");
        return HE_ERR_UNSUPPORTED;
    }
    layout.rows = moduli_count;
    layout.word_offset[0] = 0;
    for (uint32_t r = 0; r < moduli_count; ++r) {
        layout.width[r] = static_cast<uint32_t>(64 - __builtin_clzll(pc->moduli()[r]));
        layout.word_offset[r + 1] = layout.word_offset[r] + static_cast<uint32_t>(pc->degree() / 64 * layout.width[r]);
    }
    return HE_OK;
}
}  // namespace
}  // extern "C++"

size_t he_bfv_packed_plaintext_words(const he_bfv_context* ctx, uint32_t moduli_count) {
    heamd::PackedLayout layout{};
    if (ctx == nullptr || packed_layout(ctx, moduli_count, layout) != HE_OK) return 0;
    return layout.word_offset[layout.rows];
}

int he_bfv_pack_plaintexts_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* plaintexts_eval,
                                  size_t count, uint64_t* packed, he_stream s) {
    if (ctx != nullptr && ctx->impl->valid(moduli_count)) {  // (an argument check: ahead of the device, as in check_level)
        const PolyContext& pc = *ctx->impl->ciphertext(moduli_count);
        HEAMD_TRY_STATUS(heamd::check_slabs(
            "pack", {{"packed", packed, count * packed_plaintext_words(pc) * sizeof(uint64_t), true},
                     {"plaintexts_eval", plaintexts_eval, count * moduli_count * pc.degree() * sizeof(uint64_t), false}}));
    }
    heamd::PackedLayout layout{};
    int status = packed_layout(ctx, moduli_count, layout);
    if (status != HE_OK) return status;
    if (count == 0) return HE_OK;
    if (plaintexts_eval == nullptr || packed == nullptr) return invalid_argument("null operand");
    const PolyContext* pc = ctx->impl->ciphertext(moduli_count);
    HEAMD_HIP_TRY(heamd::launch_pack_rows(plaintexts_eval, packed, layout, pc->device_context().log_degree, count,
                                          as_stream(s)));
    return HE_OK;
}

int he_bfv_inner_product_plain_packed_device(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count,
                                             const uint64_t* cts, const uint64_t* packed_pts, const uint8_t* present_device,
                                             size_t count, size_t columns, uint64_t* out, he_stream s) {
    bool nothing = false;
    int status = check_inner_product_plain(ctx, moduli_count, poly_count, cts, packed_pts, present_device, count, columns, out,
                                           &nothing, 8, [&](size_t) {
                                               return packed_plaintext_words(*ctx->impl->ciphertext(moduli_count)) * sizeof(uint64_t);
                                           });
    if (status != HE_OK || nothing) return status;
    if (poly_count > 3) return invalid_argument("packed plaintexts take poly_count 1..3");
    heamd::PackedLayout layout{};
    status = packed_layout(ctx, moduli_count, layout);
    if (status != HE_OK) return status;
    const PolyContext* pc = ctx->impl->ciphertext(moduli_count);
    const heamd::AccumulatorCadence lazy = heamd::accumulator_cadence(*pc, moduli_count);
    if (lazy.cadence == 0) {
        heamd::set_last_error("moduli too wide for the packed inner product");
        return HE_ERR_UNSUPPORTED;
    }
    HEAMD_HIP_TRY(heamd::launch_inner_product_plain_packed(cts, packed_pts, layout, present_device, out,
                                                           pc->device_context(), poly_count, count, columns, lazy.cadence,
                                                           lazy.narrow_moduli, as_stream(s)));
    return HE_OK;
}

// ------------------------------------------------------------------------------------------ inner product ct . ct
size_t he_bfv_inner_product_workspace_bytes(const he_bfv_context* ctx, uint32_t moduli_count, size_t count) {
    if (ctx == nullptr || !ctx->impl->valid(moduli_count)) return 0;
    return (count * 4 + 3) * qbsk_poly_words(*ctx->impl, moduli_count) * sizeof(uint64_t);
}

extern "C++" {
namespace {
// Bfv.innerProduct(_: [CanonicalCiphertext], _: [CanonicalCiphertext]) (Bfv/Bfv.swift:315-361)
template <typename W>
int inner_product_pipeline(const he_bfv_context* ctx, const RnsToolLevel* tool, uint32_t L, const W* lhs, const W* rhs,
                           size_t count, W* out, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const size_t n = ctx->impl->degree(), ext = qbsk_poly_words(*ctx->impl, L), rows = 2 * L + 1;
    Scratch scratch(stream);
    uint64_t* raw = nullptr;
    int status = resolve_workspace(workspace, workspace_bytes, (count * 4 + 3) * ext * sizeof(W), scratch, &raw);
    if (status != HE_OK) return status;
    W* lifted = reinterpret_cast<W*>(raw);   // [count][4][2L+1][N]
    W* sum = lifted + count * 4 * ext;       // [3][2L+1][N]
    HEAMD_TRY_STATUS(lift_pairs_to_eval(*tool, L, n, ext, lhs, rhs, lifted, count, stream));
    const DeviceContext qbsk = tool->qbsk->device_context();
    // maxProductCount = maxLazyProductAccumulationCount() / 2 because poly1 takes two products per pair (Bfv.swift:339)
    const uint64_t max_lazy = tool->qbsk->max_lazy_product_accumulation_count(static_cast<uint32_t>(rows)) / 2;
    HEAMD_HIP_TRY(heamd::launch_tensor_accumulate(static_cast<const W*>(lifted), sum, qbsk, count, max_lazy ? max_lazy : 1,
                                                  stream));
    return drop_extended_base(*tool, sum, out, 3, stream);
}

// `items` inner products that share the left vector: lhs [count][2][L][N], rhs [items][count][2][L][N] -> out
// [items][3][L][N].  Every stage is one launch over all items (the left vector is lifted and transformed once).
template <typename W>
int inner_product_shared_pipeline(const he_bfv_context* ctx, const RnsToolLevel* tool, uint32_t L, const W* lhs,
                                  const W* rhs, size_t count, size_t items, W* out, hipStream_t stream) {
    const size_t ext = qbsk_poly_words(*ctx->impl, L), rows = 2 * L + 1;
    Scratch scratch(stream);
    HEAMD_HIP_TRY(scratch.allocate((count * 2 + items * count * 2 + items * 3) * ext * sizeof(W)));
    W* lifted_l = static_cast<W*>(scratch.get());      // [count][2][2L+1][N]
    W* lifted_r = lifted_l + count * 2 * ext;           // [items][count][2][2L+1][N]
    W* sum = lifted_r + items * count * 2 * ext;        // [items][3][2L+1][N]
    HEAMD_HIP_TRY(heamd::launch_lift_q_to_qbsk(lhs, lifted_l, tool->device, count * 2, stream));
    HEAMD_HIP_TRY(heamd::launch_lift_q_to_qbsk(rhs, lifted_r, tool->device, items * count * 2, stream));
    const DeviceContext qbsk = tool->qbsk->device_context();
    // lifted_l and lifted_r are adjacent: one transform launch over both
    HEAMD_HIP_TRY(ntt_records(false, lifted_l, *tool->qbsk, qbsk, static_cast<uint32_t>(rows), (1 + items) * count * 2, stream));
    if constexpr (std::is_same<W, uint64_t>::value) {
        // the carry-counting sums where they exist (rns_kernels.hip tensor_accumulate_shared_sums_kernel)
        const uint64_t cadence = heamd::tensor_sums_cadence(tool->qbsk->moduli().data(), static_cast<uint32_t>(rows));
        const hipError_t sums = heamd::launch_tensor_accumulate_shared_sums(lifted_l, lifted_r, nullptr, 0, sum, qbsk, count, items,
                                                                           cadence, stream);
        if (sums != hipErrorNotSupported) {
            HEAMD_HIP_TRY(sums);
            return drop_extended_base(*tool, sum, out, items * 3, stream);
        }
        (void)hipGetLastError();
    }
    const uint64_t max_lazy = tool->qbsk->max_lazy_product_accumulation_count(static_cast<uint32_t>(rows)) / 2;
    HEAMD_HIP_TRY(heamd::launch_tensor_accumulate_shared(static_cast<const W*>(lifted_l), static_cast<const W*>(lifted_r), sum,
                                                         qbsk, count, items, max_lazy ? max_lazy : 1, stream));
    return drop_extended_base(*tool, sum, out, items * 3, stream);
}
}  // namespace
}  // extern "C++"

// inner_product_shared_pipeline for a right-hand side that arrives in EVAL form over Q (the dim-0 inner products of a PIR
// response as their kernel leaves them, PirUtil.swift:428-437): the Q rows of its lifted records would be those words themselves
// -- the forward transform of the inverse transform of a canonical row is the row -- so the sums read them where they lie, and
// only the Bsk rows go through the inverse transform (out of place, into a Coeff copy), the lift and the forward transform.
// rhs_eval is not written.  kInnerProductEvalUnavailable: nothing launched, the caller takes rhs to Coeff
// (convertToCoeffFormat, PirUtil.swift:438) and calls he_bfv_inner_product_shared_device.
extern "C++" {
namespace heamd {
int bfv_inner_product_shared_eval_rhs(const he_bfv_context* ctx, uint32_t L, const uint64_t* lhs, const uint64_t* rhs_eval,
                                      size_t count, size_t items, uint64_t* out, hipStream_t stream) {
    const RnsToolLevel* tool = nullptr;
    int status = check_level(ctx, L, &tool);
    if (status != HE_OK) return status;
    const PolyContext* q_ctx = ctx->impl->ciphertext(L);
    const DeviceContext qbsk = tool->qbsk->device_context();
    const uint32_t rows = 2 * L + 1;
    const size_t n = ctx->impl->degree(), ext = qbsk_poly_words(*ctx->impl, L), polys = items * count * 2;
    const uint64_t cadence = heamd::tensor_sums_cadence(tool->qbsk->moduli().data(), rows);
    if (q_ctx == nullptr || polys == 0 || cadence == 0 || qbsk.log_degree < 12 || qbsk.log_degree > 13 ||
        polys * rows > (size_t(1) << 30))
        return kInnerProductEvalUnavailable;
    const DeviceContext q_device = q_ctx->device_context();
    if (q_device.approx_ok == 0) return kInnerProductEvalUnavailable;  // (no out-of-place transform for such moduli)
    Scratch scratch(stream), coeff_mem(stream);
    HEAMD_HIP_TRY(scratch.allocate((count * 2 + polys + items * 3) * ext * sizeof(uint64_t)));
    HEAMD_HIP_TRY(coeff_mem.allocate(polys * size_t(L) * n * sizeof(uint64_t)));
    uint64_t* lifted_l = static_cast<uint64_t*>(scratch.get());  // [count][2][2L+1][N]
    uint64_t* lifted_r = lifted_l + count * 2 * ext;              // [items][count][2][2L+1][N]: only the Bsk rows are used
    uint64_t* sum = lifted_r + polys * ext;                       // [items][3][2L+1][N]
    uint64_t* coeff = static_cast<uint64_t*>(coeff_mem.get());    // [items][count][2][L][N]
    HEAMD_HIP_TRY(heamd::launch_lift_q_to_qbsk(lhs, lifted_l, tool->device, count * 2, stream));
    HEAMD_HIP_TRY(ntt_records(false, lifted_l, *tool->qbsk, qbsk, rows, count * 2, stream));
    HEAMD_HIP_TRY(heamd::launch_ntt_inverse_out_of_place(rhs_eval, coeff, q_device, 0, L, polys * L, stream));
    HEAMD_HIP_TRY(heamd::launch_lift_q_to_qbsk_strided(static_cast<const uint64_t*>(coeff), lifted_r, tool->device, polys, 1,
                                                       size_t(L) * n, ext, 0, stream, false));
    HEAMD_HIP_TRY(heamd::launch_ntt_record_band(false, lifted_r, qbsk, rows, L, rows - L, polys, stream));
    HEAMD_HIP_TRY(heamd::launch_tensor_accumulate_shared_sums(lifted_l, lifted_r, rhs_eval, L, sum, qbsk, count, items, cadence,
                                                              stream));
    return drop_extended_base(*tool, sum, out, items * 3, stream);
}
}  // namespace heamd
}  // extern "C++"

extern "C++" {
template <typename W>
int heamd::bfv_inner_product_shared(const he_bfv_context* ctx, uint32_t moduli_count, const W* lhs, const W* rhs, size_t count,
                                    size_t items, W* out, hipStream_t stream) {
    const RnsToolLevel* tool = nullptr;
    // lhs and rhs are only read (lifted into scratch): lhs may be an item of rhs, or all of it
    int status = check_level(ctx, moduli_count, &tool, sizeof(W), [&](size_t n) {
        const size_t poly_bytes = size_t(moduli_count) * n * sizeof(W);
        return heamd::check_slabs("innerProduct", {{"out", out, items * 3 * poly_bytes, true},
                                                   {"lhs", lhs, count * 2 * poly_bytes, false},
                                                   {"rhs", rhs, items * count * 2 * poly_bytes, false}});
    });
    if (status != HE_OK) return status;
    if (count == 0) return invalid_argument("empty ciphertext vector");
    if (items == 0) return HE_OK;
    if (lhs == nullptr || rhs == nullptr || out == nullptr) return invalid_argument("null ciphertext");
    return inner_product_shared_pipeline(ctx, tool, moduli_count, lhs, rhs, count, items, out, stream);
}
template int heamd::bfv_inner_product_shared(const he_bfv_context*, uint32_t, const uint64_t*, const uint64_t*, size_t, size_t,
                                             uint64_t*, hipStream_t);
template int heamd::bfv_inner_product_shared(const he_bfv_context*, uint32_t, const uint32_t*, const uint32_t*, size_t, size_t,
                                             uint32_t*, hipStream_t);
namespace {
template <typename W>
int inner_product_entry(const he_bfv_context* ctx, uint32_t moduli_count, const W* lhs, const W* rhs, size_t count, W* out,
                        void* workspace, size_t workspace_bytes, he_stream s) {
    const RnsToolLevel* tool = nullptr;
    // lhs and rhs are only read (lifted into the workspace): they may be one vector
    int status = check_level(ctx, moduli_count, &tool, sizeof(W), [&](size_t n) {
        const size_t poly_bytes = size_t(moduli_count) * n * sizeof(W);
        return heamd::check_slabs("innerProduct", {{"out", out, 3 * poly_bytes, true},
                                                   {"workspace", workspace, workspace_bytes, true},
                                                   {"lhs", lhs, count * 2 * poly_bytes, false},
                                                   {"rhs", rhs, count * 2 * poly_bytes, false}});
    });
    if (status != HE_OK) return status;
    if (count == 0) return invalid_argument("empty ciphertext vector");
    if (lhs == nullptr || rhs == nullptr || out == nullptr) return invalid_argument("null ciphertext");
    return inner_product_pipeline(ctx, tool, moduli_count, lhs, rhs, count, out, workspace, workspace_bytes, as_stream(s));
}
}  // namespace
}  // extern "C++"

int he_bfv_inner_product_shared_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* lhs,
                                       const uint64_t* rhs, size_t count, size_t items, uint64_t* out, he_stream s) {
    return heamd::bfv_inner_product_shared(ctx, moduli_count, lhs, rhs, count, items, out, as_stream(s));
}
int he_bfv_inner_product_shared_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* lhs,
                                           const uint32_t* rhs, size_t count, size_t items, uint32_t* out, he_stream s) {
    return heamd::bfv_inner_product_shared(ctx, moduli_count, lhs, rhs, count, items, out, as_stream(s));
}
int he_bfv_inner_product_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* lhs,
                                const uint64_t* rhs, size_t count, uint64_t* out, void* workspace,
                                size_t workspace_bytes, he_stream s) {
    return inner_product_entry(ctx, moduli_count, lhs, rhs, count, out, workspace, workspace_bytes, s);
}
int he_bfv_inner_product_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* lhs,
                                    const uint32_t* rhs, size_t count, uint32_t* out, void* workspace,
                                    size_t workspace_bytes, he_stream s) {
    return inner_product_entry(ctx, moduli_count, lhs, rhs, count, out, workspace, workspace_bytes, s);
}

}  // extern "C"
