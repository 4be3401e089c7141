// word_layer.hpp -- the host layer under the C ABI written once for both slab words (not exported): W = uint64_t for
// Bfv<UInt64>, W = uint32_t for Bfv<UInt32> on packed 4-byte slabs (every modulus, Bsk primes included, <= 2^30 - 1).
// Most launchers are templates on W already; the others are overloaded on the slab pointer and differ in the image they
// take, which word_image yields here.  The operations that c_api.cpp, bfv_api.cpp, pnns_api.cpp and pir_api.cpp share are
// declared here, each defined once in the translation unit that owns it.  An extern "C" entry point and its `_u32` twin
// are one-line wrappers of such a body.
#pragma once

#include "api_internal.hpp"
#include "kernels.hpp"

#define HEAMD_TRY_STATUS(expr)                \
    do {                                      \
        const int status_ = (expr);           \
        if (status_ != HE_OK) return status_; \
    } while (0)

namespace heamd {

// ---- the entries that take the slab word as an argument (encrypt, decrypt, the four client files).  body(W{}) for the word W of
// a checked word_bits: with_word(word_bits, [&](auto word) { return f<decltype(word)>(...); })
template <typename Body>
auto with_word(uint32_t word_bits, Body&& body) {
    if (word_bits == 32) return body(uint32_t{});
    return body(uint64_t{});
}
inline int check_word_bits(uint32_t word_bits) {
    return word_bits == 32 || word_bits == 64 ? int(HE_OK) : invalid_argument("word_bits must be 32 or 64");
}
// bfv_api.cpp: the word, the context, the word against the context's scheme (a Bfv<UInt32> context serves 8-byte slabs too)
int check_word_and_context(const he_bfv_context* ctx, uint32_t word_bits);
inline int host_only_refusal() {  // what a device entry answers on a context made without device tables
    set_last_error("context was created host-only (no device tables)");
    return HE_ERR_DEVICE;
}

// ---- launchers by slab word.  `dc` is the 8-byte image the caller chose (a level of the context, constants it may have
// substituted, t N^-1 for instance); word_image yields the image a launch on slabs of W takes: dc itself, or the 4-byte
// image built from `pc` over the `moduli` moduli the launch walks, with dc's constants.  An he_status.
template <typename W>
int word_image(const PolyContext& pc, const DeviceContext& dc, uint32_t moduli, DeviceImage<W>& out) {
    if constexpr (sizeof(W) == 8) {
        out = dc;
        return HE_OK;
    } else {
        const int status = pc.device_context32(moduli, out);
        out.moduli = dc.moduli;
        return status;
    }
}
// Transform of `rows` rows, row r under modulus r % period: ntt_routing.hip / ntt_word32.hip
template <typename W>
hipError_t ntt_rows(bool inverse, W* slab, const PolyContext& pc, const DeviceContext& dc, uint32_t period, size_t rows,
                    hipStream_t stream) {
    DeviceImage<W> image{};
    if (word_image<W>(pc, dc, period, image) != HE_OK) return hipErrorInvalidValue;
    return launch_ntt(inverse, slab, image, 0, period, rows, stream);
}
// Transform of `records` records of record_rows rows: 8-byte words take the mixed schedule of the [Q, Bsk] slabs
template <typename W>
hipError_t ntt_records(bool inverse, W* slab, const PolyContext& pc, const DeviceContext& dc, uint32_t record_rows,
                       size_t records, hipStream_t stream) {
    if constexpr (sizeof(W) == 8) return launch_ntt_mixed(inverse, slab, dc, record_rows, records, stream);
    else return ntt_rows(inverse, slab, pc, dc, record_rows, records * record_rows, stream);
}
// lhs = op(lhs, rhs) over `rows` rows of every modulus of pc; MulScalar reads `scalars`, (scalar, Shoup factor) pairs
template <typename W>
hipError_t elementwise_rows(ElementwiseOp op, W* lhs, const W* rhs, const uint64_t* scalars, const PolyContext& pc, size_t rows,
                            hipStream_t stream) {
    DeviceImage<W> image{};
    if (word_image<W>(pc, pc.device_context(), pc.moduli_count(), image) != HE_OK) return hipErrorInvalidValue;
    return launch_elementwise(op, lhs, rhs, scalars, image, rows, stream);
}
// divideAndRoundQLast of `polys` polynomials over the first moduli_count moduli of pc
template <typename W>
hipError_t divide_and_round_q_last(const W* in, W* out, const PolyContext& pc, uint32_t moduli_count, size_t polys,
                                   hipStream_t stream) {
    DeviceImage<W> image{};
    if (word_image<W>(pc, pc.device_context(), moduli_count, image) != HE_OK) return hipErrorInvalidValue;
    return launch_divide_and_round_q_last(in, out, image, moduli_count, polys, stream);
}
// ct [batch][polys][L][N] *= pt [batch][L][N]: both words read the 8-byte image
template <typename W>
hipError_t mul_plain(W* ct, const W* pt, const DeviceContext& dc, uint32_t poly_count, size_t batch, hipStream_t stream) {
    return launch_mul_plain(ct, pt, dc, poly_count, batch, stream);
}

// What an entry point needs of pc before it launches on slabs of W: its tables on the current device, and for 4-byte
// words every modulus within 2^30 - 1 (HE_ERR_INVALID_MODULUS) and the 4-byte tables, built on first use.
template <typename W>
int check_word_device(const PolyContext& pc) {
    if constexpr (sizeof(W) == 8) return pc.check_device();
    DeviceImage<W> image{};
    return word_image<W>(pc, pc.device_context(), pc.moduli_count(), image);
}
// The 4-byte polynomial entries make that check before they look at the batch, the 8-byte ones behind their argument checks.
template <typename W>
constexpr bool kChecksDeviceFirst = sizeof(W) == 4;

// ---- c_api.cpp: he_ntt_forward/inverse_device and he_poly_add/sub/neg/mul_device, with their checks
template <typename W>
int poly_ntt(const he_poly_context* ctx, W* slab, size_t batch, bool inverse, hipStream_t stream);
template <typename W>
int poly_elementwise(const he_poly_context* ctx, ElementwiseOp op, W* lhs, const W* rhs, size_t batch, hipStream_t stream);

// ---- bfv_api.cpp
// Plaintext.convertToEvalFormat, with the checks of he_bfv_plaintext_to_eval_device (a batch of 0 with null slabs checks
// the level and nothing else)
template <typename W>
int bfv_plaintext_to_eval(const he_bfv_context* ctx, uint32_t moduli_count, const W* plaintext, W* out, size_t batch,
                          hipStream_t stream);
// encrypt_api.cpp: the device-side checks of he_bfv_encrypt_device (a host-only context, the transform of the word), for an
// entry that has to make them before it enqueues work of its own
int bfv_encrypt_check_device(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count);
// bfv_api.cpp: the same for he_bfv_decrypt_device -- the word, the level, the device, the word against the context's scheme
int bfv_decrypt_check_device(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count);
// Ciphertext.modSwitchDownToSingle, with the checks of he_bfv_mod_switch_down_to_single_device: one kernel where 8-byte words
// have it (2..8 moduli), else divideAndRoundQLast level by level through scratch of its own
template <typename W>
int bfv_mod_switch_down_to_single(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, const W* in, W* out,
                                  size_t batch, hipStream_t stream);
// How often the carry-counting accumulator of a plaintext inner product over the first `level` moduli of pc reduces:
// max_lazy is the reference's cadence, cadence (<= max_lazy) keeps the sums below 2^127, narrow_moduli says that every
// modulus is below 2^56 (kernels.hpp, launch_inner_product_plain)
struct AccumulatorCadence {
    uint64_t max_lazy, cadence;
    bool narrow_moduli;
};
AccumulatorCadence accumulator_cadence(const PolyContext& pc, uint32_t level);
// Bfv.innerProduct(ciphertexts:plaintexts:) per column with the nil-plaintext mask on the device, Bfv.innerProduct of `items`
// ciphertext vectors with one shared vector, and Bfv.relinearize: the bodies, checks included, of
// he_bfv_inner_product_plain_resident_device, he_bfv_inner_product_shared_device and he_bfv_relinearize_device
template <typename W>
int bfv_inner_product_plain_resident(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, const W* cts,
                                     const W* pts, const uint8_t* present_device, size_t count, size_t columns, W* out,
                                     hipStream_t stream);
template <typename W>
int bfv_inner_product_shared(const he_bfv_context* ctx, uint32_t moduli_count, const W* lhs, const W* rhs, size_t count,
                             size_t items, W* out, hipStream_t stream);
template <typename W>
int bfv_relinearize(const he_bfv_context* ctx, uint32_t moduli_count, const W* ct3, const W* key, W* out, size_t batch,
                    void* workspace, size_t workspace_bytes, hipStream_t stream);
// Whether a PIR response hands its dim-0 inner products on in Eval form (pir_api.cpp): the first remaining dimension then
// reads them through bfv_inner_product_shared_eval_rhs (api_internal.hpp), which exists for 8-byte words.
template <typename W>
constexpr bool kDim0ResultsStayEval = sizeof(W) == 8;

}  // namespace heamd
