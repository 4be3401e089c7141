// encrypt_api.cpp -- the entry points that MAKE secret keys, ciphertexts and evaluation keys on the device (reference
// Sources/HomomorphicEncryption/Bfv/Bfv+Encrypt.swift, Bfv+Keys.swift, PolyRq/PolyRq+Randomize.swift).  Every random
// polynomial is a function of a caller-supplied 32-byte seed through NistAes128Ctr(seed:); the library generates no seed.
// Each entry is a short pipeline of kernels on the caller's stream: the re-key chains of its seeds (aes_ctr_drbg.hpp), the
// samplers and element-wise steps of encrypt_kernels.hip, and the transforms.  Whatever the workspace held that depends on
// a secret is overwritten with zeros on the stream before it is released (the reference zeroizes errorPoly and currentKey).
// Shared with the other entries that take the slab word: the first checks and the word dispatch (word_layer.hpp), the parts of a
// workspace (workspace_layout.hpp) and its zeroing (zeroized_workspace.hpp).
#include <vector>

#include "aes_ctr_drbg.hpp"
#include "api_internal.hpp"
#include "bfv_context.hpp"
#include "encrypt_kernels.hpp"
#include "kernels.hpp"
#include "rns_kernels.hpp"
#include "word_layer.hpp"
#include "workspace_layout.hpp"
#include "zeroized_workspace.hpp"

using heamd::as_stream;
using heamd::BfvContext;
using heamd::DeviceContext;
using heamd::invalid_argument;
using heamd::KeySwitchFactors;
using heamd::PolyContext;
using heamd::Scratch;
using heamd::ZeroizedWorkspace;

extern "C++" {
namespace {

// the secret-key context: every coefficient modulus (Context.swift:128-131)
const PolyContext& secret_key_context(const BfvContext& bfv) {
    return bfv.has_key_switching() ? *bfv.key_switching(bfv.top_level()) : *bfv.ciphertext(bfv.top_level());
}

// Where the parts of a workspace lie, in bytes from its start, in the order a WorkspaceLayout is given them.  The DRBG records
// of the `a` seeds (public) lie at 0.
struct EncryptPlan {
    size_t error_chain = 0;    // the DRBG records of the error seeds
    size_t error_polys = 0;    // [count][m][N] words: e, then NTT(e) (Eval output only)
    size_t current_keys = 0;   // [keys][L + 1][N] words: s s or the rotated keys
    size_t total = 0;
};
EncryptPlan plan_encrypt_zero(const PolyContext& pc, uint32_t m, bool eval_out, size_t count, size_t word_bytes,
                              size_t current_key_bytes = 0) {
    heamd::WorkspaceLayout layout;
    EncryptPlan plan;
    layout.add(heamd::seeded_uniform_scratch_bytes(pc.device_context(m), count));
    plan.error_chain = layout.add(count * heamd::binomial_chunks(pc.degree()) * heamd::kChainRecordBytes);
    plan.error_polys = layout.add(eval_out ? count * m * pc.degree() * word_bytes : 0);
    plan.current_keys = layout.add(current_key_bytes);
    plan.total = layout.total();
    return plan;
}
EncryptPlan plan_key_switch_keys(const BfvContext& bfv, size_t keys, bool own_current_keys, size_t word_bytes) {
    const PolyContext& pc = secret_key_context(bfv);
    return plan_encrypt_zero(pc, pc.moduli_count(), true, keys * bfv.top_level(), word_bytes,
                             own_current_keys ? keys * pc.moduli_count() * pc.degree() * word_bytes : 0);
}
size_t secret_keys_bytes(const PolyContext& pc, size_t batch) {  // generateSecretKey: the DRBG records of the key seeds alone
    return heamd::round16(batch * heamd::ternary_chunks(pc.degree()) * heamd::kChainRecordBytes);
}

// The checks every entry makes, in this order: the word, the context, the word against the scheme (word_layer.hpp), and (key
// generation) supportsEvaluationKey -- argument errors first, so that they are the same with and without a device --, then the
// device and the transform: nothing is enqueued when any of them fails.
int check_encrypt_context(const he_bfv_context* ctx, uint32_t word_bits, bool needs_evaluation_key, const BfvContext** out) {
    HEAMD_TRY_STATUS(heamd::check_word_and_context(ctx, word_bits));
    const BfvContext& bfv = heamd::bfv_impl(ctx);
    if (needs_evaluation_key && !bfv.has_key_switching()) {
        heamd::set_last_error("a context with one coefficient modulus supports no evaluation key");
        return HE_ERR_UNSUPPORTED;  // Bfv+Keys.swift:35-37
    }
    *out = &bfv;
    return HE_OK;
}
int check_encrypt_device(const BfvContext& bfv, uint32_t word_bits, uint32_t moduli) {
    if (bfv.host_only()) return heamd::host_only_refusal();
    const PolyContext& pc = secret_key_context(bfv);
    HEAMD_TRY_STATUS(pc.check_device());
    if (!pc.all_ntt(moduli)) return HE_ERR_INVALID_NTT_MODULUS;
    if (word_bits == 32) {
        if (pc.degree() > 32768) {  // the 4-byte launch_ntt holds a row in the LDS
            heamd::set_last_error("UInt32 transform supports degrees up to 32768");
            return HE_ERR_UNSUPPORTED;
        }
        heamd::DeviceContext32 image{};
        HEAMD_TRY_STATUS(pc.device_context32(moduli, image));
    }
    return HE_OK;
}

// Bfv.encryptZero over the first m moduli of pc for `count` ciphertexts, out [count][2][m][N]; with current_keys the last step
// of _generateKeySwitchKey on top (encrypt_kernels.hpp launch_encrypt_finish_eval).  `ws`: a workspace laid out by `plan`.
template <typename W>
int encrypt_zero_pipeline(const PolyContext& pc, uint32_t m, bool eval_out, const W* secret_key, const uint8_t* a_seeds,
                          const uint8_t* error_seeds, W* out, size_t count, const W* current_keys, uint32_t per_key,
                          const KeySwitchFactors& factors, const ZeroizedWorkspace& ws, const EncryptPlan& plan,
                          hipStream_t stream) {
    const DeviceContext dc = pc.device_context(m);
    const size_t poly_words = size_t(m) * pc.degree();
    uint32_t* error_chain = ws.at<uint32_t>(plan.error_chain);
    // `a` is drawn in Eval form directly (Bfv+Encrypt.swift:155-156), into polynomial 1 of every ciphertext
    HEAMD_HIP_TRY(heamd::launch_seeded_uniform(a_seeds, out + poly_words, 2 * poly_words, dc, count, ws.at(0), stream));
    HEAMD_HIP_TRY(heamd::launch_seeded_chain(error_seeds, error_chain, count, heamd::binomial_chunks(pc.degree()), stream));
    if (eval_out) {
        W* error = ws.at<W>(plan.error_polys);
        HEAMD_HIP_TRY(heamd::launch_sample_centered_binomial(error_chain, error, poly_words, dc, count, stream));
        HEAMD_HIP_TRY(heamd::ntt_rows(false, error, pc, dc, m, count * m, stream));
        HEAMD_HIP_TRY(heamd::launch_encrypt_finish_eval(out, error, secret_key, current_keys, per_key, factors, dc, count, stream));
        return HE_OK;
    }
    // one inverse transform over the whole slab: both polynomials need it.  Until the finish kernel has run, polynomial 0 of the
    // caller's slab holds a s: a failure on the way clears the slab instead of leaving that behind
    hipError_t status = heamd::launch_encrypt_mul_secret(out, secret_key, dc, count, stream);
    if (status == hipSuccess) status = heamd::ntt_rows(true, out, pc, dc, m, count * 2 * m, stream);
    if (status == hipSuccess) status = heamd::launch_encrypt_finish_coeff(out, error_chain, dc, count, stream);
    if (status != hipSuccess) {
        (void)hipGetLastError();
        (void)hipMemsetAsync(out, 0, count * 2 * poly_words * sizeof(W), stream);
    }
    HEAMD_HIP_TRY(status);
    return HE_OK;
}

template <typename W>
int encrypt_zero_entry(const BfvContext& bfv, uint32_t m, bool eval_out, const void* secret_key, const uint8_t* a_seeds,
                       const uint8_t* error_seeds, const void* plaintexts, void* out, size_t batch, void* workspace,
                       size_t workspace_bytes, hipStream_t stream) {
    const PolyContext& pc = secret_key_context(bfv);
    const EncryptPlan plan = plan_encrypt_zero(pc, m, eval_out, batch, sizeof(W));
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(ws.resolve(workspace, workspace_bytes, plan.total));
    HEAMD_TRY_STATUS(encrypt_zero_pipeline<W>(pc, m, eval_out, static_cast<const W*>(secret_key), a_seeds, error_seeds,
                                              static_cast<W*>(out), batch, nullptr, 0, KeySwitchFactors{}, ws, plan, stream));
    if (plaintexts != nullptr)  // Bfv.encrypt: addAssign(&ciphertext, plaintext) (Bfv+Encrypt.swift:70)
        HEAMD_HIP_TRY(heamd::launch_plaintext_translate(static_cast<W*>(out), static_cast<const W*>(plaintexts),
                                                        bfv.tool(m)->device, 2, false, batch, stream));
    return HE_OK;
}

// modulus.reduce(keyModulus) as a MultiplyConstantModulus per ciphertext modulus (Bfv+Keys.swift:88-91)
void key_switch_factors(const BfvContext& bfv, KeySwitchFactors& factors) {
    const std::vector<heamd::u64>& q = secret_key_context(bfv).moduli();
    const heamd::u64 q_ks = q.back();
    for (uint32_t j = 0; j < bfv.top_level(); ++j) {
        const heamd::u64 factor = q_ks % q[j];
        factors.factor[j] = heamd::U64x2{factor, heamd::shoup_factor(factor, q[j])};
    }
}

enum class CurrentKeys { Callers, Square, Galois };

// Bfv._generateKeySwitchKey for `keys` current keys: the caller's, s s, or applyGalois(s, elements[k])
template <typename W>
int key_switch_keys_entry(const BfvContext& bfv, CurrentKeys kind, const void* secret_key, const void* current_keys,
                          const uint64_t* elements, const uint8_t* a_seeds, const uint8_t* error_seeds, void* out, size_t keys,
                          void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const PolyContext& pc = secret_key_context(bfv);
    const uint32_t L = bfv.top_level(), m = pc.moduli_count();
    const EncryptPlan plan = plan_key_switch_keys(bfv, keys, kind != CurrentKeys::Callers, sizeof(W));
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(ws.resolve(workspace, workspace_bytes, plan.total));
    const W* s = static_cast<const W*>(secret_key);
    const W* current = static_cast<const W*>(current_keys);
    if (kind != CurrentKeys::Callers) {
        const DeviceContext dc = pc.device_context();
        W* own = ws.at<W>(plan.current_keys);
        if (kind == CurrentKeys::Square)  // (one key)
            HEAMD_HIP_TRY(heamd::launch_secret_key_square(s, own, dc, stream));
        else  // all rotated keys in one launch (64 elements travel in a launch's arguments)
            HEAMD_HIP_TRY(heamd::launch_secret_key_galois(s, own, dc, elements, keys, stream));
        current = own;
    }
    KeySwitchFactors factors{};
    key_switch_factors(bfv, factors);
    return encrypt_zero_pipeline<W>(pc, m, true, s, a_seeds, error_seeds, static_cast<W*>(out), keys * L, current, L, factors, ws,
                                    plan, stream);
}

int check_key_generation(const he_bfv_context* ctx, uint32_t word_bits, const BfvContext** bfv) {
    HEAMD_TRY_STATUS(check_encrypt_context(ctx, word_bits, true, bfv));
    if ((*bfv)->top_level() > heamd::kMaxKeySwitchCiphertexts) {
        heamd::set_last_error("more than 32 ciphertext moduli are not supported by key generation");
        return HE_ERR_UNSUPPORTED;
    }
    return HE_OK;
}

// The pointer contract of the entries that encrypt `count` zeros over m moduli of pc (he_amd.h): out and a caller's workspace are
// written; the secret key, the seeds ([count][32] each) and the plaintexts or current keys (`extra`) are only read and may lie
// anywhere but in those two.
int check_encrypt_slabs(const char* what, const PolyContext& pc, uint32_t m, size_t word_bytes, const void* secret_key,
                        const uint8_t* a_seeds, const uint8_t* error_seeds, heamd::Slab extra, const void* out, size_t count,
                        const void* workspace, size_t workspace_bytes) {
    const size_t row = size_t(pc.degree()) * word_bytes;
    return heamd::check_slabs(what, {{"out", out, count * 2 * m * row, true},
                                     {"workspace", workspace, workspace_bytes, true},
                                     {"secret_key", secret_key, m * row, false},
                                     {"a_seeds", a_seeds, count * 32, false},
                                     {"error_seeds", error_seeds, count * 32, false},
                                     extra});
}

// What the three key generators share behind their own checks: null buffers, the pointer contract (the secret key may itself be a
// current key: both are only read), the device, and the pipeline for the slab word.  current_keys: the caller's, or NULL
int generate_key_switch_keys(const BfvContext& bfv, uint32_t word_bits, CurrentKeys kind, const char* what, const void* secret_key,
                             const void* current_keys, const uint64_t* elements, const uint8_t* a_seeds, const uint8_t* error_seeds,
                             void* out, size_t keys, void* workspace, size_t workspace_bytes, he_stream s) {
    if (secret_key == nullptr || (kind == CurrentKeys::Callers && current_keys == nullptr) || a_seeds == nullptr ||
        error_seeds == nullptr || out == nullptr)
        return invalid_argument("null keys or seeds");
    const PolyContext& pc = secret_key_context(bfv);
    const size_t key_bytes = size_t(pc.moduli_count()) * pc.degree() * (word_bits / 8);  // (a NULL slab takes part in nothing)
    HEAMD_TRY_STATUS(check_encrypt_slabs(what, pc, pc.moduli_count(), word_bits / 8, secret_key, a_seeds, error_seeds,
                                         {"current_keys", current_keys, keys * key_bytes, false}, out, keys * bfv.top_level(),
                                         workspace, workspace_bytes));
    HEAMD_TRY_STATUS(check_encrypt_device(bfv, word_bits, bfv.top_level() + 1));
    return heamd::with_word(word_bits, [&](auto word) {
        return key_switch_keys_entry<decltype(word)>(bfv, kind, secret_key, current_keys, elements, a_seeds, error_seeds, out, keys,
                                                     workspace, workspace_bytes, as_stream(s));
    });
}

int check_moduli_fit_word(const PolyContext& pc, uint32_t word_bits) {
    if (word_bits == 64) return HE_OK;
    for (heamd::u64 q : pc.moduli())
        if (q > ((uint64_t(1) << 30) - 1)) {
            heamd::set_last_error("modulus " + std::to_string(q) + " does not fit UInt32 (max 2^30 - 1)");
            return HE_ERR_INVALID_MODULUS;
        }
    return HE_OK;
}

// the polynomial-level samplers: chain, sample, zeroize the chain
template <typename W>
int poly_sample(const PolyContext& pc, bool ternary, const uint8_t* seeds, size_t batch, W* out, hipStream_t stream) {
    const uint32_t chunks = ternary ? heamd::ternary_chunks(pc.degree()) : heamd::binomial_chunks(pc.degree());
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(ws.resolve(nullptr, 0, batch * chunks * heamd::kChainRecordBytes));
    uint32_t* chain = ws.at<uint32_t>(0);
    HEAMD_HIP_TRY(heamd::launch_seeded_chain(seeds, chain, batch, chunks, stream));
    const size_t poly_words = size_t(pc.moduli_count()) * pc.degree();
    if (ternary)
        HEAMD_HIP_TRY(heamd::launch_sample_ternary(chain, out, poly_words, pc.device_context(), batch, stream));
    else
        HEAMD_HIP_TRY(heamd::launch_sample_centered_binomial(chain, out, poly_words, pc.device_context(), batch, stream));
    return HE_OK;
}
int poly_sample_entry(const he_poly_context* ctx, uint32_t word_bits, bool ternary, const uint8_t* seeds, size_t batch,
                      void* out, he_stream s) {
    HEAMD_TRY_STATUS(heamd::check_word_bits(word_bits));
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    HEAMD_TRY_STATUS(check_moduli_fit_word(pc, word_bits));
    if (batch == 0) return HE_OK;
    if (seeds == nullptr || out == nullptr) return invalid_argument("null buffer");
    HEAMD_TRY_STATUS(heamd::check_slabs(ternary ? "randomizeTernary" : "randomizeCenteredBinomialDistribution",
                                        {{"out", out, batch * pc.moduli_count() * pc.degree() * (word_bits / 8), true},
                                         {"seeds", seeds, batch * 32, false}}));
    HEAMD_TRY_STATUS(pc.check_device());
    return heamd::with_word(word_bits, [&](auto word) {
        return poly_sample(pc, ternary, seeds, batch, static_cast<decltype(word)*>(out), as_stream(s));
    });
}

}  // namespace

int heamd::bfv_encrypt_check_device(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count) {
    return check_encrypt_device(heamd::bfv_impl(ctx), word_bits, moduli_count);
}
}  // extern "C++"

size_t he_bfv_encrypt_workspace_bytes(const he_bfv_context* ctx, uint32_t word_bits, int operation, uint32_t moduli_count,
                                      int eval_out, size_t count) {
    if (ctx == nullptr || (word_bits != 32 && word_bits != 64)) return 0;
    const BfvContext& bfv = heamd::bfv_impl(ctx);
    const PolyContext& pc = secret_key_context(bfv);
    const size_t word_bytes = word_bits / 8;
    switch (operation) {
        case HE_ENCRYPT_OP_SECRET_KEY:
            return secret_keys_bytes(pc, count);
        case HE_ENCRYPT_OP_ENCRYPT_ZERO:
            if (moduli_count < 1 || moduli_count > pc.moduli_count()) return 0;
            return plan_encrypt_zero(pc, moduli_count, eval_out != 0, count, word_bytes).total;
        case HE_ENCRYPT_OP_ENCRYPT:
            if (!bfv.valid(moduli_count)) return 0;
            return plan_encrypt_zero(pc, moduli_count, false, count, word_bytes).total;
        case HE_ENCRYPT_OP_KEY_SWITCH_KEYS:
        case HE_ENCRYPT_OP_RELINEARIZATION_KEY:
        case HE_ENCRYPT_OP_GALOIS_KEYS:
            if (!bfv.has_key_switching()) return 0;
            return plan_key_switch_keys(bfv, operation == HE_ENCRYPT_OP_RELINEARIZATION_KEY ? 1 : count,
                                        operation != HE_ENCRYPT_OP_KEY_SWITCH_KEYS, word_bytes)
                .total;
        default:
            return 0;
    }
}

int he_bfv_generate_secret_key_device(const he_bfv_context* ctx, uint32_t word_bits, const uint8_t* seeds, void* out,
                                      size_t batch, void* workspace, size_t workspace_bytes, he_stream s) {
    const BfvContext* bfv = nullptr;
    HEAMD_TRY_STATUS(check_encrypt_context(ctx, word_bits, false, &bfv));
    if (batch == 0) return HE_OK;
    if (seeds == nullptr || out == nullptr) return invalid_argument("null seeds or keys");
    const PolyContext& pc = secret_key_context(*bfv);
    HEAMD_TRY_STATUS(heamd::check_slabs(
        "generateSecretKey", {{"out", out, batch * pc.moduli_count() * pc.degree() * (word_bits / 8), true},
                              {"workspace", workspace, workspace_bytes, true},
                              {"seeds", seeds, batch * 32, false}}));
    HEAMD_TRY_STATUS(check_encrypt_device(*bfv, word_bits, pc.moduli_count()));
    const hipStream_t stream = as_stream(s);
    ZeroizedWorkspace ws(stream);
    HEAMD_TRY_STATUS(ws.resolve(workspace, workspace_bytes, secret_keys_bytes(pc, batch)));
    uint32_t* chain = ws.at<uint32_t>(0);
    HEAMD_HIP_TRY(heamd::launch_seeded_chain(seeds, chain, batch, heamd::ternary_chunks(pc.degree()), stream));
    const DeviceContext dc = pc.device_context();
    const size_t poly_words = size_t(pc.moduli_count()) * pc.degree(), rows = batch * pc.moduli_count();
    return heamd::with_word(word_bits, [&](auto word) {
        auto* keys = static_cast<decltype(word)*>(out);
        HEAMD_HIP_TRY(heamd::launch_sample_ternary(chain, keys, poly_words, dc, batch, stream));
        HEAMD_HIP_TRY(heamd::ntt_rows(false, keys, pc, dc, pc.moduli_count(), rows, stream));
        return int(HE_OK);
    });
}

int he_bfv_encrypt_zero_device(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, int eval_out,
                               const void* secret_key, const uint8_t* a_seeds, const uint8_t* error_seeds, void* out,
                               size_t batch, void* workspace, size_t workspace_bytes, he_stream s) {
    const BfvContext* bfv = nullptr;
    HEAMD_TRY_STATUS(check_encrypt_context(ctx, word_bits, false, &bfv));
    if (moduli_count < 1 || moduli_count > secret_key_context(*bfv).moduli_count())
        return invalid_argument("moduli_count out of range");
    if (batch == 0) return HE_OK;
    if (secret_key == nullptr || a_seeds == nullptr || error_seeds == nullptr || out == nullptr)
        return invalid_argument("null secret key, seeds or ciphertexts");
    HEAMD_TRY_STATUS(check_encrypt_slabs("encryptZero", secret_key_context(*bfv), moduli_count, word_bits / 8, secret_key, a_seeds,
                                         error_seeds, {"", nullptr, 0, false}, out, batch, workspace, workspace_bytes));
    HEAMD_TRY_STATUS(check_encrypt_device(*bfv, word_bits, moduli_count));
    return heamd::with_word(word_bits, [&](auto word) {
        return encrypt_zero_entry<decltype(word)>(*bfv, moduli_count, eval_out != 0, secret_key, a_seeds, error_seeds, nullptr, out,
                                                  batch, workspace, workspace_bytes, as_stream(s));
    });
}

int he_bfv_encrypt_device(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, const void* secret_key,
                          const uint8_t* a_seeds, const uint8_t* error_seeds, const void* plaintexts, void* out, size_t batch,
                          void* workspace, size_t workspace_bytes, he_stream s) {
    const BfvContext* bfv = nullptr;
    HEAMD_TRY_STATUS(check_encrypt_context(ctx, word_bits, false, &bfv));
    if (!bfv->valid(moduli_count)) return invalid_argument("moduli_count out of range");
    if (batch == 0) return HE_OK;
    if (secret_key == nullptr || a_seeds == nullptr || error_seeds == nullptr || plaintexts == nullptr || out == nullptr)
        return invalid_argument("null secret key, seeds, plaintexts or ciphertexts");
    HEAMD_TRY_STATUS(check_encrypt_slabs("encrypt", secret_key_context(*bfv), moduli_count, word_bits / 8, secret_key, a_seeds,
                                         error_seeds, {"plaintexts", plaintexts, batch * bfv->degree() * (word_bits / 8), false}, out,
                                         batch, workspace, workspace_bytes));
    HEAMD_TRY_STATUS(check_encrypt_device(*bfv, word_bits, moduli_count));
    return heamd::with_word(word_bits, [&](auto word) {
        return encrypt_zero_entry<decltype(word)>(*bfv, moduli_count, false, secret_key, a_seeds, error_seeds, plaintexts, out, batch,
                                                  workspace, workspace_bytes, as_stream(s));
    });
}

int he_bfv_generate_key_switch_keys_device(const he_bfv_context* ctx, uint32_t word_bits, const void* secret_key,
                                           const void* current_keys, const uint8_t* a_seeds, const uint8_t* error_seeds,
                                           void* out, size_t keys, void* workspace, size_t workspace_bytes, he_stream s) {
    const BfvContext* bfv = nullptr;
    HEAMD_TRY_STATUS(check_key_generation(ctx, word_bits, &bfv));
    if (keys == 0) return HE_OK;
    return generate_key_switch_keys(*bfv, word_bits, CurrentKeys::Callers, "generateKeySwitchKey", secret_key, current_keys, nullptr,
                                    a_seeds, error_seeds, out, keys, workspace, workspace_bytes, s);
}

int he_bfv_generate_relinearization_key_device(const he_bfv_context* ctx, uint32_t word_bits, const void* secret_key,
                                               const uint8_t* a_seeds, const uint8_t* error_seeds, void* out, void* workspace,
                                               size_t workspace_bytes, he_stream s) {
    const BfvContext* bfv = nullptr;
    HEAMD_TRY_STATUS(check_key_generation(ctx, word_bits, &bfv));
    return generate_key_switch_keys(*bfv, word_bits, CurrentKeys::Square, "generateRelinearizationKey", secret_key, nullptr, nullptr,
                                    a_seeds, error_seeds, out, 1, workspace, workspace_bytes, s);
}

int he_bfv_generate_galois_keys_device(const he_bfv_context* ctx, uint32_t word_bits, const void* secret_key,
                                       const uint64_t* elements, size_t count, const uint8_t* a_seeds,
                                       const uint8_t* error_seeds, void* out, void* workspace, size_t workspace_bytes,
                                       he_stream s) {
    const BfvContext* bfv = nullptr;
    HEAMD_TRY_STATUS(check_key_generation(ctx, word_bits, &bfv));
    if (count != 0 && elements == nullptr) return invalid_argument("null elements");
    // isValidGaloisElement (Galois.swift:100-105), as he_bfv_apply_galois_device answers it
    for (size_t k = 0; k < count; ++k)
        if ((elements[k] & 1) == 0 || elements[k] <= 1 || elements[k] >= 2 * uint64_t(bfv->degree()))
            return invalid_argument("invalid Galois element");
    if (count == 0) return HE_OK;
    return generate_key_switch_keys(*bfv, word_bits, CurrentKeys::Galois, "generateGaloisKeys", secret_key, nullptr, elements, a_seeds,
                                    error_seeds, out, count, workspace, workspace_bytes, s);
}

int he_poly_random_ternary_from_seeds_device(const he_poly_context* ctx, uint32_t word_bits, const uint8_t* seeds, size_t batch,
                                             void* out, he_stream s) {
    return poly_sample_entry(ctx, word_bits, true, seeds, batch, out, s);
}
int he_poly_random_centered_binomial_from_seeds_device(const he_poly_context* ctx, uint32_t word_bits, const uint8_t* seeds,
                                                       size_t batch, void* out, he_stream s) {
    return poly_sample_entry(ctx, word_bits, false, seeds, batch, out, s);
}
