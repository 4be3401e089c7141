// c_api.cpp -- the extern "C" boundary declared in include/he_amd.h.
#include "../../include/he_amd.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "api_internal.hpp"
#include "ciphertext_wire_form.hpp"
#include "kernels.hpp"
#include "poly_context.hpp"
#include "serialize_form.hpp"
#include "word_layer.hpp"

using heamd::as_stream;
using heamd::check_word_device;
using heamd::invalid_argument;
using heamd::kChecksDeviceFirst;
using heamd::PolyContext;
using heamd::Scratch;

namespace {

// Runs `body(device_ptr, stream)` on a device copy of a host slab and copies the result back (blocking).
template <typename Body>
int with_device_copy(uint64_t* host, size_t words, Body body) {
    hipStream_t stream = hipStreamPerThread;
    void* device = nullptr;
    HEAMD_HIP_TRY(hipMalloc(&device, words * sizeof(uint64_t) + 16));
    int status = HE_OK;
    hipError_t e = hipMemcpyAsync(device, host, words * sizeof(uint64_t), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        status = body(static_cast<uint64_t*>(device), stream);
        if (status == HE_OK) e = hipMemcpyAsync(host, device, words * sizeof(uint64_t), hipMemcpyDeviceToHost, stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(device);
    if (status != HE_OK) return status;
    if (e != hipSuccess) return heamd::device_failure(e, "host-pointer round trip");
    return HE_OK;
}

int ntt_rows_device(const he_poly_context* ctx, uint64_t modulus, uint64_t* rows_ptr, size_t rows, bool inverse,
                    hipStream_t stream) {
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    // PolyContext.forwardNtt(dataPtr:modulus:) walks the chain for a context whose last modulus matches and
    // throws invalidPolyContext otherwise, or when that context has no nttContext (PolyRq+Ntt.swift:329-341).
    const int index = pc.modulus_index(modulus);
    if (index < 0 || !pc.host_constants()[index].has_ntt) {
        heamd::set_last_error("modulus " + std::to_string(modulus) + " has no NTT context in this PolyContext");
        return HE_ERR_INVALID_POLY_CONTEXT;
    }
    if (rows == 0) return HE_OK;
    if (rows_ptr == nullptr) return invalid_argument("null rows");
    int status = pc.check_device();
    if (status != HE_OK) return status;
    heamd::DeviceContext dc = pc.device_context();
    dc.approx_ok = modulus < (uint64_t(1) << 61) ? 1 : 0;
    dc.headroom_ok = (modulus < (uint64_t(1) << 55) && modulus >= (uint64_t(1) << 40)) ? 1 : 0;
    HEAMD_HIP_TRY(heamd::launch_ntt(inverse, rows_ptr, dc, static_cast<uint32_t>(index), 1, rows, stream));
    return HE_OK;
}

}  // namespace

// forwardNtt(poly:) / inverseNtt(poly:) on slabs of either word
template <typename W>
int heamd::poly_ntt(const he_poly_context* ctx, W* slab, size_t batch, bool inverse, hipStream_t stream) {
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    // validateNttModuli (PolyContext.swift:175-181) comes first in forwardNtt(poly:) / inverseNtt(poly:)
    if (!pc.all_ntt(pc.moduli_count())) {
        if (sizeof(W) == 8)  // (the 4-byte entries return the status alone)
            set_last_error("a modulus of this context is not an NTT modulus for degree " + std::to_string(pc.degree()));
        return HE_ERR_INVALID_NTT_MODULUS;
    }
    if (kChecksDeviceFirst<W>) HEAMD_TRY_STATUS(check_word_device<W>(pc));
    if (batch == 0) return HE_OK;
    if (slab == nullptr) return invalid_argument("null slab");
    if (!kChecksDeviceFirst<W>) HEAMD_TRY_STATUS(check_word_device<W>(pc));
    const hipError_t e = ntt_rows(inverse, slab, pc, pc.device_context(), pc.moduli_count(), batch * pc.moduli_count(), stream);
    if (sizeof(W) == 4 && e == hipErrorNotSupported) {  // the 4-byte launch_ntt holds a row in the LDS
        set_last_error("UInt32 transform supports degrees up to 32768");
        return HE_ERR_UNSUPPORTED;
    }
    HEAMD_HIP_TRY(e);
    return HE_OK;
}
template int heamd::poly_ntt(const he_poly_context*, uint64_t*, size_t, bool, hipStream_t);
template int heamd::poly_ntt(const he_poly_context*, uint32_t*, size_t, bool, hipStream_t);

template <typename W>
int heamd::poly_elementwise(const he_poly_context* ctx, ElementwiseOp op, W* lhs, const W* rhs, size_t batch,
                            hipStream_t stream) {
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    if (kChecksDeviceFirst<W>) HEAMD_TRY_STATUS(check_word_device<W>(pc));
    if (batch == 0) return HE_OK;
    if (lhs == nullptr || (rhs == nullptr && op != ElementwiseOp::Neg)) return invalid_argument("null slab");
    {
        // a lane reads lhs[k] and rhs[k] and writes lhs[k]: rhs may be lhs itself (x + x, x - x, x * x), no other overlap
        const size_t bytes = batch * pc.moduli_count() * pc.degree() * sizeof(W);
        HEAMD_TRY_STATUS(heamd::check_slabs("element-wise", {{"lhs", lhs, bytes, true}, {"rhs", rhs, bytes, false}}, {0, 1}));
    }
    if (!kChecksDeviceFirst<W>) HEAMD_TRY_STATUS(check_word_device<W>(pc));
    HEAMD_HIP_TRY(elementwise_rows(op, lhs, rhs, nullptr, pc, batch * pc.moduli_count(), stream));
    return HE_OK;
}
template int heamd::poly_elementwise(const he_poly_context*, heamd::ElementwiseOp, uint64_t*, const uint64_t*, size_t,
                                     hipStream_t);
template int heamd::poly_elementwise(const he_poly_context*, heamd::ElementwiseOp, uint32_t*, const uint32_t*, size_t,
                                     hipStream_t);

namespace {
// MultiplyConstantModulus(multiplicand:divisionModulus:) per row (PolyRq.swift:235-238)
template <typename W>
int poly_mul_scalar(const he_poly_context* ctx, W* data, const W* scalar_residues, size_t batch, he_stream s) {
    if (ctx == nullptr || scalar_residues == nullptr) return invalid_argument("null pointer");
    const PolyContext& pc = *ctx->impl;
    if (kChecksDeviceFirst<W>) HEAMD_TRY_STATUS(check_word_device<W>(pc));
    if (batch == 0) return HE_OK;
    if (sizeof(W) == 4 && data == nullptr) return invalid_argument("null slab");  // (the 8-byte entry takes its slab unchecked)
    if (!kChecksDeviceFirst<W>) HEAMD_TRY_STATUS(check_word_device<W>(pc));
    std::vector<heamd::U64x2> pairs(pc.moduli_count());
    for (uint32_t i = 0; i < pc.moduli_count(); ++i) {
        const uint64_t p = pc.moduli()[i];
        if (scalar_residues[i] >= p) return invalid_argument("scalar residue not reduced");
        pairs[i] = heamd::U64x2{scalar_residues[i], heamd::shoup_factor(scalar_residues[i], p)};
    }
    hipStream_t stream = as_stream(s);
    Scratch scratch(stream);
    HEAMD_HIP_TRY(scratch.allocate(pairs.size() * sizeof(heamd::U64x2)));
    HEAMD_HIP_TRY(hipMemcpyAsync(scratch.get(), pairs.data(), pairs.size() * sizeof(heamd::U64x2),
                                 hipMemcpyHostToDevice, stream));
    HEAMD_HIP_TRY(hipStreamSynchronize(stream));  // the pageable host vector must outlive the async copy
    HEAMD_HIP_TRY(heamd::elementwise_rows<W>(heamd::ElementwiseOp::MulScalar, data, nullptr,
                                             static_cast<const uint64_t*>(scratch.get()), pc, batch * pc.moduli_count(), stream));
    return HE_OK;
}

template <typename W>
int poly_divide_and_round_q_last(const he_poly_context* ctx, const W* in, W* out, size_t batch, he_stream s) {
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    if (pc.moduli_count() < 2) return HE_ERR_INVALID_POLY_CONTEXT;  // no next context (PolyRq.swift:366-368)
    if (kChecksDeviceFirst<W>) HEAMD_TRY_STATUS(check_word_device<W>(pc));
    if (batch == 0) return HE_OK;
    if (in == nullptr || out == nullptr) return invalid_argument("null slab");
    {
        // polynomial p reads rows p L .. p L + L - 1 and writes rows p (L - 1) ..: in place, what one polynomial stores is
        // what an earlier one still reads, in no particular order
        const size_t row = batch * pc.degree() * sizeof(W);
        HEAMD_TRY_STATUS(heamd::check_slabs("divideAndRoundQLast", {{"out", out, row * (pc.moduli_count() - 1), true},
                                                                    {"in", in, row * pc.moduli_count(), false}}));
    }
    if (!kChecksDeviceFirst<W>) HEAMD_TRY_STATUS(check_word_device<W>(pc));
    HEAMD_HIP_TRY(divide_and_round_q_last(in, out, pc, pc.moduli_count(), batch, as_stream(s)));
    return HE_OK;
}
}  // namespace

extern "C" {

const char* he_status_string(int status) {
    switch (status) {
        case HE_OK: return "ok";
        case HE_ERR_INVALID_DEGREE: return "invalidDegree";
        case HE_ERR_INVALID_MODULUS: return "invalidModulus";
        case HE_ERR_COPRIME_MODULI: return "coprimeModuli";
        case HE_ERR_EMPTY_MODULUS: return "emptyModulus";
        case HE_ERR_INVALID_NTT_MODULUS: return "invalidNttModulus";
        case HE_ERR_INVALID_POLY_CONTEXT: return "invalidPolyContext";
        case HE_ERR_POLY_CONTEXT_MISMATCH: return "polyContextMismatch";
        case HE_ERR_INVALID_CIPHERTEXT: return "invalidCiphertext";
        case HE_ERR_INCOMPATIBLE_CIPHERTEXTS: return "incompatibleCiphertexts";
        case HE_ERR_INCOMPATIBLE_CIPHERTEXT_AND_PLAINTEXT: return "incompatibleCiphertextAndPlaintext";
        case HE_ERR_MISSING_RELINEARIZATION_KEY: return "missingRelinearizationKey";
        case HE_ERR_UNEQUAL_CONTEXTS: return "unequalContexts";
        case HE_ERR_NOT_ENOUGH_PRIMES: return "notEnoughPrimes";
        case HE_ERR_NOT_INVERTIBLE: return "notInvertible";
        case HE_ERR_INVALID_ENCRYPTION_PARAMETERS: return "invalidEncryptionParameters";
        case HE_ERR_INVALID_ARGUMENT: return "invalidArgument";
        case HE_ERR_DEVICE: return "deviceError";
        case HE_ERR_UNSUPPORTED: return "unsupportedHeOperation";
        case HE_ERR_MISSING_GALOIS_KEY: return "missingGaloisKey";
        case HE_ERR_SERIALIZED_BUFFER_SIZE_MISMATCH: return "serializedBufferSizeMismatch";
        case HE_ERR_INVALID_COEFFICIENT_PACKING: return "invalidCoefficientPacking";
        case HE_ERR_SIMD_ENCODING_NOT_SUPPORTED: return "simdEncodingNotSupported";
        case HE_ERR_INVALID_DATABASE_SERIALIZATION_VERSION: return "invalidDatabaseSerializationVersion";
        case HE_ERR_INVALID_DATABASE_SERIALIZATION_PLAINTEXT_TAG: return "invalidDatabaseSerializationPlaintextTag";
        case HE_ERR_FAILED_TO_CONSTRUCT_CUCKOO_TABLE: return "failedToConstructCuckooTable";
        case HE_ERR_INVALID_CUCKOO_CONFIG: return "invalidCuckooConfig";
        case HE_ERR_INVALID_HASH_BUCKET_ENTRY_VALUE_SIZE: return "invalidHashBucketEntryValueSize";
        case HE_ERR_INVALID_HASH_BUCKET_SLOT_COUNT: return "invalidHashBucketSlotCount";
        case HE_ERR_CUCKOO_TABLE_NEEDS_EXPANSION: return "cuckooTableNeedsExpansion";
        case HE_ERR_INVALID_SHARDING: return "invalidSharding";
        default: return "unknown";
    }
}

const char* he_last_error_message(void) { return heamd::last_error(); }
const char* he_version(void) { return "he_amd 0.1 (gfx950, HIP)"; }

int he_device_count(int* out_count) {
    if (out_count == nullptr) return invalid_argument("null out_count");
    *out_count = 0;
    HEAMD_HIP_TRY(hipGetDeviceCount(out_count));
    return HE_OK;
}
int he_get_device(int* out_device) {
    if (out_device == nullptr) return invalid_argument("null out_device");
    HEAMD_HIP_TRY(hipGetDevice(out_device));
    return HE_OK;
}
int he_set_device(int device) {
    HEAMD_HIP_TRY(hipSetDevice(device));
    return HE_OK;
}

int he_device_malloc(void** out_ptr, size_t bytes) {
    if (out_ptr == nullptr) return invalid_argument("null out_ptr");
    *out_ptr = nullptr;
    HEAMD_HIP_TRY(hipMalloc(out_ptr, bytes ? bytes : 1));
    return HE_OK;
}
int he_device_free(void* ptr) {
    heamd::RelaxedCapture relaxed;
    if (ptr == nullptr) return HE_OK;
    HEAMD_HIP_TRY(hipFree(ptr));
    return HE_OK;
}
int he_host_malloc(void** out_ptr, size_t bytes) {
    if (out_ptr == nullptr) return invalid_argument("null out_ptr");
    *out_ptr = nullptr;
    HEAMD_HIP_TRY(hipHostMalloc(out_ptr, bytes ? bytes : 1, hipHostMallocDefault));
    return HE_OK;
}
int he_host_free(void* ptr) {
    heamd::RelaxedCapture relaxed;
    if (ptr == nullptr) return HE_OK;
    HEAMD_HIP_TRY(hipHostFree(ptr));
    return HE_OK;
}
int he_memcpy_h2d(void* dst_device, const void* src_host, size_t bytes, he_stream stream) {
    HEAMD_HIP_TRY(hipMemcpyAsync(dst_device, src_host, bytes, hipMemcpyHostToDevice, as_stream(stream)));
    return HE_OK;
}
int he_memcpy_d2h(void* dst_host, const void* src_device, size_t bytes, he_stream stream) {
    HEAMD_HIP_TRY(hipMemcpyAsync(dst_host, src_device, bytes, hipMemcpyDeviceToHost, as_stream(stream)));
    return HE_OK;
}
int he_stream_synchronize(he_stream stream) {
    HEAMD_HIP_TRY(hipStreamSynchronize(as_stream(stream)));
    return HE_OK;
}
int he_stream_create(he_stream* out) {
    if (out == nullptr) return invalid_argument("null out");
    hipStream_t stream = nullptr;
    HEAMD_HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    *out = stream;
    return HE_OK;
}
int he_stream_destroy(he_stream stream) {
    heamd::RelaxedCapture relaxed;
    if (stream == nullptr) return HE_OK;
    heamd::scratch_forget_stream(as_stream(stream));
    HEAMD_HIP_TRY(hipStreamDestroy(as_stream(stream)));
    return HE_OK;
}

// ---- completion primitives for the reference's `...Async` twins (HeSchemeAsync.swift:16-141): a Swift `async`
// wrapper enqueues the `_device` call and suspends on he_stream_add_callback (or polls / waits on an event) instead of
// blocking a thread of the cooperative pool in he_stream_synchronize.
int he_event_create(he_event* out) {
    if (out == nullptr) return invalid_argument("null out");
    hipEvent_t event = nullptr;
    HEAMD_HIP_TRY(hipEventCreateWithFlags(&event, hipEventDisableTiming));
    *out = event;
    return HE_OK;
}
int he_event_destroy(he_event event) {
    heamd::RelaxedCapture relaxed;
    if (event == nullptr) return HE_OK;
    HEAMD_HIP_TRY(hipEventDestroy(static_cast<hipEvent_t>(event)));
    return HE_OK;
}
int he_event_record(he_event event, he_stream stream) {
    if (event == nullptr) return invalid_argument("null event");
    HEAMD_HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(event), as_stream(stream)));
    return HE_OK;
}
int he_event_synchronize(he_event event) {
    if (event == nullptr) return invalid_argument("null event");
    HEAMD_HIP_TRY(hipEventSynchronize(static_cast<hipEvent_t>(event)));
    return HE_OK;
}
int he_event_query(he_event event, int* out_done) {
    if (event == nullptr || out_done == nullptr) return invalid_argument("null event");
    const hipError_t e = hipEventQuery(static_cast<hipEvent_t>(event));
    if (e == hipErrorNotReady) {
        (void)hipGetLastError();
        *out_done = 0;
        return HE_OK;
    }
    HEAMD_HIP_TRY(e);
    *out_done = 1;
    return HE_OK;
}
int he_stream_wait_event(he_stream stream, he_event event) {
    if (event == nullptr) return invalid_argument("null event");
    HEAMD_HIP_TRY(hipStreamWaitEvent(as_stream(stream), static_cast<hipEvent_t>(event), 0));
    return HE_OK;
}
namespace {
struct HostCallback {
    he_host_callback function;
    void* user_data;
};
void run_host_callback(void* raw) {
    HostCallback* call = static_cast<HostCallback*>(raw);
    call->function(call->user_data);
    delete call;
}
}  // namespace
int he_stream_add_callback(he_stream stream, he_host_callback callback, void* user_data) {
    if (callback == nullptr) return invalid_argument("null callback");
    HostCallback* call = new HostCallback{callback, user_data};
    const hipError_t e = hipLaunchHostFunc(as_stream(stream), run_host_callback, call);
    if (e != hipSuccess) {
        delete call;
        return heamd::device_failure(e, "hipLaunchHostFunc");
    }
    return HE_OK;
}

// ------------------------------------------------------------------------------------------ PolyContext
static int poly_context_create(uint32_t degree, const uint64_t* moduli, uint32_t moduli_count, bool host_only,
                               he_poly_context** out) {
    if (out == nullptr) return invalid_argument("null out");
    *out = nullptr;
    std::unique_ptr<PolyContext> impl;
    const int status = PolyContext::create(degree, moduli, moduli_count, impl, host_only);
    if (status != HE_OK) {
        if (status != HE_ERR_DEVICE) heamd::set_last_error(std::string("PolyContext.init: ") + he_status_string(status));
        return status;
    }
    *out = new he_poly_context{impl.release(), true};
    return HE_OK;
}
int he_poly_context_create(uint32_t degree, const uint64_t* moduli, uint32_t moduli_count, he_poly_context** out) {
    return poly_context_create(degree, moduli, moduli_count, false, out);
}
int he_poly_context_create_host_only(uint32_t degree, const uint64_t* moduli, uint32_t moduli_count,
                                     he_poly_context** out) {
    return poly_context_create(degree, moduli, moduli_count, true, out);
}
void he_poly_context_destroy(he_poly_context* ctx) {
    heamd::RelaxedCapture relaxed;
    delete ctx;
}
uint32_t he_poly_context_degree(const he_poly_context* ctx) { return ctx ? ctx->impl->degree() : 0; }
uint32_t he_poly_context_moduli_count(const he_poly_context* ctx) { return ctx ? ctx->impl->moduli_count() : 0; }
int he_poly_context_moduli(const he_poly_context* ctx, uint64_t* out_moduli) {
    if (ctx == nullptr || out_moduli == nullptr) return invalid_argument("null pointer");
    const auto& moduli = ctx->impl->moduli();
    for (size_t i = 0; i < moduli.size(); ++i) out_moduli[i] = moduli[i];
    return HE_OK;
}
uint64_t he_poly_context_max_lazy_product_accumulation_count(const he_poly_context* ctx) {
    return ctx ? ctx->impl->max_lazy_product_accumulation_count(ctx->impl->moduli_count()) : 0;
}
int he_poly_context_q_remainder(const he_poly_context* ctx, uint64_t modulus, uint64_t* out) {
    if (ctx == nullptr || out == nullptr || modulus == 0) return invalid_argument("null pointer or zero modulus");
    const auto& moduli = ctx->impl->moduli();
    *out = heamd::product_mod(moduli.data(), moduli.size(), modulus);
    return HE_OK;
}
int he_poly_context_copy_ntt_tables(const he_poly_context* ctx, uint32_t rns_index, uint64_t* root_powers,
                                    uint64_t* root_factors, uint64_t* inverse_root_powers,
                                    uint64_t* inverse_root_factors, uint64_t* inverse_degree,
                                    uint64_t* inverse_degree_root) {
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    if (rns_index >= pc.moduli_count() || !pc.host_constants()[rns_index].has_ntt) return HE_ERR_INVALID_NTT_MODULUS;
    const heamd::U64x2* forward = pc.host_forward_twiddles(rns_index);
    const heamd::U64x2* inverse = pc.host_inverse_twiddles(rns_index);
    for (uint32_t k = 0; k < pc.degree(); ++k) {
        if (root_powers) root_powers[k] = forward[k].x;
        if (root_factors) root_factors[k] = forward[k].y;
        if (inverse_root_powers) inverse_root_powers[k] = inverse[k].x;
        if (inverse_root_factors) inverse_root_factors[k] = inverse[k].y;
    }
    if (inverse_degree) *inverse_degree = pc.host_constants()[rns_index].inv_degree;
    if (inverse_degree_root) *inverse_degree_root = pc.host_constants()[rns_index].inv_degree_root;
    return HE_OK;
}
int he_generate_primes(const int32_t* significant_bit_counts, uint32_t count, int preferring_small,
                       uint32_t ntt_degree, uint64_t* out_primes) {
    if ((count > 0 && (significant_bit_counts == nullptr || out_primes == nullptr)) ||
        !heamd::is_power_of_two(ntt_degree))
        return invalid_argument("generatePrimes arguments");
    std::vector<int> bits(significant_bit_counts, significant_bit_counts + count);
    std::vector<heamd::u64> primes;
    if (!heamd::generate_primes(bits, preferring_small != 0, ntt_degree, primes)) return HE_ERR_NOT_ENOUGH_PRIMES;
    for (uint32_t i = 0; i < count; ++i) out_primes[i] = primes[i];
    return HE_OK;
}

// ------------------------------------------------------------------------------------------ NTT
int he_ntt_forward_device(const he_poly_context* ctx, uint64_t* device_slab, size_t batch, he_stream stream) {
    return heamd::poly_ntt(ctx, device_slab, batch, false, as_stream(stream));
}
int he_ntt_inverse_device(const he_poly_context* ctx, uint64_t* device_slab, size_t batch, he_stream stream) {
    return heamd::poly_ntt(ctx, device_slab, batch, true, as_stream(stream));
}
int he_ntt_forward_rows_device(const he_poly_context* ctx, uint64_t modulus, uint64_t* device_rows, size_t rows,
                               he_stream stream) {
    return ntt_rows_device(ctx, modulus, device_rows, rows, false, as_stream(stream));
}
int he_ntt_inverse_rows_device(const he_poly_context* ctx, uint64_t modulus, uint64_t* device_rows, size_t rows,
                               he_stream stream) {
    return ntt_rows_device(ctx, modulus, device_rows, rows, true, as_stream(stream));
}
static int ntt_host(const he_poly_context* ctx, uint64_t* host_slab, size_t batch, bool inverse) {
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    if (!pc.all_ntt(pc.moduli_count())) return HE_ERR_INVALID_NTT_MODULUS;
    if (batch == 0) return HE_OK;
    if (host_slab == nullptr) return invalid_argument("null slab");
    int status = pc.check_device();
    if (status != HE_OK) return status;
    // One blocking copy - kernel - copy on the calling thread's stream.  hipMemcpyAsync from pageable memory runs at the
    // link's rate here (51 GB/s of host traffic for a 64 MiB slab, both directions counted); a pipeline of page-locked
    // staging blocks filled by worker threads was built and measured SLOWER (43 GB/s: the host-side memcpy into the blocks
    // costs more than the overlap gains) -- profiles/r05d_host_seam_pipelined_vs_blocking.txt.
    const size_t words = batch * pc.moduli_count() * pc.degree();
    return with_device_copy(host_slab, words, [&](uint64_t* device, hipStream_t stream) {
        return heamd::poly_ntt(ctx, device, batch, inverse, stream);
    });
}
int he_ntt_forward(const he_poly_context* ctx, uint64_t* host_slab, size_t batch) {
    return ntt_host(ctx, host_slab, batch, false);
}
int he_ntt_inverse(const he_poly_context* ctx, uint64_t* host_slab, size_t batch) {
    return ntt_host(ctx, host_slab, batch, true);
}
// The transform with a named kernel schedule: every accepted variant computes the same, canonical NTT; anything
// else is HE_ERR_INVALID_ARGUMENT.
int he_ntt_device_variant(const he_poly_context* ctx, uint64_t* device_slab, size_t batch, int inverse, int variant,
                          he_stream stream) {
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    if (!pc.all_ntt(pc.moduli_count())) return HE_ERR_INVALID_NTT_MODULUS;
    switch (variant) {
        case heamd::kNttVariantAuto: case heamd::kNttVariantExact: case heamd::kNttVariantGeneric:
        case heamd::kNttVariantWide: case heamd::kNttVariantApprox: break;
        default: return invalid_argument("unknown NTT variant");
    }
    if (batch == 0) return HE_OK;
    if (device_slab == nullptr) return invalid_argument("null slab");
    int status = pc.check_device();
    if (status != HE_OK) return status;
    HEAMD_HIP_TRY(heamd::launch_ntt(inverse != 0, device_slab, pc.device_context(), 0, pc.moduli_count(),
                                    batch * pc.moduli_count(), as_stream(stream), variant));
    return HE_OK;
}

// ------------------------------------------------------------------------------------------ element-wise
int he_poly_add_device(const he_poly_context* ctx, uint64_t* lhs, const uint64_t* rhs, size_t batch, he_stream s) {
    return heamd::poly_elementwise(ctx, heamd::ElementwiseOp::Add, lhs, rhs, batch, as_stream(s));
}
int he_poly_sub_device(const he_poly_context* ctx, uint64_t* lhs, const uint64_t* rhs, size_t batch, he_stream s) {
    return heamd::poly_elementwise(ctx, heamd::ElementwiseOp::Sub, lhs, rhs, batch, as_stream(s));
}
int he_poly_neg_device(const he_poly_context* ctx, uint64_t* data, size_t batch, he_stream s) {
    return heamd::poly_elementwise<uint64_t>(ctx, heamd::ElementwiseOp::Neg, data, nullptr, batch, as_stream(s));
}
int he_poly_mul_device(const he_poly_context* ctx, uint64_t* lhs, const uint64_t* rhs, size_t batch, he_stream s) {
    return heamd::poly_elementwise(ctx, heamd::ElementwiseOp::Mul, lhs, rhs, batch, as_stream(s));
}
int he_poly_apply_galois_device(const he_poly_context* ctx, const uint64_t* in, uint64_t* out, size_t batch,
                                uint64_t element, int eval_format, he_stream s) {
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    const uint64_t n = pc.degree();
    // isValidGaloisElement (Galois.swift:100-105) is a precondition of applyGalois
    if ((element & 1) == 0 || element <= 1 || element >= 2 * n) return invalid_argument("invalid Galois element");
    if (batch == 0) return HE_OK;
    if (in == nullptr || out == nullptr) return invalid_argument("null slabs");
    const size_t slab_bytes = batch * pc.moduli_count() * pc.degree() * sizeof(uint64_t);  // an index permutation of each row
    HEAMD_TRY_STATUS(heamd::check_slabs("applyGalois", {{"out", out, slab_bytes, true}, {"in", in, slab_bytes, false}}));
    int status = pc.check_device();
    if (status != HE_OK) return status;
    const size_t rows = batch * pc.moduli_count();
    if (eval_format != 0) {
        HEAMD_HIP_TRY(heamd::launch_galois_eval(in, out, pc.device_context(), static_cast<uint32_t>(element), rows,
                                                as_stream(s)));
    } else {
        uint64_t inverse = element;  // Newton: g^-1 mod 2^k for odd g
        for (int k = 0; k < 6; ++k) inverse *= 2 - element * inverse;
        HEAMD_HIP_TRY(heamd::launch_galois_coeff(in, out, pc.device_context(),
                                                 static_cast<uint32_t>(inverse & (2 * n - 1)), rows, as_stream(s)));
    }
    return HE_OK;
}

int he_poly_multiply_power_of_x_device(const he_poly_context* ctx, const uint64_t* in, uint64_t* out, size_t batch,
                                       int64_t power, he_stream s) {
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    if (batch == 0) return HE_OK;
    if (in == nullptr || out == nullptr) return invalid_argument("null slabs");
    const size_t slab_bytes = batch * pc.moduli_count() * pc.degree() * sizeof(uint64_t);  // an index permutation of each row
    HEAMD_TRY_STATUS(heamd::check_slabs("multiplyPowerOfX", {{"out", out, slab_bytes, true}, {"in", in, slab_bytes, false}}));
    int status = pc.check_device();
    if (status != HE_OK) return status;
    const int64_t twice = 2 * static_cast<int64_t>(pc.degree());
    int64_t shift = power % twice;  // x^(2N) = 1
    if (shift < 0) shift += twice;
    HEAMD_HIP_TRY(heamd::launch_multiply_power_of_x(in, out, pc.device_context(), static_cast<uint32_t>(shift),
                                                    batch * pc.moduli_count(), as_stream(s)));
    return HE_OK;
}

namespace {
// bit widths and row offsets of PolyRq.serialize (PolyRq+Serialize.swift:69-99); HE_OK or the reference's errors
int serialize_layout(const PolyContext& pc, int skip_lsbs, heamd::SerializeLayout& layout) {
    if (pc.moduli_count() > heamd::kMaxSerializedRows) {
        heamd::set_last_error("serialization supports at most 64 residue rows");
        return HE_ERR_UNSUPPORTED;
    }
    layout.rows = pc.moduli_count();
    layout.byte_offset[0] = 0;
    for (uint32_t r = 0; r < layout.rows; ++r) {
        const uint64_t q = pc.moduli()[r];
        int bits = 64 - __builtin_clzll(q);               // significant bits
        if ((q & (q - 1)) == 0) bits -= 1;                // ceilLog2 (ModularArithmetic/Scalar.swift:266-269)
        // CoefficientPacking.validate (CoefficientPacking.swift:27-31)
        if (!(bits > 0 && bits > skip_lsbs && skip_lsbs >= 0)) {
            heamd::set_last_error("invalid coefficient packing: bitsPerCoeff " + std::to_string(bits) + ", skipLSBs " +
                                  std::to_string(skip_lsbs));
            return HE_ERR_INVALID_COEFFICIENT_PACKING;
        }
        layout.width[r] = static_cast<uint32_t>(bits - skip_lsbs);
        layout.byte_offset[r + 1] = layout.byte_offset[r] + (uint64_t(pc.degree()) * layout.width[r] + 7) / 8;
    }
    return HE_OK;
}
}  // namespace

extern "C++" {  // (templates)
namespace {
int check_moduli_fit_u32(const PolyContext& pc) {
    for (uint32_t i = 0; i < pc.moduli_count(); ++i)
        if (pc.moduli()[i] > ((uint64_t(1) << 30) - 1)) {
            heamd::set_last_error("modulus " + std::to_string(pc.moduli()[i]) + " does not fit UInt32 (max 2^30 - 1)");
            return HE_ERR_INVALID_MODULUS;
        }
    return HE_OK;
}

uint32_t log2_of_degree(const PolyContext& pc) { return static_cast<uint32_t>(__builtin_ctz(pc.degree())); }

// the polynomial-level wire entries, one body for 8- and 4-byte slabs (4-byte: every modulus must fit UInt32)
template <typename W>
int poly_serialize(const he_poly_context* ctx, const W* device_slab, size_t batch, int skip_lsbs, uint8_t* device_bytes,
                   he_stream s) {
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    if (sizeof(W) == 4) {
        const int fits = check_moduli_fit_u32(pc);
        if (fits != HE_OK) return fits;
    }
    heamd::SerializeLayout layout{};
    int status = serialize_layout(pc, skip_lsbs, layout);
    if (status != HE_OK) return status;
    if (batch == 0) return HE_OK;
    if (device_slab == nullptr || device_bytes == nullptr) return invalid_argument("null buffer");
    HEAMD_TRY_STATUS(heamd::check_slabs(
        "serialize", {{"device_bytes", device_bytes, batch * static_cast<size_t>(layout.byte_offset[layout.rows]), true},
                      {"device_slab", device_slab, batch * pc.moduli_count() * pc.degree() * sizeof(W), false}}));
    status = pc.check_device();
    if (status != HE_OK) return status;
    HEAMD_HIP_TRY(heamd::launch_serialize(device_slab, device_bytes, layout, log2_of_degree(pc),
                                          static_cast<uint32_t>(skip_lsbs), batch, as_stream(s)));
    return HE_OK;
}

template <typename W>
int poly_deserialize(const he_poly_context* ctx, const uint8_t* device_bytes, size_t bytes_per_poly, size_t batch,
                     int skip_lsbs, W* device_slab, he_stream s) {
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    if (sizeof(W) == 4) {
        const int fits = check_moduli_fit_u32(pc);
        if (fits != HE_OK) return fits;
    }
    heamd::SerializeLayout layout{};
    int status = serialize_layout(pc, skip_lsbs, layout);
    if (status != HE_OK) return status;
    if (bytes_per_poly < layout.byte_offset[layout.rows]) {  // PolyRq+Serialize.swift:41-51
        heamd::set_last_error("serialized buffer holds " + std::to_string(bytes_per_poly) + " bytes, expected " +
                              std::to_string(layout.byte_offset[layout.rows]));
        return HE_ERR_SERIALIZED_BUFFER_SIZE_MISMATCH;
    }
    if (batch == 0) return HE_OK;
    if (device_slab == nullptr || device_bytes == nullptr) return invalid_argument("null buffer");
    HEAMD_TRY_STATUS(heamd::check_slabs(
        "deserialize", {{"device_slab", device_slab, batch * pc.moduli_count() * pc.degree() * sizeof(W), true},
                        {"device_bytes", device_bytes, batch * bytes_per_poly, false}}));
    status = pc.check_device();
    if (status != HE_OK) return status;
    HEAMD_HIP_TRY(heamd::launch_deserialize(device_bytes, device_slab, layout, log2_of_degree(pc),
                                            static_cast<uint32_t>(skip_lsbs), bytes_per_poly, batch, as_stream(s)));
    return HE_OK;
}

template <typename W>
int poly_random_from_seeds(const he_poly_context* ctx, const uint8_t* device_seeds, size_t batch, W* device_slab,
                           he_stream s) {
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    if (sizeof(W) == 4) {
        const int fits = check_moduli_fit_u32(pc);
        if (fits != HE_OK) return fits;
    }
    if (batch == 0) return HE_OK;
    if (device_seeds == nullptr || device_slab == nullptr) return invalid_argument("null buffer");
    HEAMD_TRY_STATUS(heamd::check_slabs(
        "random(seed:)", {{"device_slab", device_slab, batch * pc.moduli_count() * pc.degree() * sizeof(W), true},
                          {"device_seeds", device_seeds, batch * 32, false}}));
    int status = pc.check_device();
    if (status != HE_OK) return status;
    heamd::Scratch chain(as_stream(s));
    HEAMD_HIP_TRY(chain.allocate(heamd::seeded_uniform_scratch_bytes(pc.device_context(), batch)));
    HEAMD_HIP_TRY(heamd::launch_seeded_uniform(device_seeds, device_slab, size_t(pc.moduli_count()) * pc.degree(),
                                               pc.device_context(), batch, chain.get(), as_stream(s)));
    return HE_OK;
}
}  // namespace
}  // extern "C++"

size_t he_poly_serialization_byte_count(const he_poly_context* ctx, int skip_lsbs) {
    if (ctx == nullptr) return 0;
    heamd::SerializeLayout layout{};
    if (serialize_layout(*ctx->impl, skip_lsbs, layout) != HE_OK) return 0;
    return static_cast<size_t>(layout.byte_offset[layout.rows]);
}

int he_poly_serialize_device(const he_poly_context* ctx, const uint64_t* device_slab, size_t batch, int skip_lsbs,
                             uint8_t* device_bytes, he_stream s) {
    return poly_serialize(ctx, device_slab, batch, skip_lsbs, device_bytes, s);
}
int he_poly_deserialize_device(const he_poly_context* ctx, const uint8_t* device_bytes, size_t bytes_per_poly,
                               size_t batch, int skip_lsbs, uint64_t* device_slab, he_stream s) {
    return poly_deserialize(ctx, device_bytes, bytes_per_poly, batch, skip_lsbs, device_slab, s);
}
int he_poly_random_from_seeds_device(const he_poly_context* ctx, const uint8_t* device_seeds, size_t batch,
                                     uint64_t* device_slab, he_stream s) {
    return poly_random_from_seeds(ctx, device_seeds, batch, device_slab, s);
}

// ------------------------------------------------------------------------------------------ PolyRq<UInt32>
int he_ntt_forward_device_u32(const he_poly_context* ctx, uint32_t* device_slab, size_t batch, he_stream s) {
    return heamd::poly_ntt(ctx, device_slab, batch, false, as_stream(s));
}
int he_ntt_inverse_device_u32(const he_poly_context* ctx, uint32_t* device_slab, size_t batch, he_stream s) {
    return heamd::poly_ntt(ctx, device_slab, batch, true, as_stream(s));
}
int he_poly_add_device_u32(const he_poly_context* ctx, uint32_t* lhs, const uint32_t* rhs, size_t batch, he_stream s) {
    return heamd::poly_elementwise(ctx, heamd::ElementwiseOp::Add, lhs, rhs, batch, as_stream(s));
}
// ---- word-size bridge for Bfv<UInt32> callers
int he_words_widen_u32_device(const uint32_t* in, uint64_t* out, size_t words, he_stream s) {
    if (words == 0) return HE_OK;
    if (in == nullptr || out == nullptr) return invalid_argument("null slab");
    // word k is read at 4 k and stored at 8 k: in place, a lane stores over words that another has yet to read
    HEAMD_TRY_STATUS(heamd::check_slabs("widen", {{"device_out", out, words * 8, true}, {"device_in", in, words * 4, false}}));
    if ((reinterpret_cast<uintptr_t>(in) & 15u) != 0 || (reinterpret_cast<uintptr_t>(out) & 15u) != 0)
        return invalid_argument("slabs must be 16-byte aligned");
    HEAMD_HIP_TRY(heamd::launch_widen_words(in, out, words, as_stream(s)));
    return HE_OK;
}
int he_words_copy_device(const uint64_t* in, uint64_t* out, size_t words, int non_temporal, he_stream s) {
    if (words == 0) return HE_OK;
    if (in == nullptr || out == nullptr) return invalid_argument("null slab");
    HEAMD_TRY_STATUS(heamd::check_slabs("copy", {{"device_out", out, words * 8, true}, {"device_in", in, words * 8, false}}));
    HEAMD_HIP_TRY(heamd::launch_stream_copy(in, out, words, non_temporal != 0, as_stream(s)));
    return HE_OK;
}
int he_words_narrow_u64_device(const uint64_t* in, uint32_t* out, size_t words, he_stream s) {
    if (words == 0) return HE_OK;
    if (in == nullptr || out == nullptr) return invalid_argument("null slab");
    HEAMD_TRY_STATUS(heamd::check_slabs("narrow", {{"device_out", out, words * 4, true}, {"device_in", in, words * 8, false}}));
    if ((reinterpret_cast<uintptr_t>(in) & 15u) != 0 || (reinterpret_cast<uintptr_t>(out) & 15u) != 0)
        return invalid_argument("slabs must be 16-byte aligned");
    HEAMD_HIP_TRY(heamd::launch_narrow_words(in, out, words, as_stream(s)));
    return HE_OK;
}

int he_poly_sub_device_u32(const he_poly_context* ctx, uint32_t* lhs, const uint32_t* rhs, size_t batch, he_stream s) {
    return heamd::poly_elementwise(ctx, heamd::ElementwiseOp::Sub, lhs, rhs, batch, as_stream(s));
}
int he_poly_neg_device_u32(const he_poly_context* ctx, uint32_t* data, size_t batch, he_stream s) {
    return heamd::poly_elementwise<uint32_t>(ctx, heamd::ElementwiseOp::Neg, data, nullptr, batch, as_stream(s));
}
int he_poly_mul_device_u32(const he_poly_context* ctx, uint32_t* lhs, const uint32_t* rhs, size_t batch, he_stream s) {
    return heamd::poly_elementwise(ctx, heamd::ElementwiseOp::Mul, lhs, rhs, batch, as_stream(s));
}
int he_poly_mul_scalar_device_u32(const he_poly_context* ctx, uint32_t* data, const uint32_t* scalar_residues,
                                  size_t batch, he_stream s) {
    return poly_mul_scalar(ctx, data, scalar_residues, batch, s);
}
int he_poly_divide_and_round_q_last_device_u32(const he_poly_context* ctx, const uint32_t* device_in,
                                               uint32_t* device_out, size_t batch, he_stream s) {
    return poly_divide_and_round_q_last(ctx, device_in, device_out, batch, s);
}

// ------------------------------------------------------------------- wire format of whole ciphertexts, and on 4-byte slabs
extern "C++" {  // (templates)
namespace {
// the record of `poly_count` polynomials behind a header of header_bytes: serialize_layout per polynomial, one after another
int ciphertext_wire_layout(const PolyContext& pc, uint32_t poly_count, const int* skip_lsbs, uint32_t header_bytes,
                           heamd::CiphertextWireLayout& out) {
    if (poly_count < 1 || poly_count > heamd::kMaxWirePolys) {
        heamd::set_last_error("a ciphertext record holds 1 to 3 polynomials, not " + std::to_string(poly_count));
        return HE_ERR_UNSUPPORTED;
    }
    out.polys = poly_count;
    out.rows = pc.moduli_count();
    out.byte_offset[0] = header_bytes;
    for (uint32_t p = 0; p < poly_count; ++p) {
        const int skip = skip_lsbs == nullptr ? 0 : skip_lsbs[p];
        heamd::SerializeLayout poly{};
        const int status = serialize_layout(pc, skip, poly);
        if (status != HE_OK) return status;
        out.skip[p] = static_cast<uint8_t>(skip);
        for (uint32_t r = 0; r < poly.rows; ++r) {
            const uint32_t f = p * poly.rows + r;
            out.width[f] = static_cast<uint8_t>(poly.width[r]);
            out.byte_offset[f + 1] = out.byte_offset[f] + (poly.byte_offset[r + 1] - poly.byte_offset[r]);
        }
    }
    return HE_OK;
}

int short_stride(size_t stride, uint64_t need) {
    heamd::set_last_error("record stride " + std::to_string(stride) + " is below the record's " + std::to_string(need) +
                          " bytes");
    return HE_ERR_SERIALIZED_BUFFER_SIZE_MISMATCH;
}

template <typename W>
int ciphertexts_serialize(const he_poly_context* ctx, const W* cts, size_t count, uint32_t poly_count, const int* skip_lsbs,
                          uint8_t* records, size_t record_stride, he_stream s) {
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    if (sizeof(W) == 4) {
        const int fits = check_moduli_fit_u32(pc);
        if (fits != HE_OK) return fits;
    }
    heamd::CiphertextWireLayout layout{};
    int status = ciphertext_wire_layout(pc, poly_count, skip_lsbs, 2, layout);
    if (status != HE_OK) return status;
    const uint64_t record_bytes = layout.byte_offset[layout.polys * layout.rows];
    if (record_stride < record_bytes) return short_stride(record_stride, record_bytes);
    if (count == 0) return HE_OK;
    if (cts == nullptr || records == nullptr) return invalid_argument("null buffer");
    // (the records' range runs from the first record's first byte to the last one's last, the gaps between them included)
    HEAMD_TRY_STATUS(heamd::check_slabs(
        "serialize", {{"records", records, (count - 1) * record_stride + static_cast<size_t>(record_bytes), true},
                      {"cts", cts, count * poly_count * pc.moduli_count() * pc.degree() * sizeof(W), false}}));
    status = pc.check_device();
    if (status != HE_OK) return status;
    HEAMD_HIP_TRY(heamd::launch_ciphertexts_serialize(cts, size_t(poly_count) * pc.moduli_count() * pc.degree(), records,
                                                      record_stride, layout, log2_of_degree(pc), count, as_stream(s)));
    return HE_OK;
}

template <typename W>
int ciphertexts_deserialize(const he_poly_context* ctx, const uint8_t* records, size_t record_stride, size_t count,
                            uint32_t poly_count, const int* skip_lsbs, W* cts, uint32_t* device_header_mismatch, he_stream s) {
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    if (sizeof(W) == 4) {
        const int fits = check_moduli_fit_u32(pc);
        if (fits != HE_OK) return fits;
    }
    heamd::CiphertextWireLayout layout{};
    int status = ciphertext_wire_layout(pc, poly_count, skip_lsbs, 2, layout);
    if (status != HE_OK) return status;
    const uint64_t record_bytes = layout.byte_offset[layout.polys * layout.rows];
    if (record_stride < record_bytes) return short_stride(record_stride, record_bytes);
    if (count == 0) return HE_OK;
    if (cts == nullptr || records == nullptr) return invalid_argument("null buffer");
    HEAMD_TRY_STATUS(heamd::check_slabs(
        "deserialize", {{"cts", cts, count * poly_count * pc.moduli_count() * pc.degree() * sizeof(W), true},
                        {"device_header_mismatch", device_header_mismatch, sizeof(uint32_t), true},
                        {"records", records, (count - 1) * record_stride + static_cast<size_t>(record_bytes), false}}));
    status = pc.check_device();
    if (status != HE_OK) return status;
    HEAMD_HIP_TRY(heamd::launch_ciphertexts_deserialize(records, record_stride, cts,
                                                        size_t(poly_count) * pc.moduli_count() * pc.degree(), layout,
                                                        log2_of_degree(pc), count, device_header_mismatch, as_stream(s)));
    return HE_OK;
}

template <typename W>
int ciphertexts_deserialize_seeded(const he_poly_context* ctx, const uint8_t* poly0_bytes, size_t record_stride,
                                   const uint8_t* seeds, size_t count, int coeff_format, W* cts, he_stream s) {
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    if (sizeof(W) == 4) {
        const int fits = check_moduli_fit_u32(pc);
        if (fits != HE_OK) return fits;
    }
    heamd::CiphertextWireLayout layout{};
    int status = ciphertext_wire_layout(pc, 1, nullptr, 0, layout);  // poly0 is a bare PolyRq record, skipLSBs 0
    if (status != HE_OK) return status;
    const uint64_t record_bytes = layout.byte_offset[layout.rows];
    if (poly0_bytes != nullptr && record_stride < record_bytes) return short_stride(record_stride, record_bytes);
    if (coeff_format != 0 && seeds != nullptr) {
        if (!pc.all_ntt(pc.moduli_count())) {  // validateNttModuli (PolyContext.swift:175-181), as he_ntt_inverse_device
            heamd::set_last_error("a modulus of this context is not an NTT modulus for degree " + std::to_string(pc.degree()));
            return HE_ERR_INVALID_NTT_MODULUS;
        }
        // nothing is enqueued for a transform that does not exist: the 4-byte launch_ntt holds a row in the LDS, up to N = 32768
        if (sizeof(W) == 4 && pc.degree() > 32768) {
            heamd::set_last_error("UInt32 transform supports degrees up to 32768");
            return HE_ERR_UNSUPPORTED;
        }
    }
    if (count == 0) return HE_OK;
    if (cts == nullptr) return invalid_argument("null ciphertexts");
    HEAMD_TRY_STATUS(heamd::check_slabs(
        "deserialize(seeded:)", {{"cts", cts, count * 2 * pc.moduli_count() * pc.degree() * sizeof(W), true},
                                 {"poly0_bytes", poly0_bytes, (count - 1) * record_stride + static_cast<size_t>(record_bytes), false},
                                 {"seeds", seeds, count * 32, false}}));
    status = pc.check_device();
    if (status != HE_OK) return status;
    hipStream_t stream = as_stream(s);
    const size_t poly_words = size_t(pc.moduli_count()) * pc.degree();
    if (poly0_bytes != nullptr)
        HEAMD_HIP_TRY(heamd::launch_ciphertexts_deserialize(poly0_bytes, record_stride, cts, 2 * poly_words, layout,
                                                            log2_of_degree(pc), count, nullptr, stream));
    if (seeds != nullptr) {
        heamd::Scratch chain(stream);
        HEAMD_HIP_TRY(chain.allocate(heamd::seeded_uniform_scratch_bytes(pc.device_context(), count)));
        HEAMD_HIP_TRY(heamd::launch_seeded_uniform(seeds, cts + poly_words, 2 * poly_words, pc.device_context(), count,
                                                   chain.get(), stream));
        // a Coeff ciphertext takes the inverse transform of its `a` (Bfv+Encrypt.swift:155-156): the rows of slot 1 are not
        // contiguous across ciphertexts, so one transform per ciphertext -- a query is a handful of ciphertexts, and the keys,
        // which come by the dozen, are Eval and take none
        if (coeff_format != 0)
            for (size_t i = 0; i < count; ++i) {
                HEAMD_HIP_TRY(ntt_rows(true, cts + (2 * i + 1) * poly_words, pc, pc.device_context(), pc.moduli_count(),
                                       pc.moduli_count(), stream));
            }
    }
    return HE_OK;
}

}  // namespace

int heamd::poly_wire_layout(const PolyContext& pc, heamd::CiphertextWireLayout& out) {
    return ciphertext_wire_layout(pc, 1, nullptr, 0, out);
}
}  // extern "C++"

int he_bfv_skip_lsbs_for_decryption(uint32_t degree, uint64_t q0, uint64_t plaintext_modulus, uint32_t moduli_count,
                                    int out_skip_lsbs[2]) {
    if (out_skip_lsbs == nullptr) return invalid_argument("null output");
    if (degree == 0 || q0 == 0 || plaintext_modulus == 0 || moduli_count == 0) return invalid_argument("zero parameter");
    out_skip_lsbs[0] = out_skip_lsbs[1] = 0;
    if (moduli_count != 1) return HE_OK;  // Bfv+Decrypt.swift:52-54
    const uint64_t t = plaintext_modulus;
    // floor(log2(q0 / t)) - 3, one bit kept for the rounding and two for the ciphertext's own error (:59-74)
    const int l_prime = q0 / 2 >= t ? (63 - __builtin_clzll(q0 / t)) - 3 : 0;
    // Int(8 sqrt(2 N / 9)): z-score 8 on the error that the dropped bits of `a` add (:100-103)
    const long long tmp = static_cast<long long>(8.0 * std::sqrt(2.0 * static_cast<double>(degree) / 9.0));
    int ceil_log2 = 0;
    if (tmp > 1) ceil_log2 = 64 - __builtin_clzll(static_cast<unsigned long long>(tmp - 1));
    const int poly1 = l_prime - ceil_log2;
    if (poly1 <= 1) {  // at most one bit off `a`: take it off `b`, whose effect is deterministic (:104-107)
        out_skip_lsbs[0] = l_prime + 1 > 0 ? l_prime + 1 : 0;
        out_skip_lsbs[1] = 0;
    } else {
        out_skip_lsbs[0] = l_prime > 0 ? l_prime : 0;
        out_skip_lsbs[1] = poly1;
    }
    return HE_OK;
}

size_t he_ciphertexts_serialization_byte_count(const he_poly_context* ctx, uint32_t poly_count, const int* skip_lsbs) {
    if (ctx == nullptr) return 0;
    heamd::CiphertextWireLayout layout{};
    if (ciphertext_wire_layout(*ctx->impl, poly_count, skip_lsbs, 2, layout) != HE_OK) return 0;
    return static_cast<size_t>(layout.byte_offset[layout.polys * layout.rows]);
}

int he_ciphertexts_wire_plan(int direction, uint32_t word_bits, const he_poly_context* ctx, uint32_t poly_count,
                             const int* skip_lsbs, size_t record_stride, uint64_t records_address, uint64_t slab_address,
                             uint32_t* out_form, size_t* out_record_bytes, size_t* out_items_per_record,
                             uint32_t* out_edge_free) {
    if (ctx == nullptr) return invalid_argument("null context");
    if (direction != 0 && direction != 1) return invalid_argument("direction must be 0 (serialize) or 1 (deserialize)");
    if (word_bits != 32 && word_bits != 64) return invalid_argument("word_bits must be 32 or 64");
    const PolyContext& pc = *ctx->impl;
    if (word_bits == 32) {
        const int fits = check_moduli_fit_u32(pc);
        if (fits != HE_OK) return fits;
    }
    uint32_t form = 0, edge_free = 0;
    uint64_t record_bytes = 0, items = 0;
    if (poly_count == 0) {  // the polynomial-level entries: serialize_form.hpp
        heamd::SerializeLayout layout{};
        const int status = serialize_layout(pc, skip_lsbs == nullptr ? 0 : skip_lsbs[0], layout);
        if (status != HE_OK) return status;
        record_bytes = layout.byte_offset[layout.rows];
        if (direction == 1 && record_stride < record_bytes) return short_stride(record_stride, record_bytes);
        namespace sf = heamd::serialize_form;
        const uintptr_t bytes = static_cast<uintptr_t>(records_address), slab = static_cast<uintptr_t>(slab_address);
        const uint32_t logn = log2_of_degree(pc);
        sf::Form f;
        if (word_bits == 64)
            f = direction == 0 ? sf::for_serialize(layout.rows, layout.width, layout.byte_offset, bytes, slab, logn)
                               : sf::for_deserialize(layout.rows, layout.width, layout.byte_offset, bytes, slab, logn,
                                                     record_stride);
        else
            f = direction == 0 ? sf::for_serialize_narrow(layout.rows, layout.byte_offset, bytes)
                               : sf::for_deserialize_narrow(layout.rows, layout.byte_offset, bytes, record_stride);
        form = static_cast<uint32_t>(f);
        const uint64_t coefficients = uint64_t(layout.rows) << log2_of_degree(pc);
        items = direction == 1 ? (f == sf::Form::kTile ? layout.rows : coefficients)
                               : (f == sf::Form::kTile ? layout.rows : f == sf::Form::kWord ? record_bytes >> 3 : record_bytes);
        edge_free = f != sf::Form::kByte;
    } else {
        heamd::CiphertextWireLayout layout{};
        const int status = ciphertext_wire_layout(pc, poly_count, skip_lsbs, 2, layout);
        if (status != HE_OK) return status;
        record_bytes = layout.byte_offset[layout.polys * layout.rows];
        if (record_stride < record_bytes) return short_stride(record_stride, record_bytes);
        namespace cf = heamd::ciphertext_wire_form;
        const cf::Plan plan = direction == 0 ? cf::for_serialize(record_bytes, record_stride,
                                                                 static_cast<uintptr_t>(records_address))
                                             : cf::for_deserialize(layout.polys, layout.rows, log2_of_degree(pc), record_stride,
                                                                   static_cast<uintptr_t>(records_address));
        form = static_cast<uint32_t>(plan.form);
        items = plan.items_per_record;
        edge_free = plan.edge_free ? 1 : 0;
    }
    if (out_form != nullptr) *out_form = form;
    if (out_record_bytes != nullptr) *out_record_bytes = static_cast<size_t>(record_bytes);
    if (out_items_per_record != nullptr) *out_items_per_record = static_cast<size_t>(items);
    if (out_edge_free != nullptr) *out_edge_free = edge_free;
    return HE_OK;
}

int he_ciphertexts_serialize_device(const he_poly_context* ctx, const uint64_t* cts, size_t count, uint32_t poly_count,
                                    const int* skip_lsbs, uint8_t* records, size_t record_stride, he_stream s) {
    return ciphertexts_serialize(ctx, cts, count, poly_count, skip_lsbs, records, record_stride, s);
}
int he_ciphertexts_serialize_device_u32(const he_poly_context* ctx, const uint32_t* cts, size_t count, uint32_t poly_count,
                                        const int* skip_lsbs, uint8_t* records, size_t record_stride, he_stream s) {
    return ciphertexts_serialize(ctx, cts, count, poly_count, skip_lsbs, records, record_stride, s);
}
int he_ciphertexts_deserialize_device(const he_poly_context* ctx, const uint8_t* records, size_t record_stride, size_t count,
                                      uint32_t poly_count, const int* skip_lsbs, uint64_t* cts,
                                      uint32_t* device_header_mismatch, he_stream s) {
    return ciphertexts_deserialize(ctx, records, record_stride, count, poly_count, skip_lsbs, cts, device_header_mismatch, s);
}
int he_ciphertexts_deserialize_device_u32(const he_poly_context* ctx, const uint8_t* records, size_t record_stride,
                                          size_t count, uint32_t poly_count, const int* skip_lsbs, uint32_t* cts,
                                          uint32_t* device_header_mismatch, he_stream s) {
    return ciphertexts_deserialize(ctx, records, record_stride, count, poly_count, skip_lsbs, cts, device_header_mismatch, s);
}
int he_ciphertexts_deserialize_seeded_device(const he_poly_context* ctx, const uint8_t* poly0_bytes, size_t record_stride,
                                             const uint8_t* seeds, size_t count, int coeff_format, uint64_t* cts,
                                             he_stream s) {
    return ciphertexts_deserialize_seeded(ctx, poly0_bytes, record_stride, seeds, count, coeff_format, cts, s);
}
int he_ciphertexts_deserialize_seeded_device_u32(const he_poly_context* ctx, const uint8_t* poly0_bytes, size_t record_stride,
                                                 const uint8_t* seeds, size_t count, int coeff_format, uint32_t* cts,
                                                 he_stream s) {
    return ciphertexts_deserialize_seeded(ctx, poly0_bytes, record_stride, seeds, count, coeff_format, cts, s);
}

int he_poly_serialize_device_u32(const he_poly_context* ctx, const uint32_t* device_slab, size_t batch, int skip_lsbs,
                                 uint8_t* device_bytes, he_stream s) {
    return poly_serialize(ctx, device_slab, batch, skip_lsbs, device_bytes, s);
}
int he_poly_deserialize_device_u32(const he_poly_context* ctx, const uint8_t* device_bytes, size_t bytes_per_poly,
                                   size_t batch, int skip_lsbs, uint32_t* device_slab, he_stream s) {
    return poly_deserialize(ctx, device_bytes, bytes_per_poly, batch, skip_lsbs, device_slab, s);
}
int he_poly_random_from_seeds_device_u32(const he_poly_context* ctx, const uint8_t* device_seeds, size_t batch,
                                         uint32_t* device_slab, he_stream s) {
    return poly_random_from_seeds(ctx, device_seeds, batch, device_slab, s);
}

int he_poly_mul_scalar_device(const he_poly_context* ctx, uint64_t* data, const uint64_t* scalar_residues,
                              size_t batch, he_stream s) {
    return poly_mul_scalar(ctx, data, scalar_residues, batch, s);
}
int he_poly_divide_and_round_q_last_device(const he_poly_context* ctx, const uint64_t* in, uint64_t* out,
                                           size_t batch, he_stream s) {
    return poly_divide_and_round_q_last(ctx, in, out, batch, s);
}
int he_poly_divide_and_round_q_last(const he_poly_context* ctx, const uint64_t* host_in, uint64_t* host_out,
                                    size_t batch) {
    if (ctx == nullptr) return invalid_argument("null context");
    const PolyContext& pc = *ctx->impl;
    if (pc.moduli_count() < 2) return HE_ERR_INVALID_POLY_CONTEXT;
    if (batch == 0) return HE_OK;
    if (host_in == nullptr || host_out == nullptr) return invalid_argument("null slab");
    int status = pc.check_device();
    if (status != HE_OK) return status;
    const size_t n = pc.degree(), L = pc.moduli_count();
    const size_t in_words = batch * L * n, out_words = batch * (L - 1) * n;
    hipStream_t stream = hipStreamPerThread;
    void* device = nullptr;
    HEAMD_HIP_TRY(hipMalloc(&device, (in_words + out_words) * sizeof(uint64_t)));
    uint64_t* d_in = static_cast<uint64_t*>(device);
    uint64_t* d_out = d_in + in_words;
    hipError_t e = hipMemcpyAsync(d_in, host_in, in_words * sizeof(uint64_t), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = heamd::launch_divide_and_round_q_last(d_in, d_out, pc.device_context(), L, batch, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(host_out, d_out, out_words * sizeof(uint64_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(device);
    if (e != hipSuccess) return heamd::device_failure(e, "he_poly_divide_and_round_q_last");
    return HE_OK;
}

int he_poly_adding_lazy_product_device(const he_poly_context* ctx, const uint64_t* lhs, const uint64_t* rhs,
                                       uint64_t* acc_lo_hi, he_stream s) {
    if (ctx == nullptr || lhs == nullptr || rhs == nullptr || acc_lo_hi == nullptr) return invalid_argument("null");
    const size_t poly_bytes = size_t(ctx->impl->moduli_count()) * ctx->impl->degree() * sizeof(uint64_t);
    HEAMD_TRY_STATUS(heamd::check_slabs("addingLazyProduct", {{"acc_lo_hi", acc_lo_hi, 2 * poly_bytes, true},
                                                              {"lhs", lhs, poly_bytes, false},
                                                              {"rhs", rhs, poly_bytes, false}}));
    int status = ctx->impl->check_device();
    if (status != HE_OK) return status;
    HEAMD_HIP_TRY(heamd::launch_adding_lazy_product(lhs, rhs, acc_lo_hi, ctx->impl->device_context(), as_stream(s)));
    return HE_OK;
}
int he_poly_reduce_accumulator_device(const he_poly_context* ctx, const uint64_t* acc_lo_hi, uint64_t* out,
                                      he_stream s) {
    if (ctx == nullptr || acc_lo_hi == nullptr || out == nullptr) return invalid_argument("null");
    const size_t poly_bytes = size_t(ctx->impl->moduli_count()) * ctx->impl->degree() * sizeof(uint64_t);
    HEAMD_TRY_STATUS(heamd::check_slabs("reduceAccumulator", {{"out", out, poly_bytes, true},
                                                              {"acc_lo_hi", acc_lo_hi, 2 * poly_bytes, false}}));
    int status = ctx->impl->check_device();
    if (status != HE_OK) return status;
    HEAMD_HIP_TRY(heamd::launch_reduce_accumulator(acc_lo_hi, out, ctx->impl->device_context(), as_stream(s)));
    return HE_OK;
}

}  // extern "C"

