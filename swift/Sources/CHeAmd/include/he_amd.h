/*
 * he_amd.h -- C ABI of the MI355X-native BFV ciphertext-arithmetic engine (libhe_amd.so).
 *
 * This is the drop-in boundary for the PolyRq/NTT hot path of apple/swift-homomorphic-encryption.  It is meant to
 * be wrapped as a SwiftPM C target next to `CUtil` (reference Package.swift:100-105) and called from
 * `Bfv<UInt64>` / `PolyContext<UInt64>`; INTEGRATION.md shows the Swift binding.  Only plain pointers and sizes
 * cross the boundary.  All citations below are file:line relative to /root/reference/Sources/.
 *
 * Conventions:
 *  - Data layout: a polynomial is the reference's Array2d row-major (moduli x N) slab of UInt64
 *    (HomomorphicEncryption/Array2d.swift:117-119); batches are [batch][L][N]; ciphertexts [batch][polys][L][N].
 *  - Every word handed across the boundary is canonical (< its row's modulus), as PolyRq asserts
 *    (PolyRq/PolyRq.swift:36,85-95); every word handed back is canonical and bit-identical to the reference.
 *  - Errors: functions return an int status, 0 = HE_OK, otherwise one code per reachable HeError case
 *    (HomomorphicEncryption/Error.swift:19-54); the Swift wrapper throws.  Nothing aborts.
 *  - Threading: contexts are immutable after creation and every entry point is re-entrant on a shared context
 *    (the reference calls the path concurrently from many tasks: Bfv/Bfv.swift:270-287).  `*_device` functions
 *    enqueue on the caller's HIP stream and return without synchronising; host-pointer functions block.
 *  - Ownership: host pointers are borrowed for the duration of the call only (the reference's seam is
 *    `withUnsafeMutableBufferPointer`, PolyRq/PolyRq+Ntt.swift:215-218).  Device buffers are owned by the caller
 *    (he_device_malloc / any HIP allocation, e.g. a torch tensor's data_ptr()).
 *  - A context lives on the HIP device that was current when it was created; calls must be made with that device
 *    current (one process per GPU).
 *  - Pointer contract: what may alias among the device slabs of ONE call (every `*_device` entry of B1-B3; the composite
 *    protocol entries of B4 and below -- he_pir_*, he_pnns_*, he_simple_pir_*, he_keyword_*, he_*_group -- are not covered
 *    yet).  A slab is the byte range its layout spans, [pointer, pointer + bytes); a caller's `workspace` is the range
 *    [workspace, workspace + workspace_bytes) and counts as written; records `stride` bytes apart span from the first
 *    record's first byte to the last record's last byte.
 *      1. Slabs a call only reads (the operands of a product, a key, a plaintext, seeds) may be the same memory or overlap
 *         freely: he_bfv_mul_device(ct, ct) squares, he_bfv_inner_product_device(v, v) is fine.
 *      2. An in-place entry (`lhs` / `data` / `ct` is updated) takes its read-only operand at EXACTLY the slab it updates where
 *         each lane reads only the words it writes: he_poly_add/sub/mul_device(x, x) double, clear and square x;
 *         he_bfv_mul_plain_device with pt == ct for one ciphertext (batch == 1: the ciphertext times its own first
 *         polynomial) or one polynomial per ciphertext.  Any other overlap of the two is HE_ERR_INVALID_ARGUMENT.
 *      3. An out-of-place entry refuses every overlap between a slab it writes and any other slab of the call:
 *         HE_ERR_INVALID_ARGUMENT, text "<operation>: <written> overlaps <other>", before anything is enqueued -- the
 *         lanes of a kernel run in no particular order, so such a call would be right for some shapes and silently wrong
 *         for others.  The exceptions, each lane-local by construction and stated again at its entry:
 *           he_bfv_relinearize_device             batch == 1 and out == ct3: one ciphertext onto its own (c0, c1)
 *           he_bfv_apply_galois[_grouped]_device  out == ct: ct is permuted into the workspace before out is stored
 *           he_bfv_mod_switch_down_to_single_device  moduli_count == 1 and out == in: already there, nothing is done
 *      4. Abutting ranges do not overlap.  Empty ranges (a batch of 0) overlap nothing: such calls stay no-ops.
 *    The refusal is an argument check: the scheme, decrypt and encrypt entries make it ahead of the device check (a host-only
 *    context refuses an overlap too), the 4-byte polynomial entries behind it, where their null-slab check is.
 */
#ifndef HE_AMD_H
#define HE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: HeError cases reachable on the path (HomomorphicEncryption/Error.swift:19-54) ---- */
enum he_status {
    HE_OK = 0,
    HE_ERR_INVALID_DEGREE = 1,                          /* invalidDegree            PolyRq/PolyContext.swift:46 */
    HE_ERR_INVALID_MODULUS = 2,                         /* invalidModulus           PolyRq/PolyContext.swift:55,58 */
    HE_ERR_COPRIME_MODULI = 3,                          /* coprimeModuli            PolyRq/PolyContext.swift:65,68 */
    HE_ERR_EMPTY_MODULUS = 4,                           /* emptyModulus             PolyRq/PolyContext.swift:71 */
    HE_ERR_INVALID_NTT_MODULUS = 5,                     /* invalidNttModulus        PolyRq/PolyContext.swift:175-181 */
    HE_ERR_INVALID_POLY_CONTEXT = 6,                    /* invalidPolyContext       PolyRq/PolyRq.swift:366-368 */
    HE_ERR_POLY_CONTEXT_MISMATCH = 7,                   /* polyContextMismatch      PolyRq/PolyRq.swift:332-336 */
    HE_ERR_INVALID_CIPHERTEXT = 8,                      /* invalidCiphertext        Bfv/Bfv+Multiply.swift:32-34,67-72 */
    HE_ERR_INCOMPATIBLE_CIPHERTEXTS = 9,                /* incompatibleCiphertexts  Bfv/Bfv+Multiply.swift:73-75 */
    HE_ERR_INCOMPATIBLE_CIPHERTEXT_AND_PLAINTEXT = 10,  /*                          Bfv/Bfv.swift:122-124 */
    HE_ERR_MISSING_RELINEARIZATION_KEY = 11,            /* missingRelinearizationKey Bfv/Bfv.swift:208-210 */
    HE_ERR_UNEQUAL_CONTEXTS = 12,                       /* unequalContexts          HeScheme.swift:1451-1455 */
    HE_ERR_NOT_ENOUGH_PRIMES = 13,                      /* notEnoughPrimes          Scalar.swift:147-152 */
    HE_ERR_NOT_INVERTIBLE = 14,                         /* notInvertible            Scalar.swift:79-85 */
    HE_ERR_INVALID_ENCRYPTION_PARAMETERS = 15,          /* invalidEncryptionParameters EncryptionParameters.swift:136-166 */
    HE_ERR_INVALID_ARGUMENT = 16,  /* what the reference traps on with `precondition` (null pointer, shape) */
    HE_ERR_DEVICE = 17,            /* HIP runtime failure (no GPU, out of memory, launch error) */
    HE_ERR_UNSUPPORTED = 18,       /* unsupportedHeOperation */
    HE_ERR_MISSING_GALOIS_KEY = 19, /* missingGaloisKey / missingGaloisElement  Bfv/Bfv.swift:184-189 */
    HE_ERR_SERIALIZED_BUFFER_SIZE_MISMATCH = 20, /* serializedBufferSizeMismatch  PolyRq/PolyRq+Serialize.swift:41-51 */
    HE_ERR_INVALID_COEFFICIENT_PACKING = 21,     /* invalidCoefficientPacking     CoefficientPacking.swift:27-31 */
    HE_ERR_SIMD_ENCODING_NOT_SUPPORTED = 22,     /* simdEncodingNotSupported      Encoding.swift:225 */
    /* PirError cases of ProcessedDatabase.init(from:context:) (PrivateInformationRetrieval/Util/Error.swift:32-33) */
    HE_ERR_INVALID_DATABASE_SERIALIZATION_VERSION = 23,      /* IndexPir/IndexPirProtocol.swift:307-311 */
    HE_ERR_INVALID_DATABASE_SERIALIZATION_PLAINTEXT_TAG = 24, /* IndexPir/IndexPirProtocol.swift:329-330 */
    /* PirError cases of the keyword database build (PrivateInformationRetrieval/Util/Error.swift) */
    HE_ERR_FAILED_TO_CONSTRUCT_CUCKOO_TABLE = 25,      /* failedToConstructCuckooTable  KeywordPir/CuckooTable.swift:390,408,480,486 */
    HE_ERR_INVALID_CUCKOO_CONFIG = 26,                 /* invalidCuckooConfig           KeywordPir/CuckooTable.swift:138-156 */
    HE_ERR_INVALID_HASH_BUCKET_ENTRY_VALUE_SIZE = 27,  /* invalidHashBucketEntryValueSize KeywordPir/HashBucket.swift:91-93 */
    HE_ERR_INVALID_HASH_BUCKET_SLOT_COUNT = 28,        /* invalidHashBucketSlotCount    KeywordPir/HashBucket.swift:146-148,178-181 */
    /* not an error of the reference: he_keyword_pir_cuckoo_place asks for the larger table CuckooTable.expand() would build */
    HE_ERR_CUCKOO_TABLE_NEEDS_EXPANSION = 29,          /*                               KeywordPir/CuckooTable.swift:466-474 */
    HE_ERR_INVALID_SHARDING = 30                       /* invalidSharding               KeywordPir/KeywordDatabase.swift:186-204 */
};

typedef struct he_poly_context he_poly_context; /* PolyContext<UInt64>   PolyRq/PolyContext.swift:19-35 */
typedef struct he_bfv_context he_bfv_context;   /* Context<Bfv<UInt64>>  Context.swift:19 */
typedef void* he_stream;                        /* hipStream_t; NULL = the default stream */

const char* he_status_string(int status);
/* Thread-local detail of the last failing call on this thread (HIP error text etc.); never NULL. */
const char* he_last_error_message(void);
/* Library version / build target, e.g. "he_amd 0.1 gfx950". */
const char* he_version(void);

/* ---- device plumbing (so a Swift host never has to link HIP) ---- */
int he_device_count(int* out_count);
int he_get_device(int* out_device); /* the calling thread's current HIP device: contexts and buffers belong to the device
                                     * that was current when they were created (HE_ERR_DEVICE on any other) */
int he_set_device(int device);
int he_device_malloc(void** out_ptr, size_t bytes);
int he_device_free(void* ptr);
/* (every destroy / free entry point of this header -- he_device_free, he_host_free, he_stream_destroy, he_event_destroy,
 * he_*_context_destroy, he_device_group_destroy -- may be called at any time from any thread, also while a stream of the
 * process is being captured into a graph: a deinit or finaliser cannot choose its moment, so these calls relax the calling
 * thread's capture mode for their duration instead of invalidating the capture) */
/* Page-locked host memory: a copy between it and the device is truly asynchronous (from pageable memory the runtime
 * stages the bytes before he_memcpy_h2d returns, and a borrowed pageable pointer has to be waited for).  What the Swift
 * host stages ciphertexts, keys and databases in: one copy and no wait per object instead of one per polynomial. */
int he_host_malloc(void** out_ptr, size_t bytes);
int he_host_free(void* ptr);
int he_memcpy_h2d(void* dst_device, const void* src_host, size_t bytes, he_stream stream);
int he_memcpy_d2h(void* dst_host, const void* src_device, size_t bytes, he_stream stream);
int he_stream_synchronize(he_stream stream);
int he_stream_create(he_stream* out);   /* a non-blocking HIP stream */
int he_stream_destroy(he_stream stream);
/* Scratch of the `_device` calls that take no workspace is stream-ordered and the library's own (never the process's
 * default pool): blocks from hipMalloc in a block cache inside the library.  A stream gets the blocks it released back
 * without any driver call, another stream after an event wait.  By default the cache's limit is 0: a block returns to the
 * driver (hipFree, which may wait for the device) at the first release or trim AFTER its own release has completed, so a call
 * whose scratch has another size than the last one's allocates and frees -- and the scratch of the last call stays held, however
 * long the process idles, until he_device_trim_scratch (tens of gigabytes after a batched expansion).  he_set_scratch_cache(bytes) lets the cache of the
 * current device keep up to `bytes` of released scratch (UINT64_MAX: everything); the `_device` calls are then enqueue-only
 * once their shapes have been seen.  What a server sets once (mapping tens of gigabytes per expansion costs seconds otherwise);
 * he_device_trim_scratch(keep_bytes) hands everything above `keep_bytes` back; he_scratch_cached_bytes reads what is held.
 * While a stream is being captured into a graph its scratch comes from a HIP memory pool of the library's (allocation nodes);
 * outside a capture that pool is not used: with it, a process's first call after a synchronisation has returned wrong words
 * (Scratch). */
int he_set_scratch_cache(uint64_t bytes);
int he_device_trim_scratch(uint64_t keep_bytes);
int he_scratch_cached_bytes(uint64_t* out_bytes);

/* ---- completion primitives: what the reference's `...Async` twins (HomomorphicEncryption/HeSchemeAsync.swift:16-141)
 * await.  A Swift `async` wrapper enqueues the `_device` call and then either suspends in a continuation resumed by
 * he_stream_add_callback, or records an event and polls / waits on it -- it never parks a thread of the cooperative
 * pool in he_stream_synchronize.  INTEGRATION.md section 7 and swift/Sources/HeAmd/HeAmdStream.swift show the wrapper. */
typedef void* he_event; /* hipEvent_t (timing disabled) */
typedef void (*he_host_callback)(void* user_data);
int he_event_create(he_event* out);
int he_event_destroy(he_event event);
int he_event_record(he_event event, he_stream stream);       /* marks everything enqueued on `stream` so far */
int he_event_synchronize(he_event event);                    /* blocks the calling thread */
int he_event_query(he_event event, int* out_done);           /* *out_done = 1 when the recorded work has finished */
int he_stream_wait_event(he_stream stream, he_event event);  /* later work on `stream` waits for the event (fork/join) */
/* Runs callback(user_data) on a runtime thread once everything enqueued on `stream` before this call has finished.
 * The callback must not call into this library's device entry points. */
int he_stream_add_callback(he_stream stream, he_host_callback callback, void* user_data);

/* =====================================================================================================
 * B1/B2: PolyContext and PolyRq operations
 * =================================================================================================== */

/* PolyContext.init(degree:moduli:) incl. its validation and error order (PolyRq/PolyContext.swift:45-141).
 * Builds, on the current device, the per-modulus NTT tables (_NttContext.init, PolyRq/PolyRq+Ntt.swift:118-169),
 * Barrett constants (Modulus.swift:24-45) and inverseQLast (PolyRq/PolyContext.swift:108-111). */
int he_poly_context_create(uint32_t degree, const uint64_t* moduli, uint32_t moduli_count, he_poly_context** out);
void he_poly_context_destroy(he_poly_context* ctx);
uint32_t he_poly_context_degree(const he_poly_context* ctx);
uint32_t he_poly_context_moduli_count(const he_poly_context* ctx);
int he_poly_context_moduli(const he_poly_context* ctx, uint64_t* out_moduli);
/* PolyContext.maxLazyProductAccumulationCount() (PolyRq/PolyContext.swift:246-253) */
uint64_t he_poly_context_max_lazy_product_accumulation_count(const he_poly_context* ctx);
/* PolyContext.qRemainder(dividingBy:) (PolyRq/PolyContext.swift:184-191) */
int he_poly_context_q_remainder(const he_poly_context* ctx, uint64_t modulus, uint64_t* out);
/* ScalarType.generatePrimes (Scalar.swift:113-154), for callers that build parameters host-side. */
int he_generate_primes(const int32_t* significant_bit_counts, uint32_t count, int preferring_small,
                       uint32_t ntt_degree, uint64_t* out_primes);

/* PolyRq<UInt64,Coeff>.forwardNtt() / PolyRq<UInt64,Eval>.inverseNtt() over a batch of polynomials
 * (PolyRq/PolyRq+Ntt.swift:209-232,524-543).  In place.  Throws invalidNttModulus like validateNttModuli. */
int he_ntt_forward(const he_poly_context* ctx, uint64_t* host_slab, size_t batch);
int he_ntt_inverse(const he_poly_context* ctx, uint64_t* host_slab, size_t batch);
int he_ntt_forward_device(const he_poly_context* ctx, uint64_t* device_slab, size_t batch, he_stream stream);
int he_ntt_inverse_device(const he_poly_context* ctx, uint64_t* device_slab, size_t batch, he_stream stream);
/* PolyContext.forwardNtt(dataPtr:modulus:) -- the reference's existing raw-pointer seam
 * (PolyRq/PolyRq+Ntt.swift:329-347): `rows` contiguous length-N rows, all transformed mod `modulus`, which must be
 * one of the context's moduli (else invalidPolyContext). */
int he_ntt_forward_rows_device(const he_poly_context* ctx, uint64_t modulus, uint64_t* device_rows, size_t rows,
                               he_stream stream);
int he_ntt_inverse_rows_device(const he_poly_context* ctx, uint64_t modulus, uint64_t* device_rows, size_t rows,
                               he_stream stream);

/* PolyRq += / -= / prefix - / *= (Eval) / *= [T]  (PolyRq/PolyRq.swift:147-174,299-309,184-204,232-245).
 * lhs/data are updated in place; slabs are [batch][L][N].  rhs may be lhs itself (x + x, x - x, x * x: a lane reads only the
 * words it writes); any other overlap of the two is HE_ERR_INVALID_ARGUMENT. */
int he_poly_add_device(const he_poly_context* ctx, uint64_t* lhs, const uint64_t* rhs, size_t batch, he_stream s);
int he_poly_sub_device(const he_poly_context* ctx, uint64_t* lhs, const uint64_t* rhs, size_t batch, he_stream s);
int he_poly_neg_device(const he_poly_context* ctx, uint64_t* data, size_t batch, he_stream s);
int he_poly_mul_device(const he_poly_context* ctx, uint64_t* lhs, const uint64_t* rhs, size_t batch, he_stream s);
/* scalar_residues: HOST array of L residues (y mod q_i) */
int he_poly_mul_scalar_device(const he_poly_context* ctx, uint64_t* data, const uint64_t* scalar_residues,
                              size_t batch, he_stream s);
/* PolyRq<_,Coeff>.divideAndRoundQLast() (PolyRq/PolyRq.swift:365-393): in [batch][L][N] -> out [batch][L-1][N].
 * invalidPolyContext when the context has no next (L == 1).  out overlapping in is HE_ERR_INVALID_ARGUMENT: polynomial p
 * reads rows p L .. and writes rows p (L - 1) .., which in place are rows an earlier polynomial still reads. */
int he_poly_divide_and_round_q_last_device(const he_poly_context* ctx, const uint64_t* in, uint64_t* out,
                                           size_t batch, he_stream s);
int he_poly_divide_and_round_q_last(const he_poly_context* ctx, const uint64_t* host_in, uint64_t* host_out,
                                    size_t batch);
/* PolyRq.addingLazyProduct (PolyRq/PolyRq.swift:210-225): acc[k] &+= lhs[k]*rhs[k] in wrapping UInt128.
 * acc is [L][N] UInt128 stored little-endian as (lo, hi) word pairs.  he_poly_reduce_accumulator_device is
 * Bfv.reduceToCiphertext's per-polynomial step (Bfv/Bfv.swift:380-394).  acc overlaps neither operand, out not acc. */
int he_poly_adding_lazy_product_device(const he_poly_context* ctx, const uint64_t* lhs, const uint64_t* rhs,
                                       uint64_t* acc_lo_hi, he_stream s);
int he_poly_reduce_accumulator_device(const he_poly_context* ctx, const uint64_t* acc_lo_hi, uint64_t* out,
                                      he_stream s);

/* ---- "next" rows of the scope table: index permutations; out overlapping in is HE_ERR_INVALID_ARGUMENT ---- */
/* PolyRq.applyGalois(element:) f(x) -> f(x^element) on [batch][L][N] slabs; eval_format = 0 for Coeff
 * (PolyRq/Galois.swift:115-143), 1 for Eval (PolyRq/Galois.swift:153-168).  An invalid element (even, <= 1,
 * >= 2N; Galois.swift:100-105) is the reference's precondition -> HE_ERR_INVALID_ARGUMENT. */
int he_poly_apply_galois_device(const he_poly_context* ctx, const uint64_t* in, uint64_t* out, size_t batch,
                                uint64_t element, int eval_format, he_stream s);
/* PolyRq<Coeff>.multiplyPowerOfX(power) (PolyRq/PolyRq.swift:398-422): f(x) x^power mod (x^N + 1), any sign. */
int he_poly_multiply_power_of_x_device(const he_poly_context* ctx, const uint64_t* in, uint64_t* out, size_t batch,
                                       int64_t power, he_stream s);

/* ---- wire format: PolyRq.serialize / PolyRq(deserialize:) on device buffers ----
 * Each residue row is a big-endian bit stream of N coefficients, ceilLog2(q_r) - skip_lsbs bits each, zero-padded
 * to a byte; rows follow one another (CoefficientPacking.swift:169-213, PolyRq/PolyRq+Serialize.swift:69-99).
 * he_poly_serialization_byte_count = PolyContext.serializationByteCount(skipLSBs:) (0 on invalid arguments).
 * device_bytes is [batch][byte count] (serialize) / [batch][bytes_per_poly] (deserialize; the leading byte count
 * of each record is read, a shorter record is serializedBufferSizeMismatch).  The bytes and the slab of a call do not overlap
 * (HE_ERR_INVALID_ARGUMENT), here and in the seeded, the ciphertext and the 4-byte forms below. */
size_t he_poly_serialization_byte_count(const he_poly_context* ctx, int skip_lsbs);
int he_poly_serialize_device(const he_poly_context* ctx, const uint64_t* device_slab, size_t batch, int skip_lsbs,
                             uint8_t* device_bytes, he_stream s);
int he_poly_deserialize_device(const he_poly_context* ctx, const uint8_t* device_bytes, size_t bytes_per_poly,
                               size_t batch, int skip_lsbs, uint64_t* device_slab, he_stream s);

/* The second polynomial of a seeded ciphertext (SerializedCiphertext.swift:53-58, Bfv/Bfv+Encrypt.swift:155-156):
 * device_slab[b] = PolyRq<UInt64, Eval>.random(context:using: NistAes128Ctr(seed: device_seeds[b])), seeds are
 * [batch][32] bytes (NistCtrDrbg.SeedCount).  NIST SP 800-90A CTR_DRBG/AES-128 as Random/NistCtrDrbg.swift has it,
 * 4096-byte refills (Random/NistAes128Ctr.swift), 128 stream bits per coefficient reduced mod q_i
 * (PolyRq/PolyRq+Randomize.swift:56-75).  A Coeff ciphertext then takes he_ntt_inverse_device of the result. */
int he_poly_random_from_seeds_device(const he_poly_context* ctx, const uint8_t* device_seeds, size_t batch,
                                     uint64_t* device_slab, he_stream s);

/* ---- PolyRq<UInt32> (polynomial layer): the same operations on slabs of 4-byte words ----
 * The context is an ordinary he_poly_context whose moduli all fit UInt32 (<= 2^30 - 1, ModularArithmetic/
 * Scalar.swift:498-511; e.g. the n_4096_logq_27_28_28 parameter sets, EncryptionParameters.swift:313-378); a larger
 * modulus returns HE_ERR_INVALID_MODULUS.  Layout [batch][L][N] of uint32_t; semantics as the UInt64 entry points
 * (the reference's generic code is the same for both word types).  Degrees above 32768: HE_ERR_UNSUPPORTED. */
int he_ntt_forward_device_u32(const he_poly_context* ctx, uint32_t* device_slab, size_t batch, he_stream s);
int he_ntt_inverse_device_u32(const he_poly_context* ctx, uint32_t* device_slab, size_t batch, he_stream s);
int he_poly_add_device_u32(const he_poly_context* ctx, uint32_t* lhs, const uint32_t* rhs, size_t batch, he_stream s);
int he_poly_sub_device_u32(const he_poly_context* ctx, uint32_t* lhs, const uint32_t* rhs, size_t batch, he_stream s);
int he_poly_neg_device_u32(const he_poly_context* ctx, uint32_t* data, size_t batch, he_stream s);
int he_poly_mul_device_u32(const he_poly_context* ctx, uint32_t* lhs, const uint32_t* rhs, size_t batch, he_stream s);
int he_poly_mul_scalar_device_u32(const he_poly_context* ctx, uint32_t* data, const uint32_t* scalar_residues,
                                  size_t batch, he_stream s);
int he_poly_divide_and_round_q_last_device_u32(const he_poly_context* ctx, const uint32_t* in, uint32_t* out, size_t batch,
                                               he_stream s);

/* The wire entries above on slabs of 4-byte words: the same contracts, widths at most 30 (HE_ERR_INVALID_MODULUS for a larger
 * modulus).  4-byte slabs take the 8-bytes-per-lane and the byte kernels (he_ciphertexts_wire_plan with poly_count 0 says which). */
int he_poly_serialize_device_u32(const he_poly_context* ctx, const uint32_t* device_slab, size_t batch, int skip_lsbs,
                                 uint8_t* device_bytes, he_stream s);
int he_poly_deserialize_device_u32(const he_poly_context* ctx, const uint8_t* device_bytes, size_t bytes_per_poly,
                                   size_t batch, int skip_lsbs, uint32_t* device_slab, he_stream s);
int he_poly_random_from_seeds_device_u32(const he_poly_context* ctx, const uint8_t* device_seeds, size_t batch,
                                         uint32_t* device_slab, he_stream s);

/* ---- wire format of whole ciphertexts: seeded in, forDecryption out, `count` per call ----
 * A record is the `polys` bytes of the reference's SerializedCiphertext.full: the polynomial count as a little-endian UInt16,
 * then PolyRq.serialize(skipLSBs[p]) of each polynomial (Serialize.swift:31-94, SerializedCiphertext.swift:126-147).  Record i
 * lies at records + i * record_stride (any stride >= the byte count, any address); its ciphertext is cts[i] of
 * [count][poly_count][L][N].  ctx is the he_poly_context of the ciphertext's level (keys: the key-switching context and its
 * L + 1 moduli); the _u32 forms take packed 4-byte slabs over a context whose moduli fit UInt32.  skip_lsbs is a HOST array
 * of poly_count entries, NULL = zeros.  Errors: HE_ERR_UNSUPPORTED for poly_count outside 1..3 (no reference ciphertext has
 * more), HE_ERR_INVALID_COEFFICIENT_PACKING per polynomial as he_poly_serialize_device reports it,
 * HE_ERR_SERIALIZED_BUFFER_SIZE_MISMATCH for a stride below the byte count.  All enqueue-only on `s`. */

/* Bfv.skipLSBsForDecryption (Bfv/Bfv+Decrypt.swift:51-109): the skips of a reply's two polynomials, from the degree, the first
 * coefficient modulus, the plaintext modulus and the ciphertext's modulus count ({0, 0} unless that is 1).  Host only. */
int he_bfv_skip_lsbs_for_decryption(uint32_t degree, uint64_t q0, uint64_t plaintext_modulus, uint32_t moduli_count,
                                    int out_skip_lsbs[2]);
/* Serialize.serializePolysBufferSize: 2 + the sum of serializationByteCount(skipLSBs[p]); 0 on invalid arguments.  Host only. */
size_t he_ciphertexts_serialization_byte_count(const he_poly_context* ctx, uint32_t poly_count, const int* skip_lsbs);
/* Which kernel form a wire call takes, without a device (csrc/ciphertext_wire_form.hpp, csrc/serialize_form.hpp).
 * direction 0 = serialize, 1 = deserialize; word_bits 32 or 64; the addresses are the two buffers' as integers.
 * poly_count 1..3: the ciphertext entries below -- form 3 ("chunk": a lane owns an aligned 8-byte chunk of the records
 * buffer, byte stores where a chunk holds a record's first or last bytes) for serialize, 4 ("field": a lane owns a
 * coefficient and reads the aligned 8-byte words around its field) for deserialize; items_per_record is the lanes' index
 * space per record and edge_free says that the record pointer and stride are multiples of 8.
 * poly_count 0: the polynomial-level entries (skip_lsbs[0]; record_stride = bytes_per_poly, ignored for serialize) -- form
 * 0 byte, 1 word, 2 tile.  Any out pointer may be NULL.  Errors as the calls themselves report them. */
int he_ciphertexts_wire_plan(int direction, uint32_t word_bits, const he_poly_context* ctx, uint32_t poly_count,
                             const int* skip_lsbs, size_t record_stride, uint64_t records_address, uint64_t slab_address,
                             uint32_t* out_form, size_t* out_record_bytes, size_t* out_items_per_record,
                             uint32_t* out_edge_free);
/* Ciphertext.serialize(forDecryption:) per ciphertext.  Bytes between a record's byte count and the stride, and everything
 * outside the records, are not written (nor read). */
int he_ciphertexts_serialize_device(const he_poly_context* ctx, const uint64_t* cts, size_t count, uint32_t poly_count,
                                    const int* skip_lsbs, uint8_t* records, size_t record_stride, he_stream s);
int he_ciphertexts_serialize_device_u32(const he_poly_context* ctx, const uint32_t* cts, size_t count, uint32_t poly_count,
                                        const int* skip_lsbs, uint8_t* records, size_t record_stride, he_stream s);
/* Ciphertext(deserialize: .full) per record.  Nothing outside [records, records + (count - 1) * record_stride + byte count)
 * is read; fields are not validated (as he_poly_deserialize_device).  The reference takes the polynomial count from the
 * buffer and throws on a mismatch; a kernel cannot, so device_header_mismatch (optional, a DEVICE word the caller has zeroed)
 * is set to 1 when some record's header differs from poly_count -- every record is still decoded as poly_count polynomials. */
int he_ciphertexts_deserialize_device(const he_poly_context* ctx, const uint8_t* records, size_t record_stride, size_t count,
                                      uint32_t poly_count, const int* skip_lsbs, uint64_t* cts,
                                      uint32_t* device_header_mismatch, he_stream s);
int he_ciphertexts_deserialize_device_u32(const he_poly_context* ctx, const uint8_t* records, size_t record_stride,
                                          size_t count, uint32_t poly_count, const int* skip_lsbs, uint32_t* cts,
                                          uint32_t* device_header_mismatch, he_stream s);
/* Ciphertext(deserialize: .seeded(poly0:seed:)) (SerializedCiphertext.swift:53-60) into cts [count][2][L][N]: slot 0 =
 * PolyRq(deserialize:) of poly0_bytes + i * record_stride (bare polynomial records, no header, stride >=
 * he_poly_serialization_byte_count(ctx, 0)); slot 1 = PolyRq<_, Eval>.random(NistAes128Ctr(seed: seeds[i])), seeds
 * [count][32], inverse-transformed when coeff_format != 0 (queries; key-switching keys are Eval).  Both kernels write at
 * ciphertext stride: no staging slab, no copy.  poly0_bytes == NULL leaves every slot 0 untouched, seeds == NULL every slot 1.
 * coeff_format != 0 enqueues one inverse transform per ciphertext after the two launches; a context with a modulus that is no
 * NTT modulus (HE_ERR_INVALID_NTT_MODULUS) or, on 4-byte words, a degree above 32768 (HE_ERR_UNSUPPORTED) is refused before
 * anything is enqueued. */
int he_ciphertexts_deserialize_seeded_device(const he_poly_context* ctx, const uint8_t* poly0_bytes, size_t record_stride,
                                             const uint8_t* seeds, size_t count, int coeff_format, uint64_t* cts,
                                             he_stream s);
int he_ciphertexts_deserialize_seeded_device_u32(const he_poly_context* ctx, const uint8_t* poly0_bytes, size_t record_stride,
                                                 const uint8_t* seeds, size_t count, int coeff_format, uint32_t* cts,
                                                 he_stream s);

/* =====================================================================================================
 * B3: Context<Bfv<UInt64>> and the HeScheme operations on the hot path
 * =================================================================================================== */

/* Context.init(encryptionParameters:) with EncryptionParameters' own checks at securityLevel .unchecked
 * (Context.swift:94-143, EncryptionParameters.swift:136-166).  The last coefficient modulus is the key-switching
 * modulus when more than one is given.  Builds the ciphertext / key-switching PolyContexts and one _RnsTool per
 * level (RnsTool.swift:132-251) incl. the Bsk primes (RnsTool.swift:28-45). */
int he_bfv_context_create(uint32_t degree, uint64_t plaintext_modulus, const uint64_t* coefficient_moduli,
                          uint32_t moduli_count, he_bfv_context** out);
void he_bfv_context_destroy(he_bfv_context* ctx);
uint32_t he_bfv_ciphertext_moduli_count(const he_bfv_context* ctx); /* L of a fresh ciphertext */
/* Borrowed sub-contexts (valid while ctx lives); moduli_count in 1..L. NULL when out of range. */
const he_poly_context* he_bfv_ciphertext_context(const he_bfv_context* ctx, uint32_t moduli_count);
const he_poly_context* he_bfv_key_switching_context(const he_bfv_context* ctx, uint32_t moduli_count);
const he_poly_context* he_bfv_qbsk_context(const he_bfv_context* ctx, uint32_t moduli_count);

/* _RnsTool pieces, exposed so each can be parity-tested on its own (RnsTool.swift):
 *   liftQToQBsk  :324-331  in [batch][L][N]    -> out [batch][2L+1][N]
 *   floorQBskToQ :453-456  in [batch][2L+1][N] -> out [batch][L][N]
 * out overlapping in is HE_ERR_INVALID_ARGUMENT (a polynomial's rows lie at different strides in the two). */
int he_rns_lift_q_to_qbsk_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* in, uint64_t* out,
                                 size_t batch, he_stream s);
int he_rns_floor_qbsk_to_q_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* in, uint64_t* out,
                                  size_t batch, he_stream s);

/* Workspace: multi-kernel operations need device scratch.  Pass workspace == NULL to let the library allocate
 * stream-ordered scratch itself (from its own pool or block cache: he_set_scratch_cache, above); otherwise pass at least
 * *_workspace_bytes().  The workspace is written: [workspace, workspace + workspace_bytes) overlapping any other slab of the
 * call is HE_ERR_INVALID_ARGUMENT. */
size_t he_bfv_mul_workspace_bytes(const he_bfv_context* ctx, uint32_t moduli_count, size_t batch);
size_t he_bfv_relinearize_workspace_bytes(const he_bfv_context* ctx, uint32_t moduli_count, size_t batch);

/* Bfv.mulAssign(_: inout CanonicalCiphertext, _: CanonicalCiphertext) = multiplyWithoutScaling + dropExtendedBase
 * (Bfv/Bfv+Multiply.swift:18-85).  lhs, rhs: [batch][2][L][N] Coeff; out: [batch][3][L][N] Coeff, overlapping neither
 * operand (HE_ERR_INVALID_ARGUMENT: parts of the batch are stored while others are still read); lhs and rhs may be one
 * ciphertext.  Enqueue-only on `s` as seen
 * from the caller: large batches also run part of the pipeline on a second stream the context owns, forked off `s` and joined
 * back into `s` by events before the call returns (not while `s` is being captured into a graph).  The context keeps up to 8
 * such streams and gives each caller stream the one it used last, so calls on different streams do not queue behind one
 * another's backlog; a call that finds all of them taken runs entirely on `s`. */
int he_bfv_mul_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* lhs, const uint64_t* rhs,
                      uint64_t* out, size_t batch, void* workspace, size_t workspace_bytes, he_stream s);
/* Bfv.relinearize (Bfv/Bfv.swift:201-219) via _computeKeySwitchingUpdate (Bfv/Bfv+Keys.swift:123-208).
 * ct3: [batch][3][L][N] Coeff; key: the relinearization key's L_top ciphertexts, [L_top][2][L_top+1][N] Eval over
 * the top key-switching context (Keys.swift:66-99); out: [batch][2][L][N] Coeff, not overlapping ct3 (the last kernel adds
 * the update to (c0, c1) as it reads them, item by item in no particular order): an overlap is HE_ERR_INVALID_ARGUMENT,
 * except a single ciphertext (batch == 1) relinearized onto its own first two polynomials (out == ct3).  key == NULL ->
 * missingRelinearizationKey. */
int he_bfv_relinearize_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* ct3,
                              const uint64_t* key, uint64_t* out, size_t batch, void* workspace,
                              size_t workspace_bytes, he_stream s);
/* Bfv.modSwitchDown (Bfv/Bfv.swift:163-171): [batch][polys][L][N] -> [batch][polys][L-1][N]; out overlapping in is
 * HE_ERR_INVALID_ARGUMENT, as for he_poly_divide_and_round_q_last_device. */
int he_bfv_mod_switch_down_device(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count,
                                  const uint64_t* in, uint64_t* out, size_t batch, he_stream s);
/* Ciphertext.modSwitchDownToSingle (Bfv/Bfv.swift:163-171): in [batch][polys][moduli_count][N] -> out [batch][polys][1][N],
 * the moduli_count - 1 divideAndRoundQLast steps in one kernel (word for word the chain of he_bfv_mod_switch_down_device).
 * out overlapping in is HE_ERR_INVALID_ARGUMENT, except out == in at moduli_count == 1, where the ciphertext is already
 * there and nothing is done. */
int he_bfv_mod_switch_down_to_single_device(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count,
                                            const uint64_t* in, uint64_t* out, size_t batch, he_stream s);
/* Bfv.mulAssign(_: inout EvalCiphertext, _: EvalPlaintext) (Bfv/Bfv.swift:120-129):
 * ct [batch][polys][L][N] *= pt [batch][L][N].  pt may be ct itself for batch == 1 (the ciphertext times its own first
 * polynomial) or poly_count == 1 (squares): a lane then reads only words it writes; any other overlap is
 * HE_ERR_INVALID_ARGUMENT. */
int he_bfv_mul_plain_device(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, uint64_t* ct,
                            const uint64_t* pt, size_t batch, he_stream s);
/* Bfv.addAssignCoeff / subAssignCoeff(_: inout CoeffCiphertext, _: CoeffPlaintext) (Bfv/Bfv.swift:110-117), i.e.
 * plaintextTranslate (Bfv/Bfv+Encrypt.swift:75-140): c0 +-= floor(Q/t) m + floor(((Q mod t) m + (t + 1)/2) / t) per
 * residue row.  ct [batch][polys][L][N] Coeff in place (only c0 is touched), plaintexts [batch][N] Coeff plaintexts
 * with values < t (batch b's plaintext goes to batch b's ciphertext).  `plaintext - ciphertext`
 * (HeScheme.swift:1540-1548) is he_poly_neg_device over the ciphertext's polynomials, then this add.  plaintexts overlapping
 * ct is HE_ERR_INVALID_ARGUMENT. */
int he_bfv_add_plain_device(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, uint64_t* ct,
                            const uint64_t* plaintexts, size_t batch, he_stream s);
int he_bfv_sub_plain_device(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, uint64_t* ct,
                            const uint64_t* plaintexts, size_t batch, he_stream s);
/* Bfv.innerProduct(ciphertexts:plaintexts:) (Bfv/Bfv.swift:476-505), batched over `columns` independent outputs
 * that share the ciphertext vector (the PIR dim-0 shape, PrivateInformationRetrieval/IndexPir/PirUtil.swift:427-445):
 *   cts      [count][polys][L][N]           Eval
 *   pts      [columns][count][L][N]         Eval plaintexts over the ciphertext context
 *   present  HOST [columns][count] bytes, 0 = nil plaintext (skipped, Bfv.swift:494); NULL = all present
 *   out      [columns][polys][L][N]         Eval
 * Every word must be a canonical residue (< q_i), as the reference's polynomials are: the accumulators count on it.
 * polys = 1, 2 or 3 polynomials per ciphertext -- or 4, 6, 8: the ciphertext vectors of 2, 3 or 4 QUERIES laid side by
 * side ([count][query][2][L][N]), which then share every plaintext word the kernel streams (out [columns][query][2]
 * [L][N]): a server that answers several queries over one database reads the database once for all of them.
 * out overlaps none of cts, pts and the device mask (HE_ERR_INVALID_ARGUMENT), here and in the resident and packed forms;
 * he_bfv_pack_plaintexts_device refuses packed overlapping plaintexts_eval. */
int he_bfv_inner_product_plain_device(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count,
                                      const uint64_t* cts, const uint64_t* pts, const uint8_t* present, size_t count,
                                      size_t columns, uint64_t* out, he_stream s);
/* The same with the mask resident on the DEVICE (NULL = all present): enqueue-only, never synchronises, may be
 * captured into a HIP graph.  (The host-mask form above waits once for the upload of the borrowed mask.) */
int he_bfv_inner_product_plain_resident_device(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count,
                                               const uint64_t* cts, const uint64_t* pts, const uint8_t* present_device,
                                               size_t count, size_t columns, uint64_t* out, he_stream s);
/* The plaintexts without the zero top bits of their words -- a layout private to this library for databases that stay
 * resident in HBM (the ct x pt inner product is bound by the bytes of plaintext it streams): row r of a plaintext is a
 * little-endian bit stream of N fields of bits(q_r) bits, rows in whole 8-byte words; a 55-bit modulus takes 6.875 bytes
 * per word instead of 8.  Degree >= 256, at most 8 moduli.
 *   he_bfv_packed_plaintext_words     8-byte words per packed plaintext (0: unsupported parameters)
 *   he_bfv_pack_plaintexts_device     plaintexts_eval [count][L][N] -> packed [count][words]
 *   he_bfv_inner_product_plain_packed_device   he_bfv_inner_product_plain_resident_device with pts packed
 *       ([columns][count][words]; polys 1..3); the same words out. */
size_t he_bfv_packed_plaintext_words(const he_bfv_context* ctx, uint32_t moduli_count);
int he_bfv_pack_plaintexts_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* plaintexts_eval,
                                  size_t count, uint64_t* packed, he_stream s);
int he_bfv_inner_product_plain_packed_device(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count,
                                             const uint64_t* cts, const uint64_t* packed_pts, const uint8_t* present_device,
                                             size_t count, size_t columns, uint64_t* out, he_stream s);
/* Bfv.innerProduct(_: [CanonicalCiphertext], _: [CanonicalCiphertext]) (Bfv/Bfv.swift:315-361):
 * lhs, rhs [count][2][L][N] Coeff -> out [3][L][N] Coeff.  lhs and rhs may be one vector; out and the workspace overlap
 * neither (HE_ERR_INVALID_ARGUMENT). */
int he_bfv_inner_product_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* lhs,
                                const uint64_t* rhs, size_t count, uint64_t* out, void* workspace,
                                size_t workspace_bytes, he_stream s);
size_t he_bfv_inner_product_workspace_bytes(const he_bfv_context* ctx, uint32_t moduli_count, size_t count);
/* `items` such inner products that share their left vector -- the remaining-dimension step of a PIR response over all
 * result groups of all chunks (PirUtil.swift:448-479): lhs [count][2][L][N], rhs [items][count][2][L][N] Coeff ->
 * out [items][3][L][N] Coeff.  Item i equals he_bfv_inner_product_device(lhs, rhs + i * count ciphertexts); every stage is
 * one launch over all items and the left vector is lifted and transformed once.  Stream-ordered scratch.  lhs may be an
 * item of rhs; out overlaps neither (HE_ERR_INVALID_ARGUMENT). */
int he_bfv_inner_product_shared_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* lhs,
                                       const uint64_t* rhs, size_t count, size_t items, uint64_t* out, he_stream s);

/* Context<Bfv<UInt32>> (scheme layer): the word type fixes the largest modulus (2^30 - 1), gamma =
 * 2^30 - 20405, mTilde = 2^16 and the 29-bit Bsk primes (ModularArithmetic/Scalar.swift:498-511,
 * RnsTool.swift:30-33).  Results equal the reference's Bfv<UInt32> words exactly. */
int he_bfv_context_create_u32(uint32_t degree, uint64_t plaintext_modulus, const uint64_t* coefficient_moduli,
                              uint32_t moduli_count, he_bfv_context** out);
/* The scheme operations on PACKED [UInt32] slabs -- what Swift's Bfv<UInt32> holds (its PolyRq arrays are [UInt32]).
 * Same layouts, arguments, errors and citations as the entry points of the same name without the suffix, every slab
 * (ciphertexts, keys, plaintexts, workspaces) in 4-byte words; the context must come from he_bfv_context_create_u32.
 * The BEHZ / key-switching / inner-product kernels are the 8-byte ones instantiated on 4-byte slabs (a word is widened
 * in its register, never in memory); the transforms are the 4-byte NTT kernels (he_ntt_*_device_u32).  Workspaces: half
 * the bytes the he_bfv_*_workspace_bytes functions report, or NULL for stream-ordered scratch. */
int he_rns_lift_q_to_qbsk_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* in, uint32_t* out,
                                     size_t batch, he_stream s);
int he_rns_floor_qbsk_to_q_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* in,
                                      uint32_t* out, size_t batch, he_stream s);
int he_rns_scale_and_round_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* in,
                                      uint64_t scaling_factor, uint32_t* out, size_t batch, he_stream s);
int he_bfv_mul_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* lhs, const uint32_t* rhs,
                          uint32_t* out, size_t batch, void* workspace, size_t workspace_bytes, he_stream s);
int he_bfv_relinearize_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* ct3,
                                  const uint32_t* key, uint32_t* out, size_t batch, void* workspace,
                                  size_t workspace_bytes, he_stream s);
int he_bfv_apply_galois_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* ct, uint64_t element,
                                   const uint32_t* galois_key, uint32_t* out, size_t batch, void* workspace,
                                   size_t workspace_bytes, he_stream s);
int he_bfv_mod_switch_down_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count,
                                      const uint32_t* in, uint32_t* out, size_t batch, he_stream s);
int he_bfv_mul_plain_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, uint32_t* ct,
                                const uint32_t* pt, size_t batch, he_stream s);
int he_bfv_add_plain_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, uint32_t* ct,
                                const uint32_t* plaintexts, size_t batch, he_stream s);
int he_bfv_sub_plain_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count, uint32_t* ct,
                                const uint32_t* plaintexts, size_t batch, he_stream s);
int he_bfv_inner_product_plain_resident_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, uint32_t poly_count,
                                                   const uint32_t* cts, const uint32_t* pts,
                                                   const uint8_t* present_device, size_t count, size_t columns,
                                                   uint32_t* out, he_stream s);
int he_bfv_inner_product_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* lhs,
                                    const uint32_t* rhs, size_t count, uint32_t* out, void* workspace,
                                    size_t workspace_bytes, he_stream s);
int he_bfv_inner_product_shared_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* lhs,
                                           const uint32_t* rhs, size_t count, size_t items, uint32_t* out, he_stream s);
/* he_pir_compute_response_device on packed 4-byte slabs (query, database, key and responses in UInt32 words): the PIR
 * parameter sets with 27/28-bit moduli (EncryptionParameters.swift:313-345) stream half the database bytes of the
 * 8-byte route.  Same shapes, same words as the reference's Bfv<UInt32>.  Enqueue-only. */
int he_pir_compute_response_device_u32(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count,
                                       const uint32_t* dim0_query_eval, const uint32_t* remaining_query,
                                       size_t remaining_query_count, const uint32_t* database,
                                       const uint8_t* present_device, size_t chunk_count,
                                       const uint32_t* relinearization_key, uint32_t* out, he_stream s);
/* he_pir_compute_response_queries_device on packed 4-byte slabs (a Bfv<UInt32> context): 1..4 queries share one pass
 * over the 4-byte database; layouts as there, 4-byte words. */
int he_pir_compute_response_queries_device_u32(const he_bfv_context* ctx, const uint32_t* dimensions,
                                               uint32_t dimension_count, size_t queries, const uint32_t* dim0_queries_eval,
                                               const uint32_t* remaining_queries, size_t remaining_query_count,
                                               const uint32_t* database, const uint8_t* present_device, size_t chunk_count,
                                               const uint32_t* const* relinearization_keys, uint32_t* out, he_stream s);
/* he_pir_compute_response_to_query_device for Bfv<UInt32> on packed 4-byte slabs (query, relinearization key, databases,
 * responses in UInt32 words).  The expansion, which is bound by its key switches and not by bytes, runs on widened words:
 * galois_keys_wide are the Galois keys as 8-byte slabs (he_words_widen_u32_device), as he_pir_expand_device takes them for
 * a UInt32 context.  Indices that share the database share its pass four at a time. */
int he_pir_compute_response_to_query_device_u32(const he_bfv_context* ctx, const uint32_t* dimensions,
                                                uint32_t dimension_count, const uint32_t* query_ciphertexts,
                                                size_t query_ciphertext_count, size_t indices_count,
                                                const uint64_t* galois_elements, const uint64_t* const* galois_keys_wide,
                                                size_t galois_key_count, const uint32_t* relinearization_key,
                                                const uint32_t* const* databases, const uint8_t* const* present_masks,
                                                size_t database_count, size_t chunk_count, uint32_t* out, he_stream s);
int he_bfv_plaintext_to_eval_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* plaintext,
                                        uint32_t* out, size_t batch, he_stream s);
int he_bfv_plaintext_to_coeff_device_u32(const he_bfv_context* ctx, uint32_t moduli_count, const uint32_t* plaintext_eval,
                                         uint32_t* out, size_t batch, he_stream s);
/* A Bfv<UInt32> context also works with every 8-byte entry point (he_bfv_*, he_rns_*, he_pir_*) on slabs of
 * zero-extended words; the PIR hooks (he_pir_*) exist in that form only.  Word-size bridge: widen a packed slab to
 * zero-extended 8-byte words and narrow results back (values of a UInt32 context are < 2^30, so the low half is the
 * word).  `words` counts coefficients; slabs 16-byte aligned; device_out overlapping device_in is HE_ERR_INVALID_ARGUMENT
 * (word k is read at 4 k and stored at 8 k), for he_words_copy_device too. */
int he_words_widen_u32_device(const uint32_t* device_in, uint64_t* device_out, size_t words, he_stream s);
int he_words_narrow_u64_device(const uint64_t* device_in, uint32_t* device_out, size_t words, he_stream s);

/* ---- "next" rows of the scope table ---- */
/* Bfv.applyGalois(ciphertext:element:using:) (Bfv/Bfv.swift:174-198): ct [batch][2][L][N] Coeff,
 * galois_key = EvaluationKey.galoisKey.keys[element] in the relinearization key's layout
 * ([L_top][2][L_top+1][N] Eval; Bfv+Keys.swift:38-45,69-103) -> out [batch][2][L][N] Coeff.
 * NULL key -> HE_ERR_MISSING_GALOIS_KEY.  out may be ct itself (ct is permuted into the workspace before the first word of
 * out is stored); any other overlap of out or the workspace with ct, the key or one another is HE_ERR_INVALID_ARGUMENT. */
int he_bfv_apply_galois_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* ct,
                               uint64_t element, const uint64_t* galois_key, uint64_t* out, size_t batch,
                               void* workspace, size_t workspace_bytes, he_stream s);
/* GaloisElement.swappingRows(degree:) and GaloisElement.rotatingColumns(by:degree:) (PolyRq/Galois.swift:174-212): the
 * elements Bfv.swapRows / Bfv.rotateColumns hand to applyGalois (HeScheme.swift:1047-1094).  step > 0 rotates right,
 * < 0 left, |step| in [1, N/2 - 1] (else HE_ERR_INVALID_ARGUMENT = invalidRotationStep); degree a power of two. */
int he_galois_element_swapping_rows(uint64_t degree, uint64_t* out_element);
int he_galois_element_rotating_columns(int64_t step, uint64_t degree, uint64_t* out_element);
/* Bfv.applyGalois on a batch whose items belong to different evaluation keys: `groups` runs of `group_size` consecutive
 * ciphertexts, group g under galois_keys[g] (host array of device pointers, he_bfv_apply_galois_device's key layout).
 * Workspace as he_bfv_apply_galois_workspace_bytes(ctx, moduli_count, groups * group_size). */
int he_bfv_apply_galois_grouped_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* ct,
                                       uint64_t element, const uint64_t* const* galois_keys, size_t groups,
                                       size_t group_size, uint64_t* out, void* workspace, size_t workspace_bytes,
                                       he_stream s);
size_t he_bfv_apply_galois_workspace_bytes(const he_bfv_context* ctx, uint32_t moduli_count, size_t batch);
/* _RnsTool.scaleAndRound(poly:scalingFactor:) (RnsTool.swift:272-302), the RNS step of Bfv.decrypt
 * (Bfv/Bfv+Decrypt.swift): in [batch][L][N] Coeff (c0 + c1 s [+ c2 s^2]) -> out [batch][N], values < t.
 * scaling_factor < t (the ciphertext's correction factor).  out overlapping in is HE_ERR_INVALID_ARGUMENT, as it is for the
 * two plaintext conversions below (L rows on one side, one row on the other). */
int he_rns_scale_and_round_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* in,
                                  uint64_t scaling_factor, uint64_t* out, size_t batch, he_stream s);
/* Plaintext<Coeff>.convertToEvalFormat(moduliCount:) (Plaintext.swift:149-170): plaintext [batch][N] (values < t)
 * -> out [batch][L][N] Eval.  This is the database preprocessing step of PIR (MulPir.swift:507-556). */
int he_bfv_plaintext_to_eval_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* plaintext,
                                    uint64_t* out, size_t batch, he_stream s);
/* Plaintext<Eval>.convertToCoeffFormat() (Plaintext.swift:176-191): [batch][L][N] Eval -> [batch][N] (values < t). */
int he_bfv_plaintext_to_coeff_device(const he_bfv_context* ctx, uint32_t moduli_count, const uint64_t* plaintext_eval,
                                     uint64_t* out, size_t batch, he_stream s);

/* ---- decryption of resident ciphertexts: plaintexts, noise budgets, transparency ----
 * The entries below take the slab word as an argument (word_bits 32 or 64, as he_ciphertexts_wire_plan does; 4-byte slabs
 * need a context from he_bfv_context_create_u32) and have no _u32 twins.  Common to all of them:
 *   cts         [batch][poly_count][L][N], L = moduli_count, Eval form when is_eval != 0, else Coeff; never written
 *   secret_key  [L_all][N] Eval over the secret-key context (every coefficient modulus); its first L rows are read
 *               (PolyRq.mulAssign(secretPoly:), PolyRq/PolyRq.swift:184-194)
 *   workspace   NULL = stream-ordered scratch, else at least he_bfv_decrypt_workspace_bytes() bytes, 16-byte aligned
 * The result slab and the workspace overlap neither cts nor secret_key nor one another (HE_ERR_INVALID_ARGUMENT).
 * Errors: word_bits other than 32 / 64 and moduli_count outside 1..he_bfv_ciphertext_moduli_count are
 * HE_ERR_INVALID_ARGUMENT, poly_count outside 1..3 is HE_ERR_UNSUPPORTED (no reference ciphertext has more); batch 0 does
 * nothing.  All enqueue-only on `s`. */
/* The scratch of the three entries that take a workspace (0 on invalid arguments).  Host only. */
size_t he_bfv_decrypt_workspace_bytes(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, uint32_t poly_count,
                                      int is_eval, size_t batch);
/* Bfv.dotProduct (Bfv/Bfv+Decrypt.swift:188-204): out [batch][L][N] Coeff = c0 + c1 s [+ c2 s^2].  Every ciphertext word is
 * read once by one kernel; s^2 is formed in registers and never stored.  Of Coeff-form input the polynomials behind the first
 * are copied into the workspace and transformed there; c0 joins after the inverse transform (the transform is linear). */
int he_bfv_secret_dot_product_device(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, uint32_t poly_count,
                                     int is_eval, const void* cts, const void* secret_key, void* out, size_t batch,
                                     void* workspace, size_t workspace_bytes, he_stream s);
/* Bfv.decryptCoeff / decryptEval (Bfv/Bfv+Decrypt.swift:21-39): out_plaintexts [batch][N] in slab words, values < t.  The
 * scaling factor of scaleAndRound is correction_factor^-1 mod t, computed on the host: a factor without an inverse is
 * HE_ERR_NOT_INVERTIBLE, one that is not below t HE_ERR_INVALID_ARGUMENT. */
int he_bfv_decrypt_device(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, uint32_t poly_count, int is_eval,
                          const void* cts, const void* secret_key, uint64_t correction_factor, void* out_plaintexts,
                          size_t batch, void* workspace, size_t workspace_bytes, he_stream s);
/* The integer behind Bfv.noiseBudgetCoeff / noiseBudgetEval (Bfv/Bfv+Decrypt.swift:116-149): per ciphertext the exact
 * max_k |[t dot_k]_Q|, each composed coefficient (CrtComposer.swift:76-97) centred as `coeff > (Q + 1) >> 1 ? Q - coeff : coeff`.
 * out_limbs [batch][he_bfv_noise_norm_limbs()] little-endian 64-bit limbs (a DEVICE array).  At most 16 moduli. */
int he_bfv_noise_norm_device(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, uint32_t poly_count,
                             int is_eval, const void* cts, const void* secret_key, uint64_t* out_limbs, size_t batch,
                             void* workspace, size_t workspace_bytes, he_stream s);
/* Bfv.isTransparentCoeff / isTransparentEval (Bfv/Bfv+Encrypt.swift:48-62): out_flags[b] (a DEVICE byte) = 1 iff every
 * polynomial of ciphertext b but the first is zero (poly_count 1: always 1). */
int he_bfv_is_transparent_device(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, uint32_t poly_count,
                                 const void* cts, uint8_t* out_flags, size_t batch, he_stream s);
/* ceil(bitlength(q_0 .. q_{L-1}) / 64), 1..16; 0 on invalid arguments.  Host only. */
uint32_t he_bfv_noise_norm_limbs(const he_bfv_context* ctx, uint32_t moduli_count);
/* The noise budget of one norm (`limbs`: a HOST array of he_bfv_noise_norm_limbs() limbs), Bfv/Bfv+Decrypt.swift:144-148:
 * +infinity for 0, else log2(qDouble / (2 Double(norm))) with qDouble the left-to-right product of the Double(q_i) from 1.0 and
 * Double(norm) rounded to nearest, ties to even.  word_bits is the width of the scheme's scalar T: when
 * crtComposeMaxIntermediateValue() (CrtComposer.swift:54-61) is not below Double(T.max) the reference composes in a wider
 * integer and demands variableTime (:151-173) -- variable_time == 0 is then HE_ERR_INVALID_ARGUMENT.  Host only.
 * Warning (the reference's, :111-112): the noise budget must never be forwarded to another party.  Sharing it acts as an
 * oracle that can be used to recover the secret key. */
int he_bfv_noise_budget_from_norm(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, const uint64_t* limbs,
                                  int variable_time, double* out);

/* ---- secret keys, encryption and evaluation keys made on the device from caller-supplied seeds ----
 * The reference draws the secret key and the error polynomials from SystemRandomNumberGenerator and `a` from
 * NistAes128Ctr(seed:); its samplers are written over any generator (PolyRq/PolyRq+Randomize.swift:87, :120).  Here EVERY
 * random polynomial is a function of a 32-byte seed through NistAes128Ctr(seed:) and equals, word for word, what the
 * reference's sampler gives on that generator.  The library generates no seed: seeds come from the caller's CSPRNG, one fresh
 * seed per polynomial, and error and key seeds are as secret as the key.  Only an `a` seed may be published (it is the seed of a
 * seeded ciphertext).
 * The entries take the slab word as an argument (word_bits 32 or 64; 4-byte slabs need a context from
 * he_bfv_context_create_u32) and have no _u32 twins.  Common to them:
 *   seeds       DEVICE bytes, [..][32]
 *   secret_key  [L_all][N] Eval over the secret-key context (every coefficient modulus), as he_bfv_decrypt_device reads it
 *   workspace   NULL = stream-ordered scratch, else at least he_bfv_encrypt_workspace_bytes() bytes, 16-byte aligned.
 *               Everything in it that depends on a secret (the DRBG records of error and key seeds, error polynomials and
 *               their transforms, s^2 and rotated keys) is overwritten with zeros on `s` before the entry releases it or returns:
 *               the first he_bfv_encrypt_workspace_bytes() bytes of a caller's workspace read zero once the stream has drained.
 * `out` and the workspace overlap none of the slabs the entry reads nor one another (HE_ERR_INVALID_ARGUMENT); slabs that are
 * only read may alias (the secret key as a current key of he_bfv_generate_key_switch_keys_device).
 * Errors: word_bits other than 32 / 64 and moduli_count outside its range HE_ERR_INVALID_ARGUMENT; a 4-byte call on a
 * Bfv<UInt64> context HE_ERR_INVALID_ARGUMENT, as the decryption entries; key generation on a context with one coefficient
 * modulus HE_ERR_UNSUPPORTED (supportsEvaluationKey, Bfv/Bfv+Keys.swift:35-37); on 4-byte words a degree above 32768
 * HE_ERR_UNSUPPORTED.  All are reported before anything is enqueued.  A count of 0 does nothing.  All enqueue-only on `s`.
 * Known limitation: the AES behind the stream is a T-table implementation in LDS; its timing depends on the bank pattern of
 * data-dependent lookups, i.e. it is not constant-time, and secret seeds pass through it. */
enum he_encrypt_operation {
    HE_ENCRYPT_OP_SECRET_KEY = 0,         /* count = batch; moduli_count and eval_out ignored */
    HE_ENCRYPT_OP_ENCRYPT_ZERO = 1,       /* count = batch */
    HE_ENCRYPT_OP_ENCRYPT = 2,            /* count = batch; eval_out ignored */
    HE_ENCRYPT_OP_KEY_SWITCH_KEYS = 3,    /* count = keys; moduli_count and eval_out ignored */
    HE_ENCRYPT_OP_RELINEARIZATION_KEY = 4, /* count ignored */
    HE_ENCRYPT_OP_GALOIS_KEYS = 5         /* count = elements */
};
/* The scratch of the entry `operation` (0 on invalid arguments).  Host only. */
size_t he_bfv_encrypt_workspace_bytes(const he_bfv_context* ctx, uint32_t word_bits, int operation, uint32_t moduli_count,
                                      int eval_out, size_t count);
/* Bfv.generateSecretKey (Bfv/Bfv+Keys.swift:20-26): randomizeTernary, then forwardNtt.  out [batch][L_all][N] Eval. */
int he_bfv_generate_secret_key_device(const he_bfv_context* ctx, uint32_t word_bits, const uint8_t* seeds, void* out,
                                      size_t batch, void* workspace, size_t workspace_bytes, he_stream s);
/* Bfv.encryptZero(for:using:with:) (Bfv/Bfv+Encrypt.swift:150-181) over the first m = moduli_count coefficient moduli,
 * 1 <= m <= L_all (m = L_all: the key-switching context of key generation); the first m rows of the one secret key are read.
 * out [batch][2][m][N].  eval_out == 0: Coeff form, [-(INTT(a s) + e), INTT(a)], the canonical ciphertext; eval_out != 0: the
 * words of that ciphertext forward-transformed, [-(a s + NTT(e)), a], formed without an inverse transform.  a_seeds[b] is the
 * `seed` of ciphertext b. */
int he_bfv_encrypt_zero_device(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, int eval_out,
                               const void* secret_key, const uint8_t* a_seeds, const uint8_t* error_seeds, void* out,
                               size_t batch, void* workspace, size_t workspace_bytes, he_stream s);
/* Bfv.encrypt (Bfv/Bfv+Encrypt.swift:66-73) = encryptZero + plaintextTranslate(.Add) (:75-139): plaintexts [batch][N] slab
 * words, values < t; out [batch][2][m][N] Coeff, 1 <= m <= he_bfv_ciphertext_moduli_count.  Word for word
 * he_bfv_encrypt_zero_device followed by he_bfv_add_plain_device. */
int he_bfv_encrypt_device(const he_bfv_context* ctx, uint32_t word_bits, uint32_t moduli_count, const void* secret_key,
                          const uint8_t* a_seeds, const uint8_t* error_seeds, const void* plaintexts, void* out, size_t batch,
                          void* workspace, size_t workspace_bytes, he_stream s);
/* Bfv._generateKeySwitchKey (Bfv/Bfv+Keys.swift:69-103) for `keys` current keys at once: current_keys [keys][L+1][N] Eval,
 * a_seeds / error_seeds [keys][L][32], out [keys][L][2][L+1][N] Eval, L = he_bfv_ciphertext_moduli_count.  Ciphertext j of a key
 * is an Eval encryption of zero over all L + 1 moduli with (q_ks mod q_j) currentKey[j] added to row j of polynomial 0.  The
 * current keys belong to the caller (the reference zeroizes its own copy).  At most 32 ciphertext moduli. */
int he_bfv_generate_key_switch_keys_device(const he_bfv_context* ctx, uint32_t word_bits, const void* secret_key,
                                           const void* current_keys, const uint8_t* a_seeds, const uint8_t* error_seeds,
                                           void* out, size_t keys, void* workspace, size_t workspace_bytes, he_stream s);
/* Bfv.generateRelinearizationKey (Bfv/Bfv+Keys.swift:58-65): the key-switch key of s s, formed in the workspace.
 * a_seeds / error_seeds [L][32], out [L][2][L+1][N] Eval as he_bfv_relinearize_device takes it. */
int he_bfv_generate_relinearization_key_device(const he_bfv_context* ctx, uint32_t word_bits, const void* secret_key,
                                               const uint8_t* a_seeds, const uint8_t* error_seeds, void* out, void* workspace,
                                               size_t workspace_bytes, he_stream s);
/* The Galois keys of Bfv.generateEvaluationKey (Bfv/Bfv+Keys.swift:38-45): per element the key-switch key of
 * applyGalois(s, element), formed in the workspace.  elements: a HOST array of `count` elements, each odd and in (1, 2N) as
 * he_poly_apply_galois_device demands (else HE_ERR_INVALID_ARGUMENT); a_seeds / error_seeds [count][L][32]; out
 * [count][L][2][L+1][N] Eval, slice e the key he_bfv_apply_galois_device takes for elements[e]. */
int he_bfv_generate_galois_keys_device(const he_bfv_context* ctx, uint32_t word_bits, const void* secret_key,
                                       const uint64_t* elements, size_t count, const uint8_t* a_seeds,
                                       const uint8_t* error_seeds, void* out, void* workspace, size_t workspace_bytes,
                                       he_stream s);
/* The polynomial-level samplers, twins of he_poly_random_from_seeds_device: seeds [batch][32] DEVICE bytes -> out
 * [batch][L][N] Coeff in slab words of word_bits.  randomizeTernary (PolyRq/PolyRq+Randomize.swift:87-104): 12 stream bytes
 * per coefficient, (value mod 3) - 1 in every row.  randomizeCenteredBinomialDistribution (:120-167) at the only
 * ErrorStdDev, stdDev32: 16 stream bytes per coefficient, popcount of 21 bits minus popcount of 21 bits.  Their DRBG records
 * live in stream-ordered scratch and are zeroized before it is released.  A modulus that does not fit 4-byte words:
 * HE_ERR_INVALID_MODULUS. */
int he_poly_random_ternary_from_seeds_device(const he_poly_context* ctx, uint32_t word_bits, const uint8_t* seeds, size_t batch,
                                             void* out, he_stream s);
int he_poly_random_centered_binomial_from_seeds_device(const he_poly_context* ctx, uint32_t word_bits, const uint8_t* seeds,
                                                       size_t batch, void* out, he_stream s);

/* =====================================================================================================
 * B4: application hook -- the PIR server's per-chunk response, device-resident
 * =================================================================================================== */

/* PirUtilProtocol.computeResponseForOneChunk (PrivateInformationRetrieval/IndexPir/PirUtil.swift:408-486,
 * MulPirServer.computeResponseForOneChunk IndexPir/MulPir.swift:369-410), all device pointers except `present`:
 *   dimensions          host, [dimension_count]             IndexPirParameter.dimensions
 *   dim0_query_eval     [d0][2][L][N] Eval                   expandedDim0Query
 *   remaining_query     [remaining_query_count][2][L][N] Coeff   expandedRemainingQuery (NULL / 0 for one dimension)
 *   database            [prod(dimensions)][L][N] Eval        dataChunk; plaintext k of column c at index c*d0 + k
 *                                                            (MulPir.swift:547-555)
 *   present             host, [prod(dimensions)] or NULL     0 = nil plaintext
 *   relinearization_key [L][2][L+1][N] Eval                  needed when dimension_count > 1
 *   out                 [2][1][N] Coeff over q_0             the response ciphertext after modSwitchDownToSingle
 * L = he_bfv_ciphertext_moduli_count(ctx).  The reference's precondition (columns == 1 or == remaining query count)
 * and a final result count != 1 return HE_ERR_INVALID_ARGUMENT. */
int he_pir_compute_response_chunk_device(const he_bfv_context* ctx, const uint32_t* dimensions,
                                         uint32_t dimension_count, const uint64_t* dim0_query_eval,
                                         const uint64_t* remaining_query, size_t remaining_query_count,
                                         const uint64_t* database, const uint8_t* present,
                                         const uint64_t* relinearization_key, uint64_t* out, he_stream s);

/* The two halves of computeResponseForOneChunk, for callers that shard the database by column (the reference groups
 * columns over tasks, PirUtil.swift:427-445; here: one column shard per GPU, the results gathered with RCCL):
 *   he_pir_dim0_columns_device          PirUtil.swift:428-446 for `columns` columns: inner product of the dim-0 query with
 *                                       each column's d0 plaintexts, then canonical (Coeff) format
 *                                       database [columns][d0][L][N] Eval, present_device DEVICE [columns][d0] or NULL
 *                                       out [columns][2][L][N] Coeff
 *   he_pir_remaining_dimensions_device  PirUtil.swift:448-485 on all columns' intermediate results:
 *                                       intermediate [columns][2][L][N] Coeff is consumed (overwritten)
 * Both are enqueue-only.  chunk = dim0_columns over all columns, then remaining_dimensions. */
int he_pir_dim0_columns_device(const he_bfv_context* ctx, const uint64_t* dim0_query_eval, size_t d0,
                               const uint64_t* database, const uint8_t* present_device, size_t columns, uint64_t* out,
                               he_stream s);
int he_pir_remaining_dimensions_device(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count,
                                       uint64_t* intermediate, const uint64_t* remaining_query,
                                       size_t remaining_query_count, const uint64_t* relinearization_key, uint64_t* out,
                                       he_stream s);
/* he_pir_remaining_dimensions_device for `chunk_count` chunks at once: intermediate [chunk][columns][2][L][N] Coeff (consumed)
 * -> out [chunk][2][1][N]; every stage one batch over the result groups of all chunks (what the chunk loop below runs after its
 * dim-0 launch, for callers that produced the dim-0 results themselves: he_pir_compute_response_group). */
int he_pir_remaining_dimensions_chunks_device(const he_bfv_context* ctx, const uint32_t* dimensions,
                                              uint32_t dimension_count, size_t chunk_count, uint64_t* intermediate,
                                              const uint64_t* remaining_query, size_t remaining_query_count,
                                              const uint64_t* relinearization_key, uint64_t* out, he_stream s);
/* PirUtilProtocol.computeResponse's chunk loop for one query (PirUtil.swift:533-563): the database holds `chunk_count`
 * chunks of prod(dimensions) plaintexts each ([chunk][prod(dimensions)][L][N] Eval), the same expanded query serves
 * every chunk, out [chunk_count][2][1][N].  The chunks are independent (the reference maps them over tasks) and are
 * answered together: one dim-0 launch over the columns of all chunks, then every stage of every remaining dimension as
 * one batch over the result groups of all chunks (he_bfv_inner_product_shared_device), in groups of chunks that keep the
 * intermediate ciphertexts under about 1 GiB.  present_device: DEVICE [chunk][prod(dimensions)] or NULL.  Enqueue-only. */
int he_pir_compute_response_device(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count,
                                   const uint64_t* dim0_query_eval, const uint64_t* remaining_query,
                                   size_t remaining_query_count, const uint64_t* database, const uint8_t* present_device,
                                   size_t chunk_count, const uint64_t* relinearization_key, uint64_t* out, he_stream s);
/* The same for `queries` (1..4) queries over the same database in one call: their dim-0 inner products share one pass
 * over the database (the plaintexts are read from HBM once for all queries; 1.7-2.1 x the single-query rate per query
 * at 2-4 queries), the remaining dimensions run query by query.
 *   dim0_queries_eval   [dimensions[0]][queries][2][L][N] Eval  (the queries' dim-0 ciphertexts side by side)
 *   remaining_queries   [queries][remaining_query_count][2][L][N] Coeff
 *   relinearization_keys HOST array of `queries` device pointers (one key per query; NULL for one-dimensional databases)
 *   out                 [queries][chunk_count][2][1][N]
 * Each query's responses equal he_pir_compute_response_device's for that query alone.  Enqueue-only. */
int he_pir_compute_response_queries_device(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count,
                                           size_t queries, const uint64_t* dim0_queries_eval,
                                           const uint64_t* remaining_queries, size_t remaining_query_count,
                                           const uint64_t* database, const uint8_t* present_device, size_t chunk_count,
                                           const uint64_t* const* relinearization_keys, uint64_t* out, he_stream s);
/* The same two with the database packed (he_bfv_pack_plaintexts_device at the top level: [chunk][prod(dimensions)]
 * [he_bfv_packed_plaintext_words] words): the dim-0 pass, which is bound by the
 * database bytes it streams, reads bits(q) / 64 of them.  Same responses, word for word. */
int he_pir_dim0_columns_packed_device(const he_bfv_context* ctx, const uint64_t* dim0_query_eval, size_t d0,
                                      const uint64_t* packed_database, const uint8_t* present_device, size_t columns,
                                      uint64_t* out, he_stream s);
int he_pir_compute_response_packed_device(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count,
                                          const uint64_t* dim0_query_eval, const uint64_t* remaining_query,
                                          size_t remaining_query_count, const uint64_t* packed_database,
                                          const uint8_t* present_device, size_t chunk_count,
                                          const uint64_t* relinearization_key, uint64_t* out, he_stream s);

/* PirUtilProtocol.computeResponse(to:using:databases:parameter:context:callOptions:) (PirUtil.swift:490-568) -- the whole
 * server side of a Query in one call: expand its ciphertexts into sum(dimensions) selection ciphertexts per queried index
 * (he_pir_expand_device), take each index's first dimensions[0] of them to Eval, answer every chunk.
 *   query_ciphertexts   [query_ciphertext_count][2][L][N] Coeff (Query.ciphertexts)
 *   indices_count       Query.indicesCount
 *   galois_elements / galois_keys / galois_key_count   the evaluation key's Galois keys, as for he_pir_expand_device
 *   relinearization_key device key (NULL for one-dimensional databases)
 *   databases           HOST array of database_count device pointers, each [chunk_count][prod(dimensions)][L][N] Eval;
 *                       database_count == 1: every index queries that database (four indices at a time then share one
 *                       pass over it); database_count >= indices_count: index i queries databases[i].  Anything else is
 *                       the reference's PirError.invalidBatchSize: HE_ERR_INVALID_ARGUMENT.
 *   present_masks       HOST array of as many DEVICE masks [chunk_count][prod(dimensions)] (entries or the array NULL:
 *                       all present)
 *   out                 [indices_count][chunk_count][2][1][N]  (Response.ciphertexts)
 * Enqueue-only once the context has seen the query's shape (he_pir_expand_device). */
int he_pir_compute_response_to_query_device(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count,
                                            const uint64_t* query_ciphertexts, size_t query_ciphertext_count,
                                            size_t indices_count, const uint64_t* galois_elements,
                                            const uint64_t* const* galois_keys, size_t galois_key_count,
                                            const uint64_t* relinearization_key, const uint64_t* const* databases,
                                            const uint8_t* const* present_masks, size_t database_count, size_t chunk_count,
                                            uint64_t* out, he_stream s);

/* MulPirServer.process(database:with:using:) (PrivateInformationRetrieval/IndexPir/MulPir.swift:431-556) -- the database
 * a server answers from, built on the device from the raw entry bytes.  The IndexPirParameter is given as its fields:
 * dimensions, entry_size_in_bytes, encoding_entry_size (nonzero: every entry is preceded by its byte count in
 * IndexPirConfig.entrySizeEncodingWidth little-endian bytes, IndexPirProtocol.swift:60-73,106-150); entry_count is the
 * number of entries handed in (the reference's PirError.invalidDatabaseEntryCount is the caller's check: it holds both).
 * he_pir_database_shape is the plan (MulPir.swift:445-450; no device work, host-only contexts too):
 *   out_chunk_count               ceil((width + entry_size_in_bytes) / bytes per plaintext)
 *   out_plaintexts_per_chunk      prod(dimensions)
 *   out_bytes_per_plaintext       N floor(log2 t) / 8          (EncryptionParameters.swift:101-110)
 *   out_entries_per_plaintext     floor(bytes per plaintext / (width + entry_size_in_bytes)) in pack mode (one chunk),
 *                                 0 in split mode (more than one chunk: entry r is row r, chunk k its k-th plaintext)
 *   out_entry_size_encoding_width 0 without a size prefix, else 1, 2, 4 or 8
 * Any out pointer may be NULL.  HE_ERR_INVALID_ARGUMENT: empty or zero dimensions; split mode with more entries than
 * prod(dimensions); pack mode with more plaintexts than prod(dimensions); entries of zero bytes without a prefix. */
int he_pir_database_shape(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count,
                          size_t entry_count, size_t entry_size_in_bytes, int encoding_entry_size, size_t* out_chunk_count,
                          size_t* out_plaintexts_per_chunk, size_t* out_bytes_per_plaintext,
                          size_t* out_entries_per_plaintext, size_t* out_entry_size_encoding_width);
/* The database itself, in the layout every he_pir_compute_response_* entry reads:
 *   entries      DEVICE [entry_count][entry_size_in_bytes]; bytes past an entry's own size are ignored (need not be zero)
 *   entry_sizes  HOST [entry_count] byte counts, or NULL: every entry is entry_size_in_bytes long.  Given, they are checked
 *                first -- an entry longer than entry_size_in_bytes is the reference's invalidDatabaseEntrySize,
 *                HE_ERR_INVALID_ARGUMENT -- and uploaded: the call returns once that copy is done (a stream synchronisation).
 *                NULL: the call is enqueue-only.
 *   database     DEVICE [chunk_count][prod(dimensions)][L][N] Eval at the top level (Plaintext.convertToEvalFormat of
 *                context.encode(values:format: .coefficient), Bfv+Encode.swift:44-50); a nil plaintext is all zeros
 *   present      DEVICE [chunk_count][prod(dimensions)]: 0 where the reference's plaintext is nil (its bytes are all zero or
 *                there are none), 1 elsewhere
 * Plaintexts are placed as the reference reorders them: plaintext j of chunk k at slot (j % R) d0 + j / R, d0 =
 * dimensions[0], R = prod(dimensions) / d0.  Errors are returned before anything is written.  A host-only context:
 * HE_ERR_DEVICE. */
int he_pir_process_database_device(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count,
                                   const uint8_t* entries, const uint64_t* entry_sizes, size_t entry_count,
                                   size_t entry_size_in_bytes, int encoding_entry_size, uint64_t* database, uint8_t* present,
                                   he_stream s);
/* The same for a Bfv<UInt32> context, the database in packed 4-byte words (he_pir_compute_response_device_u32's). */
int he_pir_process_database_device_u32(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count,
                                       const uint8_t* entries, const uint64_t* entry_sizes, size_t entry_count,
                                       size_t entry_size_in_bytes, int encoding_entry_size, uint32_t* database,
                                       uint8_t* present, he_stream s);

/* ---- the MulPIR client (PrivateInformationRetrieval/IndexPir/MulPir.swift:117-289): queries from indices, entries from replies
 * The IndexPirParameter is given as its fields, exactly as he_pir_database_shape takes them.  With N the degree, t the plaintext
 * modulus, bits = floor(log2 t), bpp = N bits / 8, w the entry-size encoding width (0 without encoding), E =
 * entry_size_in_bytes, enc = w + E, S = sum(dimensions), I = indices_count:
 *   per = bpp / enc when bpp >= enc, else 1    entryChunksPerPlaintext (MulPir.swift:150-155)
 *   R   = ceil(enc / bpp)                      expectedResponseCiphertextCount (:229-231)
 *   C   = ceil(S I / N)                        the ciphertexts of a Query (PirUtil.swift:381-404)
 * he_pir_client_plan is the plan (no device work, host-only contexts too); any out pointer may be NULL.  Its errors are those of
 * he_pir_database_shape, then indices_count == 0 or above 2^20 (HE_ERR_INVALID_ARGUMENT) and dimension_count > 16
 * (HE_ERR_UNSUPPORTED: the kernels take the dimensions by value). */
int he_pir_client_plan(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count, size_t entry_count,
                       size_t entry_size_in_bytes, int encoding_entry_size, size_t indices_count, size_t* out_expanded_query_count,
                       size_t* out_query_ciphertext_count, size_t* out_reply_ciphertext_count, size_t* out_entries_per_plaintext,
                       size_t* out_bytes_per_plaintext, size_t* out_entry_size_encoding_width);
/* MulPir.evaluationKeyConfig(expandedQueryCount:degree:keyCompression:) (MulPir.swift:86-109): the Galois elements of the
 * evaluation key he_pir_expand_device needs for a query of expanded_query_count = S I inputs, in the reference's order -- the
 * `elements` of he_bfv_generate_galois_keys_device.  *out_count (may be NULL) is their number; out_elements (a HOST array of
 * `capacity` elements, or NULL to ask for the count) too small: HE_ERR_INVALID_ARGUMENT.  One input needs no expansion: without
 * compression the list is empty (the reference's range is empty there), with compression it is the reference's 2N + 1, which no
 * key generation takes.  Host only. */
enum he_pir_key_compression {
    HE_PIR_KEY_COMPRESSION_NONE = 0,   /* PirKeyCompressionStrategy.noCompression */
    HE_PIR_KEY_COMPRESSION_HYBRID = 1, /* .hybridCompression */
    HE_PIR_KEY_COMPRESSION_MAX = 2     /* .maxCompression */
};
int he_pir_evaluation_key_elements(uint32_t degree, size_t expanded_query_count, int key_compression, uint64_t* out_elements,
                                   size_t capacity, size_t* out_count);
/* The two device entries take the slab word as an argument (word_bits 32 or 64; 4-byte slabs need a context from
 * he_bfv_context_create_u32) and have no _u32 twins.  Both are enqueue-only on `s`.  Every argument error is returned before anything is enqueued, in this order: the
 * word, the context, the shape (he_pir_client_plan's errors, moduli_count, a batch too large for one call, HE_ERR_NOT_INVERTIBLE),
 * null buffers, buffers that overlap one the call writes; HE_ERR_DEVICE comes last on a host-only context.  queries == 0 does
 * nothing.  workspace: DEVICE, 16-byte aligned, at least the bytes the entry's _workspace_bytes function gives (0 on refused
 * arguments), or NULL for stream-ordered scratch.  It holds the plaintexts in the clear and the scratch of encryption or
 * decryption: all of it is overwritten with zeros on `s` before the entry releases it or returns.
 *
 * he_pir_generate_query_device -- MulPirClient.generateQuery(at:using:) for `queries` queries of I indices each:
 *   indices       DEVICE uint64 [queries][I]; they are secret
 *   secret_key    as he_bfv_encrypt_device reads it; one key per call
 *   a_seeds, error_seeds  DEVICE [queries][C][32]
 *   out           DEVICE [queries][C][2][L][N] Coeff, L = he_bfv_ciphertext_moduli_count; slice q is the query_ciphertexts of
 *                 he_pir_compute_response_to_query_device
 *   out_of_range  DEVICE word the caller zeroes, or NULL: set to 1 when an index is >= entry_count (PirError.invalidIndex);
 *                 that index selects nothing, the other indices of its query are unaffected
 * One kernel writes the plaintexts of PirUtil.compressBinaryInputs, one lane per word: input p = c N + x of ciphertext c is
 * index i = p / S and dimension k whose range of S holds p mod S; the word is (2^ceilLog2(count_c))^-1 mod t, count_c =
 * min(N, S I - c N), when coordinate k of plaintext indices[q][i] / per (computeCoordinates, MulPir.swift:181-193) is that
 * input, else 0.  A t without that inverse: HE_ERR_NOT_INVERTIBLE.  Then he_bfv_encrypt_device's pipeline at L moduli: every
 * output word equals that entry's on the same plaintexts and seeds. */
size_t he_pir_generate_query_workspace_bytes(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                             uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                             int encoding_entry_size, size_t indices_count, size_t queries);
int he_pir_generate_query_device(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                 uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes, int encoding_entry_size,
                                 size_t indices_count, const uint64_t* indices, size_t queries, const void* secret_key,
                                 const uint8_t* a_seeds, const uint8_t* error_seeds, void* out, uint32_t* out_of_range,
                                 void* workspace, size_t workspace_bytes, he_stream s);
/* he_pir_decrypt_response_device -- MulPirClient.decrypt(response:at:using:) and decryptFull (MulPir.swift:245-288):
 *   response     DEVICE [queries][I][R][2][moduli_count][N] Coeff: per query the `out` of
 *                he_pir_compute_response_to_query_device (moduli_count 1); any level is allowed
 *   indices      as above; NULL selects decryptFull
 *   out_entries  DEVICE bytes [queries][I][E]; decryptFull: [queries][I][R bpp]
 *   out_sizes    DEVICE uint64 [queries][I]; may be NULL without a size prefix and for decryptFull
 * he_bfv_decrypt_device with correction factor 1, then one kernel with one lane per output byte.  A reply's byte string is
 * CoefficientPacking.coefficientsToBytes(bitsPerCoeff: bits) of its R plaintexts back to back, bpp bytes each, MSB first: stream
 * bit s is bit bits - 1 - (s mod bits) of coefficient s / bits.  As in the reference a coefficient is not masked to `bits`
 * bits: bit `bits` of a coefficient in [2^bits, t) is OR-ed into the last bit of the field before it when its own field does
 * not begin a byte, and is dropped when it does (CoefficientPacking.swift:186-205).
 * Entry (q, i) lies at byte pos enc of its reply, pos = indices[q][i] mod per.  Without a size prefix it is the E bytes there
 * and out_sizes, if given, is E.  With one, the first w bytes are the little-endian size z: out_sizes = min(z, E) and
 * out_entries holds the next min(z, E) bytes, then zeros up to E (the reference traps for z >= 2^63 and returns what there is
 * for E < z; here both clamp).  decryptFull: out_sizes, if given, is R bpp. */
size_t he_pir_decrypt_response_workspace_bytes(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                               uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                               int encoding_entry_size, size_t indices_count, uint32_t moduli_count,
                                               size_t queries);
int he_pir_decrypt_response_device(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                   uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                   int encoding_entry_size, size_t indices_count, uint32_t moduli_count, const void* response,
                                   const uint64_t* indices, size_t queries, const void* secret_key, uint8_t* out_entries,
                                   uint64_t* out_sizes, void* workspace, size_t workspace_bytes, he_stream s);

/* ---- keyword PIR database (PrivateInformationRetrieval/KeywordPir/) --------------------------------------------------------
 * KeywordPirServer.process (KeywordPirProtocol.swift:191-247) builds a cuckoo table of the keyword-value pairs, serializes
 * every bucket and hands each sub-table's buckets to MulPirServer.process as index-PIR entries.  Here the keyword and value
 * bytes go to the device once; the device hashes the keywords and derives the candidate buckets, the host places the entries
 * reading 8 bytes of hash, h indices and one size per entry, and the device writes the serialized buckets as the
 * [bucket][entry_size_in_bytes] slab he_pir_process_database_device reads.  None of the layered entries needs a context.
 *
 * A database is two blobs with offsets: keyword i is keywords[keyword_offsets[i], keyword_offsets[i + 1]), value i is
 * values[value_offsets[i], value_offsets[i + 1]); both lie back to back at any byte address and may be empty. */

/* CuckooTableConfig (CuckooTable.swift:18-84).  fixed_size nonzero is .fixedSize(bucketCount: bucket_count); zero is
 * .allowExpansion(expansionFactor:targetLoadFactor:).  multiple_tables nonzero: hash function i has the sub-table
 * [i bucketsPerTable, (i + 1) bucketsPerTable) to itself, table_count = hash_function_count; zero: one table. */
typedef struct he_cuckoo_table_config {
    uint32_t hash_function_count;
    uint32_t max_eviction_count;
    uint64_t max_serialized_bucket_size;
    int fixed_size;
    uint64_t bucket_count;      /* read when fixed_size is nonzero */
    double expansion_factor;    /* read when fixed_size is zero */
    double target_load_factor;  /* read when fixed_size is zero */
    int multiple_tables;
    uint32_t slot_count;
} he_cuckoo_table_config;

/* HashKeyword.hash (HashBucket.swift:264-269): SHA-256 of each keyword, the first 8 digest bytes as a little-endian UInt64.
 *   keywords DEVICE blob; keyword_offsets DEVICE uint64 [count + 1], non-decreasing; out_hashes DEVICE uint64 [count].
 * Nothing outside [keywords, keywords + keyword_offsets[count]) is read.  count above 2^32 - 1: HE_ERR_INVALID_ARGUMENT.
 * Enqueue-only. */
int he_keyword_pir_hash_keywords_device(const uint8_t* keywords, const uint64_t* keyword_offsets, size_t count,
                                        uint64_t* out_hashes, he_stream s);
/* HashKeyword.hashIndices (HashBucket.swift:221-257) with bucketCount = bucket_count (the table's bucketsPerTable):
 * out_indices DEVICE uint32 [count][hash_function_count].  A repeated index is kept after the tenth retry, as the reference
 * keeps it.  bucket_count outside 1 .. 2^32 - 1 or hash_function_count 0: HE_ERR_INVALID_ARGUMENT; hash_function_count
 * above 8: HE_ERR_UNSUPPORTED (the reference's configurations use 1 to 3).  Enqueue-only. */
int he_keyword_pir_hash_indices_device(const uint64_t* hashes, size_t count, uint64_t bucket_count,
                                       uint32_t hash_function_count, uint32_t* out_indices, he_stream s);
/* ShardingFunction.shardIndex (KeywordDatabase.swift:56-62,103-111) from the keyword hashes: hash % shard_count, or with
 * other_shard_count nonzero doubleMod's (hash % other_shard_count) % shard_count.  out DEVICE uint32 [count].  shard_count
 * outside 1 .. 2^32 - 1: HE_ERR_INVALID_ARGUMENT.  Enqueue-only. */
int he_keyword_pir_shard_indices_device(const uint64_t* hashes, size_t count, uint64_t shard_count, uint64_t other_shard_count,
                                        uint32_t* out, he_stream s);

/* CuckooTableConfig.validate() (CuckooTable.swift:138-156): HE_OK or HE_ERR_INVALID_CUCKOO_CONFIG (a target load factor that is
 * not above 0, by which the reference would divide, included); NULL: HE_ERR_INVALID_ARGUMENT.  Host. */
int he_keyword_pir_config_validate(const he_cuckoo_table_config* config);
/* The bucket count CuckooTable.init starts from (CuckooTable.swift:339-349): ceil(ceil(serialized size of all values in one
 * bucket / max_serialized_bucket_size) / target_load_factor), or the fixed count, rounded up to a multiple of the table
 * count.  value_sizes HOST [count].  Host. */
int he_keyword_pir_bucket_count(const he_cuckoo_table_config* config, const uint64_t* value_sizes, size_t count, size_t* out);
/* CuckooTable.insert / insertLoop (CuckooTable.swift:386-458) over integers: every entry in order into an empty table of
 * bucket_count buckets (a multiple of the table count).  All pointers HOST; works without a device.
 *   hashes [count], indices [count][hash_function_count] (each below bucket_count / table count), value_sizes [count]
 *   out_bucket_offsets [bucket_count + 1], out_slot_entries [count]: bucket b holds entries out_slot_entries[
 *   out_bucket_offsets[b] .. out_bucket_offsets[b + 1]) in slot order; out_placed = out_bucket_offsets[bucket_count]
 * canInsert, swapIndices, index(tableIndex:index:), the size guard of insert and maxEvictionCount are the reference's.
 * Three things are not:
 *   1. Duplicates go by the 64-bit keyword hash and the first one wins (out_duplicates_dropped counts the others).  The
 *      reference compares keyword bytes, so it would store two different keywords of one hash; a client finds only the first
 *      either way (HashBucket.find(hash:)).
 *   2. The evicted slot is candidates[splitmix64(seed).next() % candidates.count]; the reference draws from
 *      SystemRandomNumberGenerator and so builds no reproducible table.
 *   3. No entry is lost.  Where no resident value can be swapped out the reference expands and returns without inserting the
 *      pair it holds (:449-457); here the pair is part of the larger table.
 * Errors: HE_ERR_INVALID_CUCKOO_CONFIG; HE_ERR_INVALID_HASH_BUCKET_ENTRY_VALUE_SIZE for a value above 65 535 bytes;
 * HE_ERR_FAILED_TO_CONSTRUCT_CUCKOO_TABLE for a value whose single-entry bucket exceeds max_serialized_bucket_size and, with
 * fixed_size, wherever the reference throws it (evictions used up, nothing to swap); HE_ERR_INVALID_ARGUMENT for null
 * pointers, a bucket_count that is zero or no multiple of the table count, an index out of range, count above 2^32 - 1.
 * Without fixed_size a needed expansion returns HE_ERR_CUCKOO_TABLE_NEEDS_EXPANSION and out_next_bucket_count =
 * ceil(bucket_count * expansion_factor) rounded up to a multiple of the table count (:466-474): the candidate indices depend
 * on the bucket count, so the caller derives them anew and places every entry again, as the reference re-inserts them. */
int he_keyword_pir_cuckoo_place(const he_cuckoo_table_config* config, const uint64_t* hashes, const uint32_t* indices,
                                const uint64_t* value_sizes, size_t count, size_t bucket_count, uint64_t seed,
                                uint32_t* out_bucket_offsets, uint32_t* out_slot_entries, size_t* out_placed,
                                size_t* out_duplicates_dropped, size_t* out_next_bucket_count);

/* HashBucket.serialize (HashBucket.swift:90-103,177-187) of every bucket, bucket b at out + b * entry_size_in_bytes: the slot
 * count byte, per slot the 8-byte little-endian keyword hash, the UInt16 little-endian value size and the value; the rest of
 * the row is written as zero (an empty bucket is all zero).  All pointers DEVICE, any byte address for values and out:
 *   hashes [entries], values, value_offsets [entries + 1], bucket_offsets uint32 [bucket_count + 1], slot_entries uint32
 *   [bucket_offsets[bucket_count]] as he_keyword_pir_cuckoo_place writes them, out [bucket_count][entry_size_in_bytes]
 * Exactly the bytes of `out` are written and only bytes of the named arrays are read.  device_mismatch (optional, a DEVICE word
 * the caller has zeroed): bit 0 when a bucket's serialization is longer than entry_size_in_bytes (the row holds its first
 * bytes), bit 1 when a bucket has more than 255 slots (invalidHashBucketSlotCount).  Enqueue-only: the slots' running offsets
 * go to stream-ordered scratch (4 bytes per slot), then one launch. */
int he_keyword_pir_serialize_buckets_device(const uint64_t* hashes, const uint8_t* values, const uint64_t* value_offsets,
                                            const uint32_t* bucket_offsets, const uint32_t* slot_entries, size_t slot_count,
                                            size_t bucket_count, size_t entry_size_in_bytes, uint8_t* out,
                                            uint32_t* device_mismatch, he_stream s);

/* The table object: CuckooTable.init (CuckooTable.swift:328-357) of a whole database.
 *   keywords DEVICE, keyword_offsets HOST [count + 1]; values DEVICE (not read here), value_offsets HOST [count + 1]
 * The offsets are uploaded, the keywords hashed, the indices derived and both brought to the host; the entries are placed,
 * with the index kernel run again after each expansion; the hashes, the value offsets and the buckets stay on the device.
 * The call synchronises the stream (several times).  Errors as he_keyword_pir_cuckoo_place (never the expansion status), offsets that decrease:
 * HE_ERR_INVALID_ARGUMENT.  Destroy with he_keyword_pir_table_destroy (NULL is fine). */
typedef struct he_keyword_pir_table he_keyword_pir_table;
int he_keyword_pir_table_create_device(const he_cuckoo_table_config* config, const uint8_t* keywords,
                                       const uint64_t* keyword_offsets, const uint8_t* values, const uint64_t* value_offsets,
                                       size_t count, uint64_t seed, he_keyword_pir_table** out_table, he_stream s);
void he_keyword_pir_table_destroy(he_keyword_pir_table* table);
size_t he_keyword_pir_table_bucket_count(const he_keyword_pir_table* table);
size_t he_keyword_pir_table_buckets_per_table(const he_keyword_pir_table* table);
size_t he_keyword_pir_table_table_count(const he_keyword_pir_table* table);
/* CuckooTable.maxSerializedBucketSize() (:381-383): with .allowExpansion and without useMaxSerializedBucketSize this is the
 * maxEntrySize of KeywordPirProtocol.swift:205-218; otherwise that is the config's max_serialized_bucket_size. */
size_t he_keyword_pir_table_largest_bucket_size(const he_keyword_pir_table* table);
size_t he_keyword_pir_table_entry_count(const he_keyword_pir_table* table);        /* entries placed */
size_t he_keyword_pir_table_duplicates_dropped(const he_keyword_pir_table* table);
size_t he_keyword_pir_table_expansion_count(const he_keyword_pir_table* table);
float he_keyword_pir_table_load_factor(const he_keyword_pir_table* table);         /* summarize() (:361-373) */
/* CuckooTable.serializeBuckets() (:375-378) padded: he_keyword_pir_serialize_buckets_device over the whole table into out
 * DEVICE [bucket_count][entry_size_in_bytes]; values is the blob the table was created over.  entry_size_in_bytes below the
 * largest bucket: HE_ERR_INVALID_ARGUMENT.  Enqueue-only. */
int he_keyword_pir_table_entries_device(const he_keyword_pir_table* table, const uint8_t* values, size_t entry_size_in_bytes,
                                        uint8_t* out, he_stream s);
/* KeywordPirProtocol.swift:220-239: the entries into stream-ordered scratch, then he_pir_process_database_device once per
 * sub-table with entry_count = buckets_per_table, no size prefix and no entry sizes.  database DEVICE [table_count][
 * chunk_count][prod(dimensions)][L][N] and present DEVICE [table_count][chunk_count][prod(dimensions)], the order in which the
 * reference concatenates (:230-238).  The words are those of the context: uint64_t for a Context<Bfv<UInt64>>, packed
 * uint32_t for a Context<Bfv<UInt32>> (one entry for both: the context says which).  Enqueue-only. */
int he_keyword_pir_process_database_device(const he_bfv_context* ctx, const he_keyword_pir_table* table, const uint8_t* values,
                                           const uint32_t* dimensions, uint32_t dimension_count, size_t entry_size_in_bytes,
                                           void* database, uint8_t* present, he_stream s);

/* ---- the keyword PIR client (PrivateInformationRetrieval/KeywordPir/KeywordPirProtocol.swift:279-392): queries from keywords,
 * values from replies.  The index-PIR parameter of a keyword database has no size prefix and a batch of h = hashFunctionCount
 * indices (:221-228), so everything below is the MulPIR client above at encoding_entry_size = 0, indices_count = h,
 * entry_count = the table's buckets_per_table and E = entry_size_in_bytes the bucket row, with HashKeyword in front of it and
 * HashBucket.init(deserialize:) / find(hash:) behind it.  A batch of keywords is given as the database is: keywords a DEVICE
 * blob at any byte address, keyword_offsets DEVICE uint64 [queries + 1], non-decreasing; keyword q is keywords[
 * keyword_offsets[q], keyword_offsets[q + 1]).
 *
 * he_keyword_client_plan (host only, host-only contexts too; any out pointer may be NULL): he_pir_client_plan's values and
 *   value_capacity   min(E - 11, 65535), 0 for E < 11: the longest value a row holds (count byte, one 10-byte slot header)
 *   find_form        the form he_keyword_client_find_in_buckets_device takes for this E: staged for E <= 32768, else direct
 *   staged_lds_bytes the LDS of the staged kernel's instantiation for this E (0 for the direct form)
 *   reply_bytes      R bpp: what he_keyword_client_count_entries_device scans per reply
 * Errors: those of he_pir_client_plan; hash_function_count 0: HE_ERR_INVALID_ARGUMENT, above 8: HE_ERR_UNSUPPORTED (as
 * he_keyword_pir_hash_indices_device); E == 0 (the reference's "Serialized HashBucket shouldn't be empty", which no database of
 * this library reaches) and entry_count outside 1 .. 2^32 - 1: HE_ERR_INVALID_ARGUMENT. */
enum he_keyword_pir_find_form {
    HE_KEYWORD_PIR_FIND_FORM_PLAN = -1,  /* an argument only: the form the plan names */
    HE_KEYWORD_PIR_FIND_FORM_STAGED = 0, /* one workgroup a row: the row goes to LDS and is walked there */
    HE_KEYWORD_PIR_FIND_FORM_DIRECT = 1  /* one lane a row: the row is walked in global memory */
};
int he_keyword_client_plan(const he_bfv_context* ctx, const uint32_t* dimensions, uint32_t dimension_count, size_t entry_count,
                               size_t entry_size_in_bytes, uint32_t hash_function_count, size_t* out_expanded_query_count,
                               size_t* out_query_ciphertext_count, size_t* out_reply_ciphertext_count,
                               size_t* out_entries_per_plaintext, size_t* out_bytes_per_plaintext, size_t* out_value_capacity,
                               int* out_find_form, size_t* out_staged_lds_bytes, size_t* out_reply_bytes);
/* The device entries follow the MulPIR client's conventions: word_bits 32 or 64 as an argument and no _u32 twins; enqueue-only on
 * `s`; every argument error before anything is enqueued, in the order the word, the context, the shape (the index-PIR client's
 * errors, then the plan's, then a batch too large for one call), null buffers, buffers that overlap one the call writes (of
 * `keywords`, whose length lies on the device, the first byte); HE_ERR_DEVICE last on a host-only context.  queries == 0 does
 * nothing.  workspace: DEVICE, 16-byte aligned, at least the entry's _workspace_bytes (0 on refused arguments), or NULL for
 * stream-ordered scratch.  It holds the keyword hashes, the bucket indices, the decrypted bucket rows and the search's records:
 * all of it is overwritten with zeros on `s` before the entry releases it or returns.
 *
 * he_keyword_client_generate_query_device -- KeywordPirClient.generateQuery(at:using:) (:326-334) for `queries` keywords:
 * HashKeyword.hash, hashIndices(bucketCount: entry_count, hashFunctionCount: h) as uint64 [queries][h] in the workspace, then
 * he_pir_generate_query_device's pipeline: every output word equals that entry's on those indices and the same seeds.
 *   secret_key, a_seeds, error_seeds [queries][C][32], out [queries][C][2][L][N]   as he_pir_generate_query_device
 *   out_hashes   DEVICE uint64 [queries] or NULL: the keyword hashes, for a caller that keeps them for the reply
 * No index can lie outside the database, so there is no out_of_range flag. */
size_t he_keyword_client_generate_query_workspace_bytes(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                                     uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                                     uint32_t hash_function_count, size_t queries);
int he_keyword_client_generate_query_device(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                         uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                         uint32_t hash_function_count, const uint8_t* keywords, const uint64_t* keyword_offsets,
                                         size_t queries, const void* secret_key, const uint8_t* a_seeds, const uint8_t* error_seeds,
                                         void* out, uint64_t* out_hashes, void* workspace, size_t workspace_bytes, he_stream s);
/* he_keyword_client_find_in_buckets_device -- lines 352-358 of decrypt(response:at:using:) over HashBucket.init(deserialize:) and
 * find(hash:) (HashBucket.swift:51-73,118-133,200-205), bytes in and values out:
 *   buckets     DEVICE [queries][h][E] at any byte address; hashes DEVICE uint64 [queries]
 *   out_values  DEVICE [queries][value_capacity] at any byte address (may be NULL when value_capacity is 0)
 *   out_sizes   DEVICE uint64 [queries]; out_status DEVICE uint32 [queries]: 0 nil, 1 found, 2 corruptedData
 *   form        HE_KEYWORD_PIR_FIND_FORM_PLAN, or one of the two forms (staged with E > 32768: HE_ERR_INVALID_ARGUMENT)
 * A query's h buckets are taken in order.  A bucket b[0, E) is walked: count = b[0], off = 1; per slot the bucket is corrupt if
 * E < off + 10; hash = LE64(b + off), size = LE16(b + off + 8), off += 10; corrupt if off + size > E; off += size.  A corrupt
 * bucket ends the query with status 2, also when an earlier slot of that bucket matches (the reference deserializes a bucket
 * before it searches it); otherwise the first slot whose hash is the query's ends it with status 1, its size and its bytes; no
 * match in any bucket is status 0.  Zero padding behind the last slot is no slot; a found value of no bytes is status 1 with
 * size 0.  out_values[q] is the value, then zeros up to value_capacity; all zeros and size 0 for status 0 and 2.  Exactly the
 * bytes of the three outputs are written, and only bytes of buckets and hashes are read.
 * Two launches and no atomics: the walk leaves one 16-byte record per (query, bucket) in the workspace (staged: one workgroup a
 * row, 16-byte loads into LDS with the ragged ends by bytes, the chain walked at LDS latency; direct: one lane a row in global
 * memory), then one launch resolves the records in bucket order and copies, one lane per 16-byte line of out_values. */
size_t he_keyword_client_find_in_buckets_workspace_bytes(size_t entry_size_in_bytes, uint32_t hash_function_count, size_t queries);
int he_keyword_client_find_in_buckets_device(const uint8_t* buckets, const uint64_t* hashes, size_t entry_size_in_bytes,
                                          uint32_t hash_function_count, size_t queries, int form, uint8_t* out_values,
                                          uint64_t* out_sizes, uint32_t* out_status, void* workspace, size_t workspace_bytes,
                                          he_stream s);
/* he_keyword_client_decrypt_response_device -- KeywordPirClient.decrypt(response:at:using:) (:343-359) for `queries` keywords:
 *   response   DEVICE [queries][h][R][2][moduli_count][N], as he_pir_decrypt_response_device takes it with indices_count = h
 *   keywords, keyword_offsets as above; or keywords NULL and hashes DEVICE uint64 [queries] (he_keyword_client_generate_query_device's
 *              out_hashes)
 * The hashes and indices are derived, he_pir_decrypt_response_device's pipeline writes the bucket rows [queries][h][E] into the
 * workspace, then he_keyword_client_find_in_buckets_device's two launches in the plan's form; outputs as there. */
size_t he_keyword_client_decrypt_response_workspace_bytes(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                                       uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                                       uint32_t hash_function_count, uint32_t moduli_count, size_t queries);
int he_keyword_client_decrypt_response_device(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                           uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                           uint32_t hash_function_count, uint32_t moduli_count, const void* response,
                                           const uint8_t* keywords, const uint64_t* keyword_offsets, const uint64_t* hashes,
                                           size_t queries, const void* secret_key, uint8_t* out_values, uint64_t* out_sizes,
                                           uint32_t* out_status, void* workspace, size_t workspace_bytes, he_stream s);
/* he_keyword_client_count_entries_device -- countEntriesInResponse (:376-391): decryptFull gives [queries][h][R bpp] in the
 * workspace, he_keyword_client_count_bucket_entries_device scans it.  out_counts DEVICE uint64 [queries]. */
size_t he_keyword_client_count_entries_workspace_bytes(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                                    uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                                    uint32_t hash_function_count, uint32_t moduli_count, size_t queries);
int he_keyword_client_count_entries_device(const he_bfv_context* ctx, uint32_t word_bits, const uint32_t* dimensions,
                                        uint32_t dimension_count, size_t entry_count, size_t entry_size_in_bytes,
                                        uint32_t hash_function_count, uint32_t moduli_count, const void* response, size_t queries,
                                        const void* secret_key, uint64_t* out_counts, void* workspace, size_t workspace_bytes,
                                        he_stream s);
/* The scan of countEntriesInResponse (:379-389) over bytes DEVICE [queries][replies_per_query][reply_bytes] at any byte address:
 * per reply off = 0; while off < reply_bytes a bucket is deserialized from b[off, reply_bytes) by the walk above; where that
 * fails the scan of the reply ends and the bucket's slots do not count, otherwise its slot count is added and off advances by its
 * serialized size.  A zero byte is an empty bucket of one byte: padding is stepped over, eight bytes at a time where eight zero
 * bytes are left.  out_counts DEVICE uint64 [queries]: the sum over the query's replies.  One wave a query, a lane a reply; no
 * atomics, no scratch.  Enqueue-only. */
int he_keyword_client_count_bucket_entries_device(const uint8_t* bytes, size_t reply_bytes, size_t replies_per_query, size_t queries,
                                               uint64_t* out_counts, he_stream s);

/* ---- sharded keyword database: KeywordDatabase.init(rows:sharding:shardingFunction:) (KeywordDatabase.swift:406-437) -------
 * PIRProcessDatabase hashes every keyword, takes its shard index and splits the rows into one KeywordDatabaseShard per index;
 * each shard then becomes a cuckoo table (above).  Here the rows are split on the device: a stable counting sort of the rows
 * by shard index and a gather of both byte blobs into the new order, so that the bytes that crossed PCIe once stay where
 * they are until every shard's Eval database is built. */

/* Sharding (KeywordDatabase.swift:152-242).  by_entry_count zero: .shardCount(value); nonzero: .entryCountPerShard(value).
 * has_max_shard_count zero: maxShardCount == nil.  require_power_of_two: nil and false behave alike in the reference. */
typedef struct he_keyword_sharding {
    int by_entry_count;
    uint64_t value;
    int has_max_shard_count;
    uint64_t max_shard_count;
    int require_power_of_two;
} he_keyword_sharding;
/* Sharding.init's checks (:186-204) and shardCount(for:) (:252-267): the flooring divide, max(.., 1), the cap and
 * previousPowerOfTwo.  Every invalidSharding case is HE_ERR_INVALID_SHARDING.  One difference from the reference: with
 * .entryCountPerShard and maxShardCount == 0 the reference resolves to 0 shards and would divide by zero in shardIndex; here
 * that is HE_ERR_INVALID_SHARDING.  NULL: HE_ERR_INVALID_ARGUMENT.  Host. */
int he_keyword_sharding_shard_count(const he_keyword_sharding* sharding, size_t row_count, size_t* out);

/* The partition.  All pointers DEVICE, any byte address for the four blobs; empty keywords and values are legal.
 *   keywords / values with keyword_offsets / value_offsets uint64 [count + 1], non-decreasing, as above; keyword_bytes /
 *   value_bytes = offsets[count] - offsets[0]: the sizes of out_keywords / out_values, which the caller has allocated
 *   shard_indices uint32 [count] (he_keyword_pir_shard_indices_device), shard_count in 1 .. 2^32 - 1
 *   out_order uint32 [count]: row j of the output is input row out_order[j]
 *   out_shard_starts uint32 [shard_count + 1]: shard s owns output rows out_shard_starts[s] .. out_shard_starts[s + 1], in
 *   input order (the reference iterates a Dictionary and defines no order; input order makes every table downstream
 *   reproducible).  shard_count 1 is the identity.
 *   out_keywords / out_values: the rows back to back in the new order; out_keyword_offsets / out_value_offsets uint64
 *   [count + 1]: their running sums, starting at 0.
 * Exactly the bytes of the six outputs are written and only bytes of the named inputs are read.  count up to 2^32 - 2.
 * device_mismatch (optional, a DEVICE word the caller has zeroed): bit 0 when an index is >= shard_count (the row goes to the
 * last shard), bit 1 when a blob's offsets do not span keyword_bytes / value_bytes (the bytes both agree on are written).
 * Nothing is written out of bounds either way.
 * The order comes from least-significant-digit passes of 8 bits over the order array alone (none for one shard, one up to
 * 256 shards); no blob byte moves before the order is final.  Enqueue-only; the second order array, the digit counts, the
 * scans' sums and the row every 512 output bytes start in are stream-ordered scratch.  he_keyword_database_partition_plan says
 * what a call runs. */
int he_keyword_database_partition_device(const uint8_t* keywords, const uint64_t* keyword_offsets, size_t keyword_bytes,
                                         const uint8_t* values, const uint64_t* value_offsets, size_t value_bytes,
                                         size_t count, const uint32_t* shard_indices, size_t shard_count,
                                         uint8_t* out_keywords, uint64_t* out_keyword_offsets, uint8_t* out_values,
                                         uint64_t* out_value_offsets, uint32_t* out_order, uint32_t* out_shard_starts,
                                         uint32_t* device_mismatch, he_stream s);
/* What he_keyword_database_partition_device runs for a shape.  Host only; any out pointer may be NULL.
 *   out_digit_passes: ceil(bits(shard_count - 1) / 8), 0 for one shard or no row
 *   out_workgroups_per_pass = ceil(count / out_rows_per_workgroup); out_last_workgroup_rows: the rows of the last one
 *   out_keyword_gather_form / out_value_gather_form: HE_KEYWORD_GATHER_NONE (no byte to move) or HE_KEYWORD_GATHER_CHUNK (a
 *   lane owns an aligned 8-byte chunk of the output blob) */
#define HE_KEYWORD_GATHER_NONE 0u
#define HE_KEYWORD_GATHER_CHUNK 1u
int he_keyword_database_partition_plan(size_t count, size_t shard_count, size_t keyword_bytes, size_t value_bytes,
                                       uint32_t* out_digit_passes, size_t* out_workgroups_per_pass,
                                       uint32_t* out_rows_per_workgroup, size_t* out_last_workgroup_rows,
                                       uint32_t* out_keyword_gather_form, uint32_t* out_value_gather_form);

/* The object: KeywordDatabase on the device.
 *   keywords DEVICE, keyword_offsets HOST [count + 1]; values DEVICE, value_offsets HOST [count + 1]: as the table object
 * The offsets are uploaded, the keywords hashed once, the shard indices derived (other_shard_count nonzero: doubleMod), the
 * rows partitioned, and one cuckoo table built per shard that received a row, over the partitioned blobs, which the object
 * owns; the input blobs are not referenced after the call returns.  Shard s's table is, field for field, the table
 * he_keyword_pir_table_create_device builds from that shard's rows in input order with seed + s (mod 2^64); its hashes are
 * gathered through the order, not computed again.  A shard without a row has no table (NULL, row count 0), as the reference
 * has no such shard (:423).  shard_table(s) and shard_values(s) are the `table` and `values` arguments of
 * he_keyword_pir_table_entries_device and he_keyword_pir_process_database_device.
 * One difference from the reference: it throws invalidDatabaseDuplicateKeyword here (:423-433); this library resolves
 * duplicates in the table by 64-bit hash with the first one winning (difference 1 above).  Equal keywords land in the same
 * shard, so nothing changes, and the shard table's duplicates_dropped is the report.
 * The call synchronises the stream.  Errors as he_keyword_pir_table_create_device; shard_count outside 1 .. 2^32 - 1:
 * HE_ERR_INVALID_ARGUMENT.  Destroy with he_keyword_database_destroy (NULL is fine). */
typedef struct he_keyword_database he_keyword_database;
int he_keyword_database_create_device(const he_cuckoo_table_config* config, const uint8_t* keywords,
                                      const uint64_t* keyword_offsets, const uint8_t* values,
                                      const uint64_t* value_offsets, size_t count, size_t shard_count,
                                      uint64_t other_shard_count, uint64_t seed, he_keyword_database** out, he_stream s);
void he_keyword_database_destroy(he_keyword_database* database);
size_t he_keyword_database_shard_count(const he_keyword_database* database);
size_t he_keyword_database_shard_row_count(const he_keyword_database* database, size_t shard);
const he_keyword_pir_table* he_keyword_database_shard_table(const he_keyword_database* database, size_t shard);
const uint8_t* he_keyword_database_shard_values(const he_keyword_database* database, size_t shard);
/* out_host HOST uint32 [count]: shard after shard, the input rows each holds */
int he_keyword_database_order(const he_keyword_database* database, uint32_t* out_host);

/* ---- processed-database files: ProcessedDatabase.serialize() / init(from:context:) ----------------------
 * The file PIRProcessDatabase writes and every index- and keyword-PIR server loads (PrivateInformationRetrieval/IndexPir/
 * IndexPirProtocol.swift:248-379):
 *   [version: 1 byte = 1 (:253-255)][plaintext count: UInt32 little-endian (:313-315, :367)], then per plaintext in array order
 *   tag 0 (serializedZeroPlaintextTag, :258-260) and nothing else, or tag 1 (serializedPlaintextTag, :263-265) followed by
 *   Plaintext<Eval>.serialize().poly: a bare PolyRq.serialize record over the top-level ciphertext context with skipLSBs 0,
 *   S = he_poly_serialization_byte_count(he_bfv_ciphertext_context(ctx, L), 0) bytes (:317-328, :369-376).
 * Array order is the order MulPirServer.process returns (MulPir.swift:487-503, :542-555): the flat [chunk_count][prod(
 * dimensions)] order of he_pir_process_database_device's database and present mask -- file index p is device slot p.  So the
 * tag of plaintext i lies at byte 5 + i + S rank(i), rank(i) the number of present plaintexts before i, and the file has
 * 5 + count + S popcount(present) bytes (:338-349).
 *
 * The three host entries need no device and work on host-only contexts. */

/* The walk along the tags, which is sequential by nature (where tag i lies depends on tags 0 .. i - 1): over `bytes`, the HOST
 * image of a file from its first byte.  present_out (HOST, `capacity` bytes; may be NULL) gets one byte per plaintext, 0 or 1.
 * Errors: a version other than 1 HE_ERR_INVALID_DATABASE_SERIALIZATION_VERSION; a tag other than 0 or 1
 * HE_ERR_INVALID_DATABASE_SERIALIZATION_PLAINTEXT_TAG; a buffer that ends inside the header, before a tag or inside a payload
 * HE_ERR_INVALID_ARGUMENT (the reference traps); present_out given with capacity below the file's count
 * HE_ERR_INVALID_ARGUMENT, nothing written.  Bytes after the last plaintext are ignored, as the reference ignores them:
 * out_bytes_consumed says where the file ended.  The out values (any may be NULL) are written on success only; after a tag or
 * truncation error present_out holds the plaintexts before it. */
int he_pir_database_file_scan(const he_bfv_context* ctx, const uint8_t* bytes, size_t byte_count, uint8_t* present_out,
                              size_t capacity, size_t* out_count, size_t* out_present_count, size_t* out_bytes_consumed);
/* ProcessedDatabase.serializationByteCount (:338-349) of a whole file with this HOST mask (a byte != 0: present): 5 + count +
 * S popcount; 5 for count 0.  count + S popcount of a range of the mask is the byte count of that segment of the body. */
int he_pir_database_file_byte_count(const he_bfv_context* ctx, const uint8_t* present, size_t count, size_t* out);
/* The version byte and the count (:366-367).  HE_ERR_INVALID_ARGUMENT for a count above UInt32.max. */
int he_pir_database_file_header(size_t count, uint8_t out[5]);

/* The body of a file, or any segment of it cut at a plaintext boundary, into the database: `records` (DEVICE, any address)
 * points at the TAG of the range's first plaintext, not at the file's first byte; present (DEVICE, [count]) and database
 * (DEVICE, [count][L][N] at the top level) are the range's.  A 30 GB file goes through a staging buffer in pieces this way,
 * and a keyword-PIR server loads its sub-tables one by one.  Every word of `database` is written: a present plaintext
 * (mask byte != 0) gets exactly the words he_poly_deserialize_device gives for its payload bytes -- fields are not validated,
 * fields at or above the modulus and set pad bits included -- a nil plaintext all zeros, which is what
 * he_pir_process_database_device produces.  Nothing outside [records, records + records_bytes) is read; bytes the range would
 * need past records_bytes read as zero.  Whether records_bytes covers count + S popcount cannot be known on the host without
 * the mask, and a kernel cannot throw: device_mismatch (optional, a DEVICE word the caller has zeroed) gets bit 0 when the
 * range needs more than records_bytes and bit 1 when a tag byte is not the one the mask implies.
 * Errors, all before anything is enqueued: null pointers and `database` overlapping `records` HE_ERR_INVALID_ARGUMENT; a
 * context of more than 64 moduli HE_ERR_UNSUPPORTED; a host-only context HE_ERR_DEVICE.  Enqueue-only: a prefix count of the
 * mask into stream-ordered scratch (4 bytes per plaintext), then one launch. */
int he_pir_database_load_device(const he_bfv_context* ctx, const uint8_t* records, size_t records_bytes,
                                const uint8_t* present, size_t count, uint64_t* database, uint32_t* device_mismatch,
                                he_stream s);
/* The inverse: tags and payloads of the range into `records` (no 5-byte header: he_pir_database_file_header).  The slab of a
 * plaintext whose mask byte is 0 is ignored and need not be zero.  Exactly the bytes [records, records + min(records_bytes,
 * count + S popcount)) are written and no byte of the buffer is read: an aligned 8-byte chunk inside a payload is one store,
 * a chunk that holds a payload's first or last bytes is byte stores.  device_mismatch bit 0 as above.  Same errors. */
int he_pir_database_save_device(const he_bfv_context* ctx, const uint64_t* database, const uint8_t* present, size_t count,
                                uint8_t* records, size_t records_bytes, uint32_t* device_mismatch, he_stream s);
/* The same on the packed 4-byte slabs of a Bfv<UInt32> context (HE_ERR_INVALID_ARGUMENT on any other). */
int he_pir_database_load_device_u32(const he_bfv_context* ctx, const uint8_t* records, size_t records_bytes,
                                    const uint8_t* present, size_t count, uint32_t* database, uint32_t* device_mismatch,
                                    he_stream s);
int he_pir_database_save_device_u32(const he_bfv_context* ctx, const uint32_t* database, const uint8_t* present,
                                    size_t count, uint8_t* records, size_t records_bytes, uint32_t* device_mismatch,
                                    he_stream s);

/* ---- PNNS server database (PrivateNearestNeighborSearch/) ------------------------------------------------------------------
 * Database.process (ProcessedDatabase.swift:194-229) for one context, on the device: the float vectors are normalised,
 * scaled and rounded, packed diagonally into SIMD plaintexts (PlaintextMatrix.swift:417-483) and converted to Eval form.
 * The result is the PlaintextMatrix<Scheme, Eval> that mulTranspose(vector:) (MatrixMultiplication.swift:131-226) reads:
 * he_pnns_mul_transpose_device / he_pnns_compute_response_device below.
 *
 * he_pnns_context -- what a he_bfv_context lacks for Context.encode(values:format: .simd): plaintextContext, the PolyContext
 * over [t] (Context.swift:128-130) with its NTT tables on the device, and simdEncodingMatrix (generateEncodingMatrix,
 * Encoding.swift:197-219), built on the host and uploaded once.  t not an NTT modulus for N: HE_ERR_SIMD_ENCODING_NOT_SUPPORTED
 * (Encoding.swift:225).  A host-only BFV context gives a host-only PNNS context: he_pnns_matrix_shape works, device entry
 * points return HE_ERR_DEVICE.  The BFV context is borrowed and must outlive the PNNS context.  he_pnns_context_create takes a
 * Context<Bfv<UInt64>>, he_pnns_context_create_u32 a Context<Bfv<UInt32>> (HE_ERR_INVALID_ARGUMENT for the other kind).
 * Synchronises (tables are uploaded).  Destroy (NULL is accepted) once the work enqueued with it is done. */
typedef struct he_pnns_context he_pnns_context;
int he_pnns_context_create(const he_bfv_context* ctx, he_pnns_context** out);
int he_pnns_context_create_u32(const he_bfv_context* ctx, he_pnns_context** out);
void he_pnns_context_destroy(he_pnns_context* ctx);
/* MatrixPacking (PlaintextMatrix.swift:21-37), in the reference's case order */
enum { HE_PNNS_PACKING_DENSE_COLUMN = 0, HE_PNNS_PACKING_DENSE_ROW = 1, HE_PNNS_PACKING_DIAGONAL = 2 };
/* PlaintextMatrix.plaintextCount (PlaintextMatrix.swift:246-275) and BabyStepGiantStep.init (MatrixMultiplication.swift:
 * 33-60).  Host only.  baby_step 0: the default, ceil(sqrt(nextPowerOfTwo(column_count))); otherwise giant_step =
 * ceil(nextPowerOfTwo(column_count) / baby_step).  Any out pointer may be NULL.  HE_ERR_INVALID_ARGUMENT: baby_step <
 * giant_step (the reference's precondition), zero rows or columns (invalidMatrixDimensions), column_count > N / 2 under
 * denseRow or diagonal, an unknown packing. */
int he_pnns_matrix_shape(const he_pnns_context* ctx, size_t row_count, size_t column_count, int packing, uint32_t baby_step,
                         size_t* out_plaintext_count, uint32_t* out_baby_step, uint32_t* out_giant_step);
/* Array2d<Float>.normalizedScaledAndRounded (PrivateNearestNeighborSearch/Util.swift:74-89), bit-exact: per row the float32
 * sum of squares accumulated left to right from 0, its correctly rounded square root, then (v * scaling_factor) / norm
 * rounded half away from zero; a row of norm 0 gives zeros.  vectors DEVICE [rows][cols] float32 row-major, out DEVICE
 * [rows][cols] int64 (the reference's Array2d<SignedScalar>).  Enqueue-only on `s`. */
int he_pnns_quantize_rows_device(const float* vectors, size_t rows, size_t cols, float scaling_factor, int64_t* out,
                                 he_stream s);
/* PlaintextMatrix(context:dimensions:packing: .diagonal(bsgs), signedValues:reduce:).convertToEvalFormat(moduliCount:)
 * (PlaintextMatrix.swift:165-188, 417-483; Encoding.swift:222-234; Plaintext.swift:149-170).
 *   signed_values  DEVICE [rows][cols] int64 row-major
 *   baby_step      as in he_pnns_matrix_shape
 *   reduce         nonzero: values go through Modulus.reduce for signed input (the plaintext-CRT case,
 *                  ProcessedDatabase.swift:213-220); 0: centeredToRemainder, and a value outside [-(t >> 1), (t - 1) >> 1]
 *                  sets *out_of_range to 1 (its plaintext is then unspecified)
 *   out            DEVICE [plaintext_count][moduli_count][N] Eval; plaintext index = diagonal * plaintextsPerColumn + chunk,
 *                  the reference's append order
 *   out_of_range   DEVICE, one word the caller zeroes; may be NULL
 * Enqueue-only on `s` and capturable; staging comes from the library's stream-ordered scratch, in groups of plaintexts of
 * about 1 GiB of output.  Argument errors (those of he_pnns_matrix_shape, a moduli_count out of range, a null pointer, a
 * context of the other word size) are returned before anything is enqueued.  A host-only context: HE_ERR_DEVICE. */
int he_pnns_diagonal_matrix_device(const he_pnns_context* ctx, const int64_t* signed_values, size_t rows, size_t cols,
                                   uint32_t baby_step, int reduce, uint32_t moduli_count, uint64_t* out,
                                   uint32_t* out_of_range, he_stream s);
/* The same for a Bfv<UInt32> context, the matrix in packed 4-byte words. */
int he_pnns_diagonal_matrix_device_u32(const he_pnns_context* ctx, const int64_t* signed_values, size_t rows, size_t cols,
                                       uint32_t baby_step, int reduce, uint32_t moduli_count, uint32_t* out,
                                       uint32_t* out_of_range, he_stream s);

/* ---- PNNS server response (PrivateNearestNeighborSearch/Server.swift:61-88) ------------------------------------------------
 * PlaintextMatrix.mulTranspose(vector:using:) (MatrixMultiplication.swift:131-226) for `query_count` independent one-row
 * query vectors against one diagonally packed matrix, in one call.  For a one-row CiphertextMatrix, mulTranspose(matrix:using:)
 * (:236-276) is this: extractDenseRow returns the ciphertext itself and the column packing is rotateColumnsAndSum of one
 * element.  With P = nextPowerOfTwo(cols), G = ceil(P / baby_step), C = ceil(rows / N), L = he_bfv_ciphertext_moduli_count:
 *   matrix                  DEVICE [P C][L][N] Eval, 16-byte aligned: what he_pnns_diagonal_matrix_device writes at moduli_count L
 *   matrix_plaintext_count  the plaintexts the matrix holds; anything but P C is the reference's invalidMatrixDimensions
 *                           (:147-149: the query's column count does not match the matrix): HE_ERR_INVALID_ARGUMENT
 *   rows, cols              the matrix's dimensions; shape errors as he_pnns_matrix_shape under HE_PNNS_PACKING_DIAGONAL
 *   baby_step               the one the matrix was packed with (the packing carries it, :137); 0 is HE_ERR_INVALID_ARGUMENT
 *   queries                 DEVICE [query_count][2][L][N] Coeff: each client's dense-row packed vector
 *   galois_keys             HOST [query_count][2] device pointers (he_bfv_apply_galois_device's key layout): query q's keys of
 *                           rotatingColumns(by: -1) at [2 q] and of rotatingColumns(by: -baby_step) at [2 q + 1].  The first is
 *                           needed when baby_step > 1 (:182-187), the second when G > 1 (HeScheme.swift:113-133); a needed key
 *                           that is NULL (or the array) is HE_ERR_MISSING_GALOIS_KEY; one that is not needed is not read
 *   out                     DEVICE [query_count][C][2][L][N] Coeff: mulTranspose's result ciphertexts per query
 * The order of operations is the reference's and every word equals its: baby_step - 1 serial rotations by -1 (not hoisted),
 * each one batch over the queries; every state to Eval; the inner products of all giant steps (Bfv.swift:476-505) in one pass
 * over the matrix for up to four queries at a time; inverse NTT; then G - 1 times rotate by -baby_step and add, each one batched
 * key switch over all query_count x C accumulators.  Enqueue-only on `s`; scratch comes from the library's stream-ordered
 * cache, the inner products in groups of result ciphertexts of about 2 GiB.  Argument errors are returned before anything is
 * enqueued, in the order above; query_count 0 is HE_OK.  A host-only context: HE_ERR_DEVICE. */
int he_pnns_mul_transpose_device(const he_pnns_context* ctx, const uint64_t* matrix, size_t matrix_plaintext_count, size_t rows,
                                 size_t cols, uint32_t baby_step, const uint64_t* queries, size_t query_count,
                                 const uint64_t* const* galois_keys, uint64_t* out, he_stream s);
/* The same for a Bfv<UInt32> context on packed 4-byte words (matrix, queries, keys and out), batched as above. */
int he_pnns_mul_transpose_device_u32(const he_pnns_context* ctx, const uint32_t* matrix, size_t matrix_plaintext_count,
                                     size_t rows, size_t cols, uint32_t baby_step, const uint32_t* queries, size_t query_count,
                                     const uint32_t* const* galois_keys, uint32_t* out, he_stream s);
/* Server.computeResponse (Server.swift:61-88) for such queries: the same, then Ciphertext.modSwitchDownToSingle
 * (Bfv.swift:163-171) and Coeff form (:84-86).  out DEVICE [query_count][C][2][1][N] Coeff over q_0: what
 * Response.ciphertextMatrices holds. */
int he_pnns_compute_response_device(const he_pnns_context* ctx, const uint64_t* matrix, size_t matrix_plaintext_count,
                                    size_t rows, size_t cols, uint32_t baby_step, const uint64_t* queries, size_t query_count,
                                    const uint64_t* const* galois_keys, uint64_t* out, he_stream s);
int he_pnns_compute_response_device_u32(const he_pnns_context* ctx, const uint32_t* matrix, size_t matrix_plaintext_count,
                                        size_t rows, size_t cols, uint32_t baby_step, const uint32_t* queries,
                                        size_t query_count, const uint32_t* const* galois_keys, uint32_t* out, he_stream s);

/* ---- PNNS server response to query matrices of several rows ---------------------------------------------------------------
 * PlaintextMatrix.mulTranspose(matrix:using:) (MatrixMultiplication.swift:236-298) for `query_count` clients, each with a
 * dense-row packed CiphertextMatrix of `query_rows` rows: per row CiphertextMatrix.extractDenseRow (CiphertextMatrix.swift:
 * 252-370) and mulTranspose(vector:), then the dense-column packing of the per-row results (:267-290).  With N the degree,
 * P = nextPowerOfTwo(cols), R = query_rows, C = ceil(rows / N), cps = (N / 2) / rows (columnsPerSimdRowCount):
 *   K = ceil(R / (2 (N / 2) / P))    ciphertexts of a query (PlaintextMatrix.plaintextCount under denseRow)
 *   M = ceil(R / (2 cps)) when cps > 0, else R C    result ciphertexts of a client, in the order of `innerProducts` (:265, :289)
 *
 * he_pnns_query_matrix_shape -- host only: K, M and which keys the shape needs: bit i of *out_pack_needs for slot i < 4 of
 * galois_keys below, bit 4 for the rotation plan and its keys.  Bits 0 and 1 are those of the default baby step (baby_step is
 * no argument here); for another one they are as in he_pnns_mul_transpose_device.  Any out pointer may be NULL.
 * HE_ERR_INVALID_ARGUMENT: cols > N / 2, zero rows, columns or query rows (invalidMatrixDimensions). */
int he_pnns_query_matrix_shape(const he_pnns_context* ctx, size_t matrix_rows, size_t cols, size_t query_rows,
                               size_t* out_query_ciphertexts, size_t* out_result_ciphertexts, uint32_t* out_pack_needs);
/* One step of the plan rotateColumnsMultiStep(by: rows) executes (_HomomorphicEncryptionExtras/HeScheme.swift:21-60):
 * `count` rotations by `step` columns. */
typedef struct he_pnns_pack_step {
    int64_t step;
    uint32_t count;
} he_pnns_pack_step;
/*   matrix .. baby_step     as in he_pnns_mul_transpose_device
 *   queries                 DEVICE [query_count][K][2][L][N] Coeff, 16-byte aligned: each client's query (denseRowPlaintexts,
 *                           PlaintextMatrix.swift:341-406)
 *   pack_steps              HOST [pack_step_count], in application order: the plan of rotateColumnsMultiStep(by: rows).  The
 *                           reference iterates a Swift Dictionary, so its order -- and with it every word of the result -- is
 *                           the caller's to know.  The single pair {rows, 1} when the key holds rotatingColumns(by: rows).
 *                           HE_ERR_INVALID_ARGUMENT when the steps do not sum to rows mod N / 2 or one is outside
 *                           [1, N / 2 - 1].  Read only when cps >= 2 and R >= 2
 *   galois_keys             HOST [query_count][4 + pack_step_count] device pointers per client: [0] rotatingColumns(by: -1),
 *                           [1] (by: -baby_step), [2] swappingRows, [3] rotatingColumns(by: P), [4 + i] the key of
 *                           pack_steps[i].step.  Needed: [0] and [1] as in he_pnns_mul_transpose_device; [2] when R > 1
 *                           (extractDenseRow) or cps > 0 and R > cps (swapRowsAndAdd); [3] when R > 1 and some row's
 *                           rotateCount > 0; the plan's when cps >= 2 and R >= 2.  A needed key that is NULL is
 *                           HE_ERR_MISSING_GALOIS_KEY; one that is not needed is not read
 *   out                     DEVICE [query_count][M][2][L][N] Coeff
 * The order of operations is the reference's and every word equals its; only independent items share a launch.  The masks
 * depend on (N, cols, R) alone and are built once per call; every query ciphertext goes to Eval once and is read once for all
 * the rows packed in it; a step of the replication (:347-353) is one key switch over every (client, row) that still rotates;
 * the rows of all clients share the passes over the matrix four at a time; a step of the packing sums (HeScheme.swift:113-133)
 * is one key switch over every half-chunk of every client that has an element left.  With R = 1 every word is
 * he_pnns_mul_transpose_device's.  Enqueue-only on `s`, scratch from the stream-ordered cache; argument errors in the order
 * above, before anything is enqueued; query_count 0 is HE_OK; a host-only context: HE_ERR_DEVICE. */
int he_pnns_mul_transpose_matrix_device(const he_pnns_context* ctx, const uint64_t* matrix, size_t matrix_plaintext_count,
                                        size_t rows, size_t cols, uint32_t baby_step, const uint64_t* queries,
                                        size_t query_rows, size_t query_count, const he_pnns_pack_step* pack_steps,
                                        size_t pack_step_count, const uint64_t* const* galois_keys, uint64_t* out, he_stream s);
/* The same on packed 4-byte words. */
int he_pnns_mul_transpose_matrix_device_u32(const he_pnns_context* ctx, const uint32_t* matrix, size_t matrix_plaintext_count,
                                            size_t rows, size_t cols, uint32_t baby_step, const uint32_t* queries,
                                            size_t query_rows, size_t query_count, const he_pnns_pack_step* pack_steps,
                                            size_t pack_step_count, const uint32_t* const* galois_keys, uint32_t* out,
                                            he_stream s);
/* Server.computeResponse (Server.swift:61-88) for such queries: the same, then modSwitchDownToSingle over the M results of
 * every client.  out DEVICE [query_count][M][2][1][N] Coeff over q_0. */
int he_pnns_compute_response_matrix_device(const he_pnns_context* ctx, const uint64_t* matrix, size_t matrix_plaintext_count,
                                           size_t rows, size_t cols, uint32_t baby_step, const uint64_t* queries,
                                           size_t query_rows, size_t query_count, const he_pnns_pack_step* pack_steps,
                                           size_t pack_step_count, const uint64_t* const* galois_keys, uint64_t* out,
                                           he_stream s);
int he_pnns_compute_response_matrix_device_u32(const he_pnns_context* ctx, const uint32_t* matrix,
                                               size_t matrix_plaintext_count, size_t rows, size_t cols, uint32_t baby_step,
                                               const uint32_t* queries, size_t query_rows, size_t query_count,
                                               const he_pnns_pack_step* pack_steps, size_t pack_step_count,
                                               const uint32_t* const* galois_keys, uint32_t* out, he_stream s);

/* ---- PNNS client (PrivateNearestNeighborSearch/Client.swift:74-127) --------------------------------------------------------
 * Client.generateQuery(for:using:) and Client.decrypt(response:using:) on the device, and the two layers under them as entries
 * of their own.  The conventions of the decrypt and encrypt entries hold for all of them: the slab word is an argument
 * (word_bits 32 or 64, packed 4-byte or 8-byte words; it must be the word of the context's scheme -- he_pnns_context_create
 * for 64, he_pnns_context_create_u32 for 32 -- else HE_ERR_INVALID_ARGUMENT) and there are no _u32 twins; enqueue-only on `s`;
 * scratch comes from the library's stream-ordered cache; every argument error (in the order of the argument lists below: the
 * word, the contexts, the shape, null buffers, buffers that overlap one the call writes) is returned before anything is
 * enqueued; a host-only context is HE_ERR_DEVICE after the argument checks; an empty batch does nothing.
 *
 * Layer 1 -- Context.encodeSimd / decodeSimd (Encoding.swift:222-245) for `batch` plaintexts.
 *   slots / out_slots            DEVICE [batch][N] words in slot order; a caller with fewer than N values pads with zeros, as
 *                                encodeSimd does
 *   plaintexts / out_plaintexts  DEVICE [batch][N] Coeff words below t
 *   out_of_range                 DEVICE, one word the caller zeroes, may be NULL: set to 1 when a slot value is not below t
 *                                (validDataForEncoding); that plaintext is then unspecified
 * Encoding scatters value i to word simdEncodingMatrix[i] -- written as a gather through the inverse table, so the stores are
 * contiguous -- into out_plaintexts and runs the inverse NTT over [t] there; decoding runs the forward NTT on a scratch copy
 * (the input is never written) and reads out_slots[b][i] = transformed[b][simdEncodingMatrix[i]]. */
int he_pnns_simd_encode_device(const he_pnns_context* ctx, uint32_t word_bits, const void* slots, size_t batch,
                               void* out_plaintexts, uint32_t* out_of_range, he_stream s);
int he_pnns_simd_decode_device(const he_pnns_context* ctx, uint32_t word_bits, const void* plaintexts, size_t batch,
                               void* out_slots, he_stream s);
/* Layer 2 -- PlaintextMatrix(context:dimensions:packing: .denseRow, signedValues:reduce:) (PlaintextMatrix.swift:165-236,
 * 341-406) and PlaintextMatrix.unpack() -> [Scalar] (:489-590).
 *   signed_values   DEVICE [rows][cols] int64 row-major; reduce and out_of_range exactly as in he_pnns_diagonal_matrix_device
 *   out_plaintexts  DEVICE [K][N] Coeff, K from he_pnns_matrix_shape(.., HE_PNNS_PACKING_DENSE_ROW, ..)
 *   packing         of the plaintexts handed to unpack: HE_PNNS_PACKING_DENSE_COLUMN (unpackDenseColumn, with its transposition
 *                   to row-major) or HE_PNNS_PACKING_DENSE_ROW; plaintexts DEVICE [count][N] Coeff, count from
 *                   he_pnns_matrix_shape under that packing
 *   out_values      DEVICE [rows][cols] uint64 row-major, values below t
 * Packing is one kernel with a lane per slab word of all K plaintexts -- word -> slot -> (row, column) or zero in closed form,
 * the zero padding to nextPowerOfTwo(cols) and the repeated rows of the last plaintext (:388-402) included -- and the inverse
 * NTT in out_plaintexts; unpacking is the forward NTT on a scratch copy and one kernel with a lane per value.  Shape errors are
 * those of he_pnns_matrix_shape; more than 2^40 values or slab words: HE_ERR_INVALID_ARGUMENT.
 * Out of scope: dense-column PACKING and diagonal UNPACKING -- nothing on the device produces a matrix to pack by columns or
 * consumes an unpacked diagonal matrix.  he_pnns_unpack_device under HE_PNNS_PACKING_DIAGONAL is HE_ERR_UNSUPPORTED, and there is
 * no he_pnns_pack_dense_columns_device. */
int he_pnns_pack_dense_rows_device(const he_pnns_context* ctx, uint32_t word_bits, const int64_t* signed_values, size_t rows,
                                   size_t cols, int reduce, void* out_plaintexts, uint32_t* out_of_range, he_stream s);
int he_pnns_unpack_device(const he_pnns_context* ctx, uint32_t word_bits, int packing, const void* plaintexts, size_t rows,
                          size_t cols, uint64_t* out_values, he_stream s);
/* Layer 3 -- the client.  ctxs: a HOST array of context_count PNNS contexts, one per plaintext modulus (Client.contexts).
 * HE_ERR_INVALID_ARGUMENT: context_count 0 or above 8, a NULL context, contexts that differ in degree, coefficient moduli or
 * word, two equal plaintext moduli, 2 x the product of the plaintext moduli above UInt64.max (compose's precondition,
 * CrtComposer.swift:78-79); HE_ERR_NOT_INVERTIBLE: plaintext moduli that are not pairwise coprime.
 *
 * he_pnns_generate_query_device -- Client.generateQuery(for:using:) (Client.swift:74-91):
 *   vectors        DEVICE [query_rows][cols] float32 row-major
 *   secret_key     as he_bfv_encrypt_device reads it
 *   a_seeds, error_seeds   DEVICE [context_count][K][32], K the dense-row plaintext count of a query_rows x cols matrix
 *   out            DEVICE [context_count][K][2][L][N] Coeff, L = he_bfv_ciphertext_moduli_count: slice c is a client's argument
 *                  `queries` of he_pnns_compute_response_matrix_device under context c
 *   out_of_range   as in layer 2 (one context: reduce is off, Client.swift:81)
 *   workspace      DEVICE, 16-byte aligned, he_pnns_generate_query_workspace_bytes bytes, or NULL: stream-ordered scratch
 * One normalizedScaledAndRounded (he_pnns_quantize_rows_device's kernel), then per context layer 2 with reduce =
 * (context_count > 1) and he_bfv_encrypt_device at L moduli: every word equals that composition on the same seeds.  The
 * quantised values, the plaintexts and the encryption's own scratch depend on the user's query: the whole workspace is
 * overwritten with zeros on the stream before it is released or the entry returns (as he_bfv_encrypt_device's).
 *
 * he_pnns_decrypt_response_device -- Client.decrypt(response:using:) (Client.swift:100-127):
 *   response       DEVICE [context_count][M][2][moduli_count][N] Coeff, M the dense-column plaintext count of a
 *                  rows x query_rows matrix; moduli_count is 1 for a Response (he_pnns_compute_response_matrix_device's out per
 *                  context), any level is allowed
 *   out_distances  DEVICE [rows][query_rows] float32 row-major
 *   workspace      as above, he_pnns_decrypt_response_workspace_bytes bytes
 * Per context he_bfv_decrypt_device (correction factor 1) and the forward NTT over that context's [t_i]; then one kernel with
 * a lane per distance: it gathers its residue from every context's transformed plaintexts (dense-column position -> slot ->
 * simdEncodingMatrix), composes them as CrtComposer.compose does -- acc = addMod(acc, ((inv_i x_i) mod t_i) (q / t_i), q) in
 * UInt64, in row order, inversePuncturedProducts from the host, q the product of the t_i; skipped for one context --, centres the
 * result (remainderToCentered(modulus: q)) and returns Float(signed) / (scaling_factor * scaling_factor): the float product is
 * formed first, the division is one correctly rounded division.  Plaintexts go through the workspace in groups of about 1 GiB,
 * one kernel per group.  The decrypted plaintexts and the decryption's own scratch are zeroized as above.
 *
 * The two *_workspace_bytes are host only and return 0 for arguments the entries refuse. */
size_t he_pnns_generate_query_workspace_bytes(const he_pnns_context* const* ctxs, size_t context_count, uint32_t word_bits,
                                              size_t query_rows, size_t cols);
int he_pnns_generate_query_device(const he_pnns_context* const* ctxs, size_t context_count, uint32_t word_bits,
                                  const float* vectors, size_t query_rows, size_t cols, float scaling_factor,
                                  const void* secret_key, const uint8_t* a_seeds, const uint8_t* error_seeds, void* out,
                                  uint32_t* out_of_range, void* workspace, size_t workspace_bytes, he_stream s);
size_t he_pnns_decrypt_response_workspace_bytes(const he_pnns_context* const* ctxs, size_t context_count, uint32_t word_bits,
                                                uint32_t moduli_count, size_t rows, size_t query_rows);
int he_pnns_decrypt_response_device(const he_pnns_context* const* ctxs, size_t context_count, uint32_t word_bits,
                                    uint32_t moduli_count, const void* response, const void* secret_key, size_t rows,
                                    size_t query_rows, float scaling_factor, float* out_distances, void* workspace,
                                    size_t workspace_bytes, he_stream s);

/* ---- SimplePirServer (PrivateInformationRetrieval/SimplePir/)------------------------------------------------------------
 * The other index-PIR server: a database matrix of plaintext_bits-wide elements, a hint for the clients, and replies that
 * are one wrap-around integer matrix product.  word_bits is the reference's Scalar: 64 (entries without suffix) or 32
 * (_u32: 4-byte request / response / hint words).
 *
 * Device layout of the database: the reference's transposed processedDatabase, [column_size][database_columns] row-major,
 * each element in element_bytes = 1 (plaintext_bits <= 8), 2 (<= 16), 4 (<= 32) or 8 bytes instead of a whole Scalar;
 * padding elements are zero.  A reply streams the database once, so its stored bytes are the reply's time.  Every `database`
 * pointer below must be aligned to element_bytes (HE_ERR_INVALID_ARGUMENT otherwise); the reply reads 16 bytes per lane when
 * the pointer is 16-byte aligned and database_columns x element_bytes is a multiple of 16, element by element otherwise.
 *
 * he_simple_pir_shape -- SimplePirServerProtocol.computingParams (SimplePir+Database.swift:209-243), the padded column size
 * of process (:262-268), SimplePirParameters.aPolyCount (:171-175) and SimplePirContext.init's modulus
 * (SimplePirContext.swift:76-87).  Host only: no device is touched.
 *   out_entry_size_in_scalar  ceil(8 entry_size_in_bytes / plaintext_bits)
 *   out_entries_per_column, out_chunks_per_entry, out_database_columns   as the reference rounds them (Double.rounded():
 *                             halves away from zero; the max(.., 1) clamps)
 *   out_column_size           rows of the database = words of one reply
 *   out_a_poly_count          ceil(database_columns / lattice_dimension)
 *   out_modulus               the NTT-friendly prime p of ciphertext_bits + 1 significant bits, preferring small
 *   out_element_bytes         1, 2, 4 or 8
 * Any out pointer may be NULL.  HE_ERR_INVALID_ARGUMENT: word_bits not 32 / 64, plaintext_bits 0, ciphertext_bits <=
 * plaintext_bits, ciphertext_bits above 29 (word_bits 32: p must be a PolyRq<UInt32> modulus) or 60 (word_bits 64),
 * lattice_dimension not a power of two, an empty database, or a shape with entries_per_column and chunks_per_entry both
 * above 1 (SimplePirParameters.init's precondition, SimplePir.swift:157).  HE_ERR_NOT_ENOUGH_PRIMES: no such prime. */
int he_simple_pir_shape(uint32_t plaintext_bits, uint32_t ciphertext_bits, uint32_t lattice_dimension, uint32_t word_bits,
                        size_t entry_count, size_t entry_size_in_bytes, size_t* out_entry_size_in_scalar,
                        size_t* out_entries_per_column, size_t* out_chunks_per_entry, size_t* out_database_columns,
                        size_t* out_column_size, size_t* out_a_poly_count, uint64_t* out_modulus,
                        uint32_t* out_element_bytes);
/* SimplePirContext<Scalar>.init(params:) (SimplePirContext.swift:76-87) for process: the plan above and extraContext
 * (degree lattice_dimension, the one modulus p) on the current device.  Same errors as he_simple_pir_shape, and
 * HE_ERR_DEVICE without a device.  Synchronises (tables are uploaded).  Destroy with he_simple_pir_context_destroy (NULL
 * is accepted) once the work enqueued with it is done. */
typedef struct he_simple_pir_context he_simple_pir_context;
int he_simple_pir_context_create(uint32_t plaintext_bits, uint32_t ciphertext_bits, uint32_t lattice_dimension,
                                 uint32_t word_bits, size_t entry_count, size_t entry_size_in_bytes,
                                 he_simple_pir_context** out);
void he_simple_pir_context_destroy(he_simple_pir_context* ctx);
/* SimplePirServerProtocol.process(database:encryptionParams:seed:) (SimplePir+Database.swift:252-290) on the device.
 *   entries   DEVICE [entry_count][entry_size_in_bytes] (RawDatabase)
 *   seed      DEVICE [32], the NistAes128Ctr seed of generateAPolynomials (:178-181)
 *   database  DEVICE [column_size][database_columns] elements of element_bytes (layout above), written whole
 *   hint      DEVICE [column_size][lattice_dimension] words mod p, 16-byte aligned: database x A mod p (:279-281)
 * The matrix A (materializeAMatrix, :186-206) is not formed: with a_k the seeded polynomials and d_{r,k} the k-th block of
 * lattice_dimension elements of database row r, hint row r = sum_k d_{r,k} * a_k(x^(2N-1)) in Z_p[x]/(x^N + 1), computed
 * with the forward / inverse NTT in blocks of rows.  Enqueue-only on `s`; scratch comes from the library's stream-ordered
 * cache.  The context must be of the entry's word size (HE_ERR_INVALID_ARGUMENT otherwise). */
int he_simple_pir_process_database_device(const he_simple_pir_context* ctx, const uint8_t* entries, const uint8_t* seed,
                                          void* database, uint64_t* hint, he_stream s);
int he_simple_pir_process_database_device_u32(const he_simple_pir_context* ctx, const uint8_t* entries, const uint8_t* seed,
                                              void* database, uint32_t* hint, he_stream s);
/* The reference's wide image of a processed database (Array2d<Scalar>.data of SimplePirDatabase, `elements` words) to the
 * device layout and back: what a server that loaded a saved database (SimplePirDatabase.init(from:),
 * SimplePir+Database.swift:86-106) calls before it answers.  Both DEVICE, element-wise, enqueue-only.  pack keeps the low
 * plaintext_bits of every word: a word at or above 2^plaintext_bits is masked, not rejected (rejecting would need a
 * read-back).  HE_ERR_INVALID_ARGUMENT: plaintext_bits 0 or above the word. */
int he_simple_pir_pack_database_device(uint32_t plaintext_bits, const uint64_t* wide, void* database, size_t elements,
                                       he_stream s);
int he_simple_pir_pack_database_device_u32(uint32_t plaintext_bits, const uint32_t* wide, void* database, size_t elements,
                                           he_stream s);
int he_simple_pir_unpack_database_device(uint32_t plaintext_bits, const void* database, uint64_t* wide, size_t elements,
                                         he_stream s);
int he_simple_pir_unpack_database_device_u32(uint32_t plaintext_bits, const void* database, uint32_t* wide, size_t elements,
                                             he_stream s);
/* SimplePirServer.computeResponse(to:) (SimplePir+Server.swift:31-38; Array2d.multiply(transposing:mask:),
 * SimplePir+Precompute.swift:51-114) for a batch of stacked requests:
 *   responses[q][r] = (sum_c database[r][c] * requests[q][c]) & (2^ciphertext_bits - 1)
 *   database   DEVICE [column_size][database_columns] in the layout above (plaintext_bits selects element_bytes)
 *   requests   DEVICE [query_count][database_columns] words (Requests, one request per row)
 *   responses  DEVICE [query_count][column_size] words (the reference's transposed result)
 * query_count is free: requests are answered eight to a pass over the database.  Enqueue-only on `s`, no scratch.
 * ciphertext_bits may be anything up to the word here (the product needs no prime; he_simple_pir_shape stops at 29 / 60
 * because process does).  HE_ERR_INVALID_ARGUMENT: ciphertext_bits <= plaintext_bits or above the word, a misaligned
 * database. */
int he_simple_pir_compute_response_device(uint32_t plaintext_bits, uint32_t ciphertext_bits, const void* database,
                                          size_t column_size, size_t database_columns, const uint64_t* requests,
                                          size_t query_count, uint64_t* responses, he_stream s);
int he_simple_pir_compute_response_device_u32(uint32_t plaintext_bits, uint32_t ciphertext_bits, const void* database,
                                              size_t column_size, size_t database_columns, const uint32_t* requests,
                                              size_t query_count, uint32_t* responses, he_stream s);

/* computeResponse for LARGE request batches, on the int8 matrix cores (v_mfma_i32_16x16x64_i8).  Layouts, argument checks,
 * error codes and results are those of he_simple_pir_compute_response_device(_u32): the words are identical.  The modulus
 * is a power of two, so the product splits exactly into 7-bit limbs; one read of the database answers
 * `requests_per_pass` requests (32, or 16 above 4 / 6 shift classes at 4- / 8-byte words) instead of eight.
 * The matrix kernel covers 1-byte elements with plaintext_bits <= 7 and 2-byte elements with plaintext_bits <= 14, at both
 * word sizes and every ciphertext_bits the entry above accepts; for plaintext_bits 8, 15, 16 and the 4- and 8-byte
 * elements the call runs the existing reply kernel.  he_simple_pir_batch_response_plan says which, without a device.
 * PRECONDITION on the matrix path: every element is below 2^plaintext_bits, as process and pack produce them -- a stray
 * high bit would be read as a sign (the entry above multiplies whatever the element holds).  Request words may hold
 * anything: bits at and above ciphertext_bits fall out under the final mask, as there.
 * Enqueue-only on `s`, no scratch.
 * When to call it: measured on one MI355X over 32768 x 32768 elements, this entry is the faster one from
 * query_count 4 at 7 / 28 bits in 4-byte words and from 8 at 14 / 42 bits in 8-byte words (9 - 10 x at 32 and more); for a
 * single request the entry above is faster (0.20 against 0.27 ms, 0.35 against 0.70 ms). */
int he_simple_pir_compute_response_batch_device(uint32_t plaintext_bits, uint32_t ciphertext_bits, const void* database,
                                                size_t column_size, size_t database_columns, const uint64_t* requests,
                                                size_t query_count, uint64_t* responses, he_stream s);
int he_simple_pir_compute_response_batch_device_u32(uint32_t plaintext_bits, uint32_t ciphertext_bits, const void* database,
                                                    size_t column_size, size_t database_columns, const uint32_t* requests,
                                                    size_t query_count, uint32_t* responses, he_stream s);
/* What the batch entries do for a shape.  Host only: callable without a GPU.  Any out pointer may be NULL.
 * HE_ERR_INVALID_ARGUMENT: word_bits not 32 / 64, ciphertext_bits <= plaintext_bits or above the word.
 * HEAMD_SIMPLE_PIR_FOLD_COLUMNS=<columns> lowers the fold cadence (to a multiple of 64, never below 64) and never raises
 * it; the plan reports the cadence in force.  Off the matrix path database_limbs and fold_columns are 0 and
 * requests_per_pass is the existing kernel's 8. */
int he_simple_pir_batch_response_plan(uint32_t plaintext_bits, uint32_t ciphertext_bits, uint32_t word_bits,
                                      size_t database_columns, size_t query_count,
                                      uint32_t* out_matrix_path,       /* 1: int8 matrix kernel, 0: the existing reply kernel */
                                      uint32_t* out_database_limbs,    /* 1 (plaintext_bits <= 7) or 2 (9 .. 14) */
                                      uint32_t* out_request_limbs,     /* ceil(ciphertext_bits / 7) = shift classes kept */
                                      uint32_t* out_requests_per_pass, /* requests answered by one read of the database */
                                      size_t* out_fold_columns,        /* columns after which the i32 accumulators are folded */
                                      size_t* out_workspace_bytes);    /* scratch from the stream-ordered cache: 0 */

/* ---- the SimplePIR client (PrivateInformationRetrieval/SimplePir/SimplePir+Client.swift, SimplePir+Precompute.swift) ----------
 * Batches of `batch` independent precomputed queries on the device, bit for bit the reference's words.  With N the lattice
 * dimension, C = chunks_per_entry, D = database_columns and p the modulus of he_simple_pir_shape:
 *   a_polynomials              [a_poly_count][N] words mod p, Eval form
 *   secrets                    [batch][C][N] Coeff words in {0, 1, p - 1}
 *   queries                    [batch][C][D] words below 2^ciphertext_bits (Requests: C rows per query)
 *   results_without_response   [batch][C][column_size] words mod p
 *   responses                  [batch][C][column_size] words: he_simple_pir_compute_response_device of `queries` as batch x C
 *                              stacked requests
 * word_bits (32 / 64) is an argument and must be the context's (HE_ERR_INVALID_ARGUMENT otherwise); there are no _u32 twins.
 * Every random value is a function of a caller-supplied 32-byte seed through NistAes128Ctr(seed:): the library generates no
 * seed, and a seed must never be used twice.  Every call is enqueue-only on `s`.  The workspace is the caller's: DEVICE, 16-byte
 * aligned, at least he_simple_pir_client_workspace_bytes() bytes (NULL or fewer: HE_ERR_INVALID_ARGUMENT); whatever a call
 * leaves there depends on secrets, errors, indices or entries and is set to zero on `s` before the call's work is done, as are
 * the secret codes the hint product holds in LDS.  Written slabs may overlap nothing else (HE_ERR_INVALID_ARGUMENT).  batch 0: a
 * no-op returning HE_OK after the argument checks that need no buffer.  HE_ERR_DEVICE: no device, or another device current.
 * Known limitation, as for the encryption entries: the AES behind the stream is a T-table implementation in LDS; its timing
 * depends on the bank pattern of data-dependent lookups, i.e. it is not constant-time, and secret seeds pass through it.
 * Not here: DefaultQueryGenerator's queue and actor, seed generation, protobuf Requests / Responses.  (DatabaseMap sharding: the
 * section after this one.) */
#define HE_SIMPLE_PIR_ERROR_STDDEV32 0 /* ErrorStdDev.stdDev32: sigma 3.2, k = 21 trial bits a side, 16 stream bytes a coefficient */
#define HE_SIMPLE_PIR_ERROR_STDDEV64 1 /* ErrorStdDev.stdDev64: sigma 6.4, k = 82, 32 stream bytes, mask 2^18 - 1 on words 1 and 3 */
/* What the client entries do for a shape (the first six arguments are he_simple_pir_shape's, with its errors) and a batch.  Host
 * only: callable without a GPU.  Any out pointer may be NULL.  HE_ERR_INVALID_ARGUMENT also for an unknown error_std_dev and a
 * batch above 2^20.
 *   out_chunk_size               SimplePirParameters.chunkSize = ceil(entry_size_in_scalar / C)
 *   out_query_words              C D: words of one precomputed query      out_result_words   C column_size
 *   out_error_stream_bytes       stream bytes per error coefficient: 16 or 32 (a query's error is ONE generator over C D
 *                                coefficients, drawn in 4096-byte refills)
 *   out_secret_rows_per_pass     secret rows answered per read of the hint by the hint product (16: one 64-bit accumulator
 *                                per row and lane)
 *   out_fold_terms               terms of at most p a 64-bit accumulator of the hint product holds before it is folded to
 *                                below p: floor((2^64 - 1) / p)
 *   out_row_block                secret rows encrypt_zero stages at a time (its staged sample stays near 128 MiB);
 *                                HEAMD_SIMPLE_PIR_CLIENT_ROW_BLOCK=<rows> lowers it and never raises it
 *   out_hint_product_lds_bytes   LDS of a workgroup of the hint product: the codes of a slab of 1024 columns and the sums
 *   out_*_workspace_bytes        he_simple_pir_client_workspace_bytes of each entry for `batch` (secret x hint: batch x C rows) */
int he_simple_pir_client_plan(uint32_t plaintext_bits, uint32_t ciphertext_bits, uint32_t lattice_dimension, uint32_t word_bits,
                              size_t entry_count, size_t entry_size_in_bytes, int error_std_dev, size_t batch,
                              size_t* out_chunk_size, size_t* out_query_words, size_t* out_result_words,
                              uint32_t* out_error_stream_bytes, uint32_t* out_secret_rows_per_pass, uint64_t* out_fold_terms,
                              size_t* out_row_block, size_t* out_hint_product_lds_bytes,
                              size_t* out_a_polynomials_workspace_bytes, size_t* out_encrypt_zero_workspace_bytes,
                              size_t* out_secret_times_hint_workspace_bytes, size_t* out_precompute_workspace_bytes,
                              size_t* out_decrypt_responses_workspace_bytes);
#define HE_SIMPLE_PIR_CLIENT_OP_A_POLYNOMIALS 0
#define HE_SIMPLE_PIR_CLIENT_OP_ENCRYPT_ZERO 1
#define HE_SIMPLE_PIR_CLIENT_OP_SECRET_TIMES_HINT 2 /* count: secret rows */
#define HE_SIMPLE_PIR_CLIENT_OP_PRECOMPUTE 3
#define HE_SIMPLE_PIR_CLIENT_OP_DECRYPT_RESPONSES 4
/* Workspace bytes of a client entry for `count` queries (secret rows for SECRET_TIMES_HINT), a multiple of 16; 0 for a NULL
 * context, an unknown operation, an unknown standard deviation (only ENCRYPT_ZERO and PRECOMPUTE depend on it; every operation
 * but SECRET_TIMES_HINT checks it) and a count above 2^20.  add_indices takes no workspace. */
size_t he_simple_pir_client_workspace_bytes(const he_simple_pir_context* ctx, int operation, int error_std_dev, size_t count);
/* generateAPolynomials (SimplePir+Database.swift:178-181) and convertToEvalFormat, as DefaultQueryGenerator.init caches them
 * (SimplePir+Precompute.swift:331): a_poly_count polynomials from ONE NistAes128Ctr(seed), the sampler process uses, without its
 * Galois map.  Once per database; every precompute call reads the result.
 *   seed  DEVICE [32], the database's seed      out  DEVICE [a_poly_count][N] words mod p, Eval form */
int he_simple_pir_a_polynomials_device(const he_simple_pir_context* ctx, uint32_t word_bits, const uint8_t* seed, void* out,
                                       void* workspace, size_t workspace_bytes, he_stream s);
/* SimplePirContext.encryptZero (SimplePir+Client.swift:59-82) for `batch` queries: noiselessSample (:29-50) -- the forward NTT
 * of the secrets, a_k s for every k through the inverse NTT, concatenated and cut to D --, then in one kernel
 * Array2d.divideAndRound(initialMod: p, newMod: 2^c) (Array2d.swift:489-514), the error of
 * Array2d.randomCenteredBinomialDistribution(standardDeviation:mod: [2^c]) (:382-429) and the mask.  The error of query b is ONE
 * generator NistAes128Ctr(error_seeds[b]) over C D coefficients; row q of the query takes coefficients q D ... (the reference
 * reshapes a 1 x n array).  The error never reaches memory; the un-noised sample is staged in the workspace row_block secret
 * rows at a time and zeroed.
 *   a_polynomials  DEVICE, he_simple_pir_a_polynomials_device's      secrets      DEVICE [batch][C][N]
 *   error_seeds    DEVICE [batch][32]                                queries      DEVICE [batch][C][D], written whole */
int he_simple_pir_encrypt_zero_device(const he_simple_pir_context* ctx, uint32_t word_bits, int error_std_dev,
                                      const void* a_polynomials, const void* secrets, const uint8_t* error_seeds, void* queries,
                                      size_t batch, void* workspace, size_t workspace_bytes, he_stream s);
/* secretMatrix.multiply(transposing: hint, modulus: p) (Array2d.multiply(transposing:modulus:), SimplePir+Precompute.swift:
 * 122-188) for `rows` secret rows: results[r][j] = sum_n secrets[r][n] hint[j][n] mod p.
 *   secrets  DEVICE [rows][N]      hint  DEVICE [column_size][N] as he_simple_pir_process_database_device writes it, 16-byte
 *   aligned (HE_ERR_INVALID_ARGUMENT otherwise)      results  DEVICE [rows][column_size]
 * column_size is an argument (any number of hint rows over the context's ring; the precompute entry passes the shape's).
 * PRECONDITION: every secret word is 0, 1 or p - 1 -- any other word counts as 0 (the kernel adds hint words, it does not
 * multiply; the reference's product takes any matrix).  The secrets are packed to 2-bit codes in the workspace; a workgroup
 * reads a tile of 64 hint rows once per pass of 16 secret rows, 16 bytes per lane. */
int he_simple_pir_secret_times_hint_device(const he_simple_pir_context* ctx, uint32_t word_bits, const void* secrets, size_t rows,
                                           const void* hint, size_t column_size, void* results, void* workspace,
                                           size_t workspace_bytes, he_stream s);
/* PrecomputedQueries.WithoutIndices.init (SimplePir+Precompute.swift:199-227) for `batch` queries: generateSecretPolys
 * (SimplePir+Client.swift:21-27; polynomial (b, q) is randomizeTernary over NistAes128Ctr(secret_seeds[b][q])), then the two
 * entries above on the same secrets, which live in the workspace alone.
 *   secret_seeds  DEVICE [batch][C][32]      error_seeds  DEVICE [batch][32]
 *   queries       DEVICE [batch][C][D]       results_without_response  DEVICE [batch][C][column_size] */
int he_simple_pir_precompute_queries_device(const he_simple_pir_context* ctx, uint32_t word_bits, int error_std_dev,
                                            const void* a_polynomials, const void* hint, const uint8_t* secret_seeds,
                                            const uint8_t* error_seeds, void* queries, void* results_without_response,
                                            size_t batch, void* workspace, size_t workspace_bytes, he_stream s);
/* WithoutIndices.add(index:) (SimplePir+Precompute.swift:241-256) for `batch` queries in place: for q < C,
 * queries[b][q][(q + indices[b] C) / entries_per_column] = (... + 2^(c - plaintext_bits)) & (2^c - 1).
 *   indices  DEVICE [batch] 8-byte words      flags  DEVICE [batch] or NULL: 1 for an index at or above entry_count, whose query
 *   stays untouched (the reference would trap), 0 otherwise */
int he_simple_pir_add_indices_device(const he_simple_pir_context* ctx, uint32_t word_bits, void* queries, const uint64_t* indices,
                                     uint32_t* flags, size_t batch, he_stream s);
/* prepareResponse, integrate and SimplePirClient.decrypt (SimplePir+Precompute.swift:281-311, SimplePir+Client.swift:85-95,
 * 112-121) for `batch` queries: extractEntries of both slabs at the index, ((response - result + (delta >> 1)) & mask) >>
 * (c - plaintext_bits) wrapping in the word, then coefficientsToBytes(bitsPerCoeff: plaintext_bits) cut to
 * entry_size_in_bytes.
 *   entries  DEVICE [batch][entry_size_in_bytes]; all zero for an index at or above entry_count      flags  as above, or NULL */
int he_simple_pir_decrypt_responses_device(const he_simple_pir_context* ctx, uint32_t word_bits, const void* responses,
                                           const void* results_without_response, const uint64_t* indices, uint8_t* entries,
                                           uint32_t* flags, size_t batch, void* workspace, size_t workspace_bytes, he_stream s);

/* ---- SimplePIR over sharded databases (PrivateInformationRetrieval/SimplePir/DatabaseMap.swift, SimplePir+Shards.swift) ------
 * What Sources/SimplePIRProcessDatabase/main.swift runs before SimplePirServer.process, and what SimplePirClientForAllShards
 * does around the per-shard clients.  With S = shard_count, C = chunk_size, len_e the bytes of value e
 * (value_offsets[e + 1] - value_offsets[e]) and order_e its row of shard_orders -- the reference's randomShards, a permutation
 * of 0 .. S - 1 (DatabaseMap.swift:92):
 *   c_e = ceil(len_e / C) chunks; an empty value has none but keeps its entry (size 0, chunks [])
 *   chunk k of entry e lies in shard order_e[k mod S], at index (rows that shard got from entries before e) + floor(k / S)
 *   entry e gives shard s exactly floor(c_e / S) + [order_e^-1(s) < c_e mod S] rows
 * The reference draws order_e from the system generator; this library generates no randomness, so the orders are an input and
 * every result is a function of the arguments.  A flat chunk id counts chunks in entry-then-chunk order: chunk k of entry e is
 * out_chunk_starts[e] + k.  All device entries are enqueue-only on `s`; 8-byte arrays are 8-byte aligned, 4-byte arrays 4-byte
 * aligned (HE_ERR_INVALID_ARGUMENT otherwise), written arrays overlap nothing else (HE_ERR_INVALID_ARGUMENT).  Every store is
 * bounded by the capacities stated here, whatever the device arrays hold.  No _u32 twins: nothing here has a slab word.
 * Reference behaviour kept: ShardMap.shardCount is the number of shards that RECEIVED a chunk, not S (SimplePir+Shards.swift:
 * 31-36), and SimplePirClientForAllShards.init throws when it differs from the client count (:65-69) -- host logic, left to the
 * caller (heamd.SimplePirShardMap / SimplePirClientForAllShards do it).
 * Not here: drawing the orders, the Array2d / SimplePirDatabase files, protobuf SimplePIRConfig and databaseMapping. */
#define HE_SIMPLE_PIR_SHARD_FORM_NONE 0 /* nothing to write */
#define HE_SIMPLE_PIR_SHARD_FORM_BYTE 1 /* a lane writes 1 byte */
#define HE_SIMPLE_PIR_SHARD_FORM_WORD 2 /* 8 bytes: the written slab (and the chunks the assembly reads) on 8-byte boundaries, C a multiple of 8 */
#define HE_SIMPLE_PIR_SHARD_FORM_WIDE 3 /* 16 bytes: the same on 16-byte boundaries, C a multiple of 16 */
/* What DatabaseMap.shardDatabase (DatabaseMap.swift:82-110) does for a database.  Host only: callable without a GPU.
 *   value_offsets  HOST [count + 1]      shards_address  where the slab of he_simple_pir_shard_scatter_device will lie (its low
 *   four bits decide the form; nothing is read there)
 *   out_total_chunks         sum of c_e: rows of all shards, and the capacity of the three chunk arrays below
 *   out_maximum_chunk_count  ShardMap.maximumChunkCount (SimplePir+Shards.swift:37)
 *   out_chunks_per_shard     ceil(maximum_chunk_count / S): ShardMap.chunksPerShard (:39) when every shard received a chunk
 *   out_scatter_form         HE_SIMPLE_PIR_SHARD_FORM_* of the scatter
 *   out_map_tile_entries     entries of one workgroup in the two map passes (128)      out_map_tiles  their workgroups
 *   out_count_workgroups     workgroups of the chunk-count pass
 *   out_scratch_bytes        stream-ordered scratch of the map: O(out_map_tiles x S) and the sums of two scans
 * Any out pointer may be NULL.  HE_ERR_INVALID_ARGUMENT: S outside 1 .. 256, C = 0, count above 2^32 - 2, offsets that
 * decrease, more than 2^32 - 1 chunks. */
int he_simple_pir_shard_plan(const uint64_t* value_offsets, size_t count, size_t shard_count, size_t chunk_size,
                             uint64_t shards_address, uint64_t* out_total_chunks, uint64_t* out_maximum_chunk_count,
                             uint64_t* out_chunks_per_shard, uint32_t* out_scatter_form, uint32_t* out_map_tile_entries,
                             size_t* out_map_tiles, size_t* out_count_workgroups, size_t* out_scratch_bytes);
/* The map of DatabaseMap.shardDatabase (DatabaseMap.swift:90-104: the chunk locations of every entry).  All pointers DEVICE.
 *   value_offsets         [count + 1] 8-byte words      shard_orders  [count][S] bytes
 *   total_chunks          the caller's claim (he_simple_pir_shard_plan's) and the capacity of the three chunk arrays
 *   out_chunk_starts      [count + 1] 8-byte words: the exclusive scan of c_e
 *   out_chunk_shard       [total_chunks] 4-byte words: the shard of each chunk, by flat chunk id (ChunkLocation.shardIndex)
 *   out_chunk_index       [total_chunks] 4-byte words: its index within that shard (ChunkLocation.index)
 *   out_shard_row_starts  [S + 1] 8-byte words: shard s owns rows starts[s] .. starts[s + 1] of the scatter's slab
 *   out_row_chunk         [total_chunks] 4-byte words: the flat chunk id that fills each slab row
 *   device_mismatch       optional, one 4-byte word the caller has zeroed.  Bit 0: a row of shard_orders is no permutation of
 *                         0 .. S - 1 (a value at or above S, or a repeat); that entry is split under the identity order.
 *                         Bit 1: out_chunk_starts[count] != total_chunks; the chunk arrays then hold nothing usable.
 * Nothing is written outside the stated arrays in either case.  Three passes over tiles of 128 entries (chunk counts and their
 * scan; per-tile rows of every shard; their scan by [shard][tile]; the apply pass) -- no workgroup waits for another, and no
 * atomic decides a position.  Scratch from the library's stream-ordered cache. */
int he_simple_pir_shard_map_device(const uint64_t* value_offsets, const uint8_t* shard_orders, size_t count, size_t shard_count,
                                   size_t chunk_size, uint64_t total_chunks, uint64_t* out_chunk_starts, uint32_t* out_chunk_shard,
                                   uint32_t* out_chunk_index, uint64_t* out_shard_row_starts, uint32_t* out_row_chunk,
                                   uint32_t* device_mismatch, he_stream s);
/* The shards of DatabaseMap.shardDatabase (DatabaseMap.swift:93-102, :106-108), back to back.  All pointers DEVICE.
 *   values         value e is values[value_offsets[e] .. value_offsets[e + 1]); any byte address.  Nothing at or above
 *                  values_bytes is read
 *   chunk_starts, row_chunk   the map's out_chunk_starts and out_row_chunk
 *   shards         [total_chunks][C] bytes.  Every byte is written, the zero padding of each entry's last chunk included, and no
 *                  other byte.  shards + out_shard_row_starts[s] * C with starts[s + 1] - starts[s] rows is the `entries`
 *                  argument of he_simple_pir_process_database_device(_u32) for shard s (entry_size_in_bytes = C)
 * A lane owns an aligned piece of the slab (HE_SIMPLE_PIR_SHARD_FORM_*, by the slab's address and C; the plan says which). */
int he_simple_pir_shard_scatter_device(const uint8_t* values, uint64_t values_bytes, const uint64_t* value_offsets, size_t count,
                                       size_t chunk_size, uint64_t total_chunks, const uint64_t* chunk_starts,
                                       const uint32_t* row_chunk, uint8_t* shards, he_stream s);
/* SimplePirClientForAllShards.query(for:) up to add(index:) (SimplePir+Shards.swift:71-87) for `batch` lookups.  All DEVICE.
 *   entry_positions  [batch] 8-byte words: positions in the entry list; at or above count: no such entry (the dictionary from
 *                    originalIndex to position stays on the host)
 *   chunk_starts, chunk_shard, chunk_index   the map's arrays      maximum_chunk_count, chunks_per_shard  ShardMap's
 *   out_indices      [S][batch][chunks_per_shard] 8-byte words: in shard s's plane the indices of the entry's chunks in that shard
 *                    come first, in chunk order, then zeros (the fake queries at index 0).  A plane is the `indices` argument of
 *                    he_simple_pir_add_indices_device with batch x chunks_per_shard queries on shard s's context
 *   out_found        [batch] 4-byte words: 1 for a position below count
 * HE_ERR_INVALID_ARGUMENT also for maximum_chunk_count above total_chunks or chunks_per_shard 0 with maximum_chunk_count > 0.
 * No scratch. */
int he_simple_pir_shard_query_indices_device(const uint64_t* entry_positions, size_t batch, size_t count, size_t shard_count,
                                             uint64_t total_chunks, uint64_t maximum_chunk_count, uint64_t chunks_per_shard,
                                             const uint64_t* chunk_starts, const uint32_t* chunk_shard, const uint32_t* chunk_index,
                                             uint64_t* out_indices, uint32_t* out_found, he_stream s);
/* SimplePirClientForAllShards.decrypt after the per-shard decryptions (SimplePir+Shards.swift:139-171).  All DEVICE.
 *   chunks       [S][batch][chunks_per_shard][C] bytes: what he_simple_pir_decrypt_responses_device wrote, per shard
 *   indices      he_simple_pir_shard_query_indices_device's out_indices      entry_positions  as there
 *   out_entries  [batch][maximum_chunk_count * C] bytes      out_sizes  [batch] 8-byte words      out_found  [batch] 4-byte words
 * Chunk k of an entry comes from the LAST slot of its shard whose index equals the chunk's index, from slot 0 when none does
 * (:159-164) -- so a real chunk at index 0 is read from a trailing fake query.  Bytes at and above the entry's size are zero.
 * An absent entry walks (shard 0, index 0) for all maximum_chunk_count chunks (:147-157) and yields zeros, size 0, found 0: it
 * reads and writes as many bytes as a present one, and the mask comes last.  No scratch. */
int he_simple_pir_shard_assemble_device(const uint8_t* chunks, const uint64_t* indices, const uint64_t* entry_positions, size_t batch,
                                        const uint64_t* value_offsets, size_t count, size_t shard_count, size_t chunk_size,
                                        uint64_t total_chunks, uint64_t maximum_chunk_count, uint64_t chunks_per_shard,
                                        const uint64_t* chunk_starts, const uint32_t* chunk_shard, const uint32_t* chunk_index,
                                        uint8_t* out_entries, uint64_t* out_sizes, uint32_t* out_found, he_stream s);

/* PirUtil.expand(ciphertexts:outputCount:using:) (PrivateInformationRetrieval/IndexPir/PirUtil.swift:196-355):
 * oblivious expansion of `ciphertext_count` query ciphertexts [..][2][L][N] (Coeff, top level) into `output_count`
 * ciphertexts, in the reference's output order.  The evaluation key is given as parallel host arrays:
 * galois_elements[k] and the device pointer galois_keys[k] of that element's key (layout as in
 * he_bfv_apply_galois_device).  Per tree level the largest element <= the target element is applied
 * 2^(log2(target-1) - log2(element-1)) times (PirUtil.swift:217-231); none available -> HE_ERR_MISSING_GALOIS_KEY.
 * The count preconditions of PirUtil.swift:325-326 return HE_ERR_INVALID_ARGUMENT.
 * The recursion is planned on the host once per (ciphertext_count, output_count) and context: the first call of a shape
 * uploads the plan (a blocking copy of a few KB, kept by the context); every later one is enqueue-only. */
int he_pir_expand_device(const he_bfv_context* ctx, const uint64_t* ciphertexts, size_t ciphertext_count,
                         size_t output_count, const uint64_t* galois_elements, const uint64_t* const* galois_keys,
                         size_t galois_key_count, uint64_t* out, he_stream s);
/* `queries` independent expansions of one shape in one call (several clients' queries answered together): every tree
 * level is one batch over all queries, so the first levels -- 1, 2, 4, ... ciphertexts per query -- fill the chip too.
 *   ciphertexts  [queries][ciphertext_count][2][L][N]      out  [queries][output_count][2][L][N]
 *   galois_keys  host array [queries][galois_key_count] of device pointers: query q's key of galois_elements[k] at
 *                [q * galois_key_count + k] (queries of one client repeat the pointer; only the inner product with the
 *                key is launched per run of equal keys)
 * he_pir_expand_device is this call with queries = 1. */
int he_pir_expand_batch_device(const he_bfv_context* ctx, const uint64_t* ciphertexts, size_t queries,
                               size_t ciphertext_count, size_t output_count, const uint64_t* galois_elements,
                               const uint64_t* const* galois_keys, size_t galois_key_count, uint64_t* out, he_stream s);

/* =====================================================================================================
 * Device groups: the path's multi-GPU split in one process
 * =====================================================================================================
 * Every unit of the path -- a polynomial of a batch (Bfv.swift:266-287), a database column of a PIR chunk
 * (PirUtil.swift:424-445) -- is independent; the reference spreads them over the tasks of one process.  A device group spreads
 * them over GPUs: one he_bfv_context and one stream per member device (contexts replicated, a few MiB of tables each), `total`
 * units split by he_shard_bounds -- member m owns [begin, end), the first total % members members one unit more -- and nothing
 * on the data path crossing devices: the query is copied to the members on the way in, the finished shards to the home
 * device (member 0's) on the way out, as peer copies on the members' streams joined into the caller's stream by events.
 * A device may be listed more than once (two shards on one GPU).  HE_GROUP_STAGE_ALL makes every member but the first go
 * through the copies of a remote device even when it is the same GPU -- the whole exchange on a one-GPU box (tests).
 * Group calls are enqueue-only; `home_stream` is a stream of member 0's device (NULL: its default stream), pointers
 * marked "home" live there, shard m lives on member m's device. */
typedef struct he_device_group he_device_group;
#define HE_GROUP_STAGE_ALL 1u
int he_shard_bounds(size_t total, uint32_t members, uint32_t member, size_t* out_begin, size_t* out_end);
int he_device_group_create(const int* devices, uint32_t device_count, uint32_t flags, uint32_t degree,
                           uint64_t plaintext_modulus, const uint64_t* coefficient_moduli, uint32_t moduli_count,
                           he_device_group** out);
void he_device_group_destroy(he_device_group* group);
uint32_t he_device_group_size(const he_device_group* group);
int he_device_group_device(const he_device_group* group, uint32_t member, int* out_device);
const he_bfv_context* he_device_group_context(const he_device_group* group, uint32_t member); /* owned by the group */
he_stream he_device_group_stream(const he_device_group* group, uint32_t member);              /* owned by the group */
int he_device_group_synchronize(he_device_group* group); /* blocks until every member's stream has drained */
/* PolyContext.forwardNtt / inverseNtt over a batch that lives sharded: member m transforms
 * slab_shards[m] = [its share of batch][moduli_count][N] in place on its own stream; nothing moves between devices. */
int he_ntt_forward_group(he_device_group* group, uint32_t moduli_count, uint64_t* const* slab_shards, size_t batch);
int he_ntt_inverse_group(he_device_group* group, uint32_t moduli_count, uint64_t* const* slab_shards, size_t batch);
/* he_pir_dim0_columns_device over a database sharded by column (BASELINE configs[4]): database_shards[m] =
 * [its share of columns][d0][L][N] Eval (present_shards[m] its mask or NULL; present_shards itself may be NULL);
 * dim0_query_eval (home) is replicated to the members; out (home) [columns][2][L][N] Coeff receives every member's columns
 * at their place.  Whole columns stay on one device, so there is no reduction, only this gather. */
int he_pir_dim0_columns_group(he_device_group* group, const uint64_t* dim0_query_eval, size_t d0,
                              const uint64_t* const* database_shards, const uint8_t* const* present_shards, size_t columns,
                              uint64_t* out, he_stream home_stream);
/* computeResponseForOneChunk over the group (chunk_count = 1): he_pir_dim0_columns_group, then the remaining dimensions on the
 * home device (they need every column).  remaining_query, relinearization_key, out: home. */
/* The chunk loop of PirUtil.computeResponse (PirUtil.swift:533-563) over the group: the columns of all `chunk_count` chunks are
 * one column range, sharded as above (database_shards[m] = member m's share of chunk_count x columns columns); one dim-0 pass
 * per member, the gather, then the remaining dimensions of all chunks on the home device.  out (home) [chunk_count][2][1][N].
 * Where he_shard_bounds falls on chunk boundaries for every member (chunk_count a multiple of the group's size) each member
 * answers its chunks from start to finish instead -- he_pir_compute_response_device on its own stream, the queries and the key
 * replicated to it -- and only the finished responses come back: no part of the call is left to one device alone. */
int he_pir_compute_response_group(he_device_group* group, const uint32_t* dimensions, uint32_t dimension_count,
                                  const uint64_t* dim0_query_eval, const uint64_t* remaining_query,
                                  size_t remaining_query_count, const uint64_t* const* database_shards,
                                  const uint8_t* const* present_shards, size_t chunk_count,
                                  const uint64_t* relinearization_key, uint64_t* out, he_stream home_stream);
int he_pir_compute_response_chunk_group(he_device_group* group, const uint32_t* dimensions, uint32_t dimension_count,
                                        const uint64_t* dim0_query_eval, const uint64_t* remaining_query,
                                        size_t remaining_query_count, const uint64_t* const* database_shards,
                                        const uint8_t* const* present_shards, const uint64_t* relinearization_key,
                                        uint64_t* out, he_stream home_stream);

/* =====================================================================================================
 * Diagnostics and test hooks (not part of the reference's surface)
 * =================================================================================================== */

/* Builds the host-side precomputation only (no device upload): lets the setup math (roots, twiddle order, Barrett /
 * Shoup constants) be checked where no GPU exists.  Every compute entry point on such a context returns
 * HE_ERR_DEVICE. */
int he_poly_context_create_host_only(uint32_t degree, const uint64_t* moduli, uint32_t moduli_count,
                                     he_poly_context** out);
/* Copies the _NttContext tables of modulus row `rns_index` (PolyRq/PolyRq+Ntt.swift:109-115); any out may be NULL. */
int he_poly_context_copy_ntt_tables(const he_poly_context* ctx, uint32_t rns_index, uint64_t* root_powers,
                                    uint64_t* root_factors, uint64_t* inverse_root_powers,
                                    uint64_t* inverse_root_factors, uint64_t* inverse_degree,
                                    uint64_t* inverse_degree_root);
/* A streaming copy of `words` 8-byte words, 8 bytes per lane -- the access width of the transforms' row loads and stores;
 * non_temporal != 0 also takes their cache policy.  What bench.py reports as the attainable rate next to the nominal
 * 8 TB/s (`roofline.copy_rate`: the faster of the two policies). */
int he_words_copy_device(const uint64_t* device_in, uint64_t* device_out, size_t words, int non_temporal, he_stream s);
/* NTT with a named kernel schedule -- every accepted variant computes the same canonical transform (parity tests
 * pin each schedule against the oracle): 0 = auto (production), 1 = exact-quotient butterflies, 2 = generic radix-2
 * kernel, 3 = 16 words per lane, 10 = [0, 8p) butterflies.  Anything else:
 * HE_ERR_INVALID_ARGUMENT. */
int he_ntt_device_variant(const he_poly_context* ctx, uint64_t* device_slab, size_t batch, int inverse, int variant,
                          he_stream stream);
/* Same host-only construction for the BFV context; he_bfv_copy_bsk_moduli returns the L+1 Bsk primes
 * (RnsTool.swift:28-33). */
int he_bfv_context_create_host_only(uint32_t degree, uint64_t plaintext_modulus, const uint64_t* coefficient_moduli,
                                    uint32_t moduli_count, he_bfv_context** out);
/* The same for Context<Bfv<UInt32>> (he_bfv_context_create_u32's checks and constants, nothing uploaded). */
int he_bfv_context_create_u32_host_only(uint32_t degree, uint64_t plaintext_modulus, const uint64_t* coefficient_moduli,
                                        uint32_t moduli_count, he_bfv_context** out);
int he_bfv_copy_bsk_moduli(const he_bfv_context* ctx, uint64_t* out_bsk);

#ifdef __cplusplus
}
#endif
#endif /* HE_AMD_H */
