// kernels.hpp -- host-callable launchers of the HIP kernels (all asynchronous on `stream`).  A kernel family that exists on
// both slab words has ONE launcher name, overloaded on the slab pointer: uint64_t slabs take a DeviceContext, uint32_t slabs
// (PolyRq<UInt32>, every modulus <= 2^30 - 1) a DeviceContext32 -- word_layer.hpp word_image<W> yields either.  Both overloads
// of a family are defined by the family's unit(s), named at the head of each block below; the transforms' 4-byte overloads by
// ntt_word32.hip.  Where the 8-byte kernel has something the 4-byte one lacks, the 4-byte overload returns
// hipErrorNotSupported before any launch: the signal every caller already falls back on.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "device_context.hpp"

namespace heamd {

// ---- the transforms -- 8-byte slabs: ntt_routing.hip (launchers; the kernels are in the other ntt_*.hip units); 4-byte
// slabs: ntt_word32.hip (kernels and launchers) -----------------------------------------------------------------------------
// kernel schedule for launch_ntt (tests pin each against the oracle; production callers pass kNttVariantAuto).  Every
// variant computes the same canonical transform.
enum {
    kNttVariantAuto = 0,     // tiled kernel, 8 words per lane where a workgroup of <= 1024 lanes allows it
    kNttVariantExact = 1,    // same kernel, exact-quotient butterflies (what moduli >= 2^61 get)
    kNttVariantGeneric = 2,  // radix-2 stage loop (what degrees without a tiled kernel get)
    kNttVariantWide = 3,     // tiled kernel, 16 words per lane
    kNttVariantApprox = 10   // production kernel pinned to the [0, 8p) butterflies (what 56..61-bit moduli get)
};

// NTT of `rows` contiguous length-N rows.  Row r uses modulus index mod_base + (r % mod_period).
hipError_t launch_ntt(bool inverse, uint64_t* slab, const DeviceContext& ctx, uint32_t mod_base, uint32_t mod_period,
                      size_t rows, hipStream_t stream, int force_variant = kNttVariantAuto);
// (4-byte words hold a row in the LDS: hipErrorNotSupported above N = 32768)
hipError_t launch_ntt(bool inverse, uint32_t* slab, const DeviceContext32& ctx, uint32_t mod_base, uint32_t mod_period,
                      size_t rows, hipStream_t stream);
// Inverse NTT out of place: rows read from `source`, written to the same places of `slab` (N = 4096 / 8192 with every modulus
// below 2^61; hipErrorNotSupported, nothing launched, elsewhere)
hipError_t launch_ntt_inverse_out_of_place(const uint64_t* source, uint64_t* slab, const DeviceContext& ctx, uint32_t mod_base,
                                           uint32_t mod_period, size_t rows, hipStream_t stream);
// Key-switching decomposition fused into the forward NTT (Bfv+Keys.swift:165-179): spread [polys][L][L+1][N] row
// (poly, j, r) = NTT_{ks modulus r}( source row j of polynomial `poly`, reduced mod r when q_j > modulus r ), read
// from source + poly * poly_stride + j * N.  galois_inverse = g^-1 mod 2N: the source polynomial is first taken through
// f(x) -> f(x^g) (Coeff form, PolyRq/Galois.swift:115-143) as its rows are loaded; 0: as it is.
// hipErrorNotSupported for degrees without a tiled kernel (the caller then runs launch_key_switch_spread + launch_ntt),
// and on 4-byte words for galois_inverse != 0.
hipError_t launch_ntt_spread(const uint64_t* source, size_t poly_stride, uint32_t source_moduli, size_t polys,
                             uint64_t* spread, const DeviceContext& ks_ctx, uint32_t galois_inverse, hipStream_t stream);
hipError_t launch_ntt_spread(const uint32_t* source, size_t poly_stride, uint32_t source_moduli, size_t polys,
                             uint32_t* spread, const DeviceContext32& ks_ctx, uint32_t galois_inverse, hipStream_t stream);
// Plaintext.convertToEvalFormat fused into the forward NTT (Plaintext.swift:149-170): out [polys][L][N] row (poly, r)
// = NTT_{q_r}(centred lift of plaintexts[poly][N] mod q_r).  hipErrorNotSupported for degrees without a tiled kernel.
hipError_t launch_ntt_lift(const uint64_t* plaintexts, uint64_t plaintext_modulus, size_t polys, uint64_t* out,
                           const DeviceContext& ctx, hipStream_t stream);
// NTT of `records` records of `record_rows` rows each (row r uses modulus r), the leading ctx.headroom_prefix rows on
// the fold-free butterflies and the rest on the [0, 8p) ones (the [Q, Bsk] slabs of BEHZ multiplication)
hipError_t launch_ntt_mixed(bool inverse, uint64_t* slab, const DeviceContext& ctx, uint32_t record_rows, size_t records,
                            hipStream_t stream);
// The rows [first, first + count) of every record only; hipErrorNotSupported (nothing launched) for degrees without a tiled kernel.
hipError_t launch_ntt_record_band(bool inverse, uint64_t* slab, const DeviceContext& ctx, uint32_t record_rows, uint32_t first,
                                  uint32_t count, size_t records, hipStream_t stream);
// Forward NTT of lifted [Q, Bsk] records [records][record_rows][N] whose first source_moduli rows were left unwritten by
// the lift: they are read from the source polynomials -- record = item * 4 + slot from polynomial slot & 1 of item
// `item` of `base` (slots 0, 1) or `second` (slots 2, 3), items `stride` words apart; second == nullptr: record r from
// base + r * stride (8-byte words only).  hipErrorNotSupported (ntt_lifted_forward_supported false): lift with the copy,
// then launch_ntt_mixed / launch_ntt.
bool ntt_lifted_forward_supported(const DeviceContext& ctx, uint32_t record_rows, uint32_t source_moduli, size_t records);
bool ntt_lifted_forward_supported(const DeviceContext32& ctx, uint32_t record_rows, uint32_t source_moduli, size_t records);
hipError_t launch_ntt_lifted_forward(uint64_t* slab, const DeviceContext& ctx, uint32_t record_rows, size_t records,
                                     const uint64_t* base, const uint64_t* second, size_t stride, uint32_t source_moduli,
                                     hipStream_t stream);
hipError_t launch_ntt_lifted_forward(uint32_t* slab, const DeviceContext32& ctx, uint32_t record_rows, size_t records,
                                     const uint32_t* base, const uint32_t* second, size_t stride, uint32_t source_moduli,
                                     hipStream_t stream);
// Bfv+Multiply.swift:80-82 into the inverse transform's load: lifted [items][4][record_rows][N] (Eval) -> out
// [items][3][record_rows][N] (Coeff; the context carries t N^-1).  hipErrorNotSupported for degrees without a tiled kernel.
hipError_t launch_ntt_tensor_inverse(const uint64_t* lifted, uint64_t* out, const DeviceContext& ctx, uint32_t record_rows,
                                     size_t items, hipStream_t stream);
hipError_t launch_ntt_tensor_inverse(const uint32_t* lifted, uint32_t* out, const DeviceContext32& ctx, uint32_t record_rows,
                                     size_t items, hipStream_t stream);
// Bfv+Keys.swift:180-207 into the inverse transform's load: spread [polys][L][L+1][N], key [L][2][top_rows][N] -> out
// [polys][2][L+1][N] (Coeff).  hipErrorNotSupported for degrees without a tiled kernel (4-byte words: and for L > 15).
hipError_t launch_ntt_key_mac_inverse(const uint64_t* spread, const uint64_t* key, uint64_t* out, const DeviceContext& ks,
                                      uint32_t L, uint32_t top_rows, size_t polys, hipStream_t stream);
hipError_t launch_ntt_key_mac_inverse(const uint32_t* spread, const uint32_t* key, uint32_t* out, const DeviceContext32& ks,
                                      uint32_t L, uint32_t top_rows, size_t polys, hipStream_t stream);
// launch_ntt_key_mac_inverse with the key switch's last step (drop the special modulus, add the update to the first
// `added_polys` polynomials of the ciphertext at ct_base + polynomial * ct_stride) applied as the rows are stored:
// out [polys][2][L][N]; of `prod` ([polys][2][L+1][N]) only the q_ks rows are written.  hipErrorNotSupported (nothing
// launched, ntt_key_mac_finish_supported false): launch_ntt_key_mac_inverse + launch_key_switch_finish.
// KeySwitchEnd says which end: relinearize (the update added to the first `added_polys` polynomials), the Galois key switch
// (galois_inverse = g^-1 mod 2N: ct_base holds the ciphertexts BEFORE the automorphism, c0 is read through it), or one step
// of PirUtil.expand on top of that (expand_shift != 0: out takes the two children of every polynomial; own_base: the
// ciphertexts the children are formed with, nullptr = ct_base; targets_*: rns_kernels.hpp ExpandTargets).  poly_base: the
// launch's first polynomial in ct_base / own_base / out (spread, key and prod are passed from a run's own start).
// 4-byte words have the relinearize end only: any other field off its default is hipErrorNotSupported.
template <typename W>
struct KeySwitchEnd {
    const W* ct_base;
    size_t ct_stride;
    W* out;
    uint32_t added_polys;
    uint32_t galois_inverse = 0, expand_shift = 0;
    const W* own_base = nullptr;
    const uint32_t* targets_table = nullptr;
    size_t targets_group_size = 1, targets_group_stride = 0;
    size_t poly_base = 0;
};
bool ntt_key_mac_finish_supported(const DeviceContext& ks, uint32_t L, size_t polys);
bool ntt_key_mac_finish_supported(const DeviceContext32& ks, uint32_t L, size_t polys);
hipError_t launch_ntt_key_mac_inverse_finish(const uint64_t* spread, const uint64_t* key, uint64_t* prod,
                                             const KeySwitchEnd<uint64_t>& end, const DeviceContext& ks, uint32_t L,
                                             uint32_t top_rows, size_t polys, hipStream_t stream);
hipError_t launch_ntt_key_mac_inverse_finish(const uint32_t* spread, const uint32_t* key, uint32_t* prod,
                                             const KeySwitchEnd<uint32_t>& end, const DeviceContext32& ks, uint32_t L,
                                             uint32_t top_rows, size_t polys, hipStream_t stream);
const char* ntt_variant_name(uint32_t log_degree);

// ---- behz_kernels.hip -- BEHZ multiplication row by row (Bfv+Multiply.swift:18-85): per (item, [Q, Bsk] row) the four forward
// transforms, the tensor product and the three inverse transforms scaled by t in one workgroup, the transformed rows never
// leaving its registers.  lhs, rhs: [items][2][source_moduli][N] Coeff, items ct_stride words apart (their rows are the Q
// rows of the lifted polynomials); lifted: [items][4][record_rows][N] with the Bsk rows written by the lift (the Q rows are
// not read); scaled_qbsk: the [Q, Bsk] context with t N^-1 as inverse-degree constants; out: [items][3][record_rows][N]
// Coeff, what launch_floor_qbsk_to_q takes.  hipErrorNotSupported (nothing launched, behz_rows_fused_supported false):
// launch_ntt_lifted_forward + launch_ntt_tensor_inverse.
bool behz_rows_fused_supported(const DeviceContext& qbsk, uint32_t record_rows, uint32_t source_moduli, size_t items);
// whether the row bands that read the lift's rows take them in [0, 5p) (every such row on the fold butterflies of the plus form,
// whose first stage wants x < 8p and any y): the lift may then skip its three conditional subtracts per word
bool behz_lifted_rows_may_be_lazy(const DeviceContext& scaled_qbsk, uint32_t record_rows, uint32_t source_moduli);
constexpr int kBehzAllRows = 0, kBehzCiphertextRows = 1, kBehzLiftedRows = 2;
hipError_t launch_behz_rows_fused(const uint64_t* lhs, const uint64_t* rhs, size_t ct_stride, const uint64_t* lifted,
                                  uint64_t* out, const DeviceContext& scaled_qbsk, uint32_t record_rows, uint32_t source_moduli,
                                  size_t items, hipStream_t stream, int part = kBehzAllRows);

// ---- poly_kernels.hip: element-wise operations, modulus switching and lazy inner products, on both slab words ---------------
enum class ElementwiseOp : int { Add = 0, Sub = 1, Neg = 2, Mul = 3, MulScalar = 4 };
// lhs[k] = op(lhs[k], rhs[k]) over `rows` rows of [..][L][N]; rhs may be NULL for Neg and MulScalar.  MulScalar reads
// `scalars`, a device array of L (scalar, 64-bit Shoup factor) pairs, and nothing else does.
hipError_t launch_elementwise(ElementwiseOp op, uint64_t* lhs, const uint64_t* rhs, const uint64_t* scalars,
                              const DeviceContext& ctx, size_t rows, hipStream_t stream);
hipError_t launch_elementwise(ElementwiseOp op, uint32_t* lhs, const uint32_t* rhs, const uint64_t* scalars,
                              const DeviceContext32& ctx, size_t rows, hipStream_t stream);
// ct [batch][polys][L][N] *= pt [batch][L][N] (either word under the 8-byte image)
hipError_t launch_mul_plain(uint64_t* ct, const uint64_t* pt, const DeviceContext& ctx, uint32_t poly_count,
                            size_t batch, hipStream_t stream);
hipError_t launch_mul_plain(uint32_t* ct, const uint32_t* pt, const DeviceContext& ctx, uint32_t poly_count, size_t batch,
                            hipStream_t stream);
// divideAndRoundQLast with the first `moduli_count` moduli of ctx: in [polys][L][N] -> out [polys][L-1][N]
hipError_t launch_divide_and_round_q_last(const uint64_t* in, uint64_t* out, const DeviceContext& ctx,
                                          uint32_t moduli_count, size_t polys, hipStream_t stream);
hipError_t launch_divide_and_round_q_last(const uint32_t* in, uint32_t* out, const DeviceContext32& ctx,
                                          uint32_t moduli_count, size_t polys, hipStream_t stream);
// Ciphertext.modSwitchDownToSingle: in [polys][moduli_count][N] -> out [polys][1][N], the moduli_count - 1 steps of
// divideAndRoundQLast in one kernel (2..8 moduli; hipErrorNotSupported otherwise: chain the kernel above).
hipError_t launch_mod_switch_down_to_single(const uint64_t* in, uint64_t* out, const DeviceContext& ctx,
                                            uint32_t moduli_count, size_t polys, hipStream_t stream);
hipError_t launch_adding_lazy_product(const uint64_t* lhs, const uint64_t* rhs, uint64_t* acc_lo_hi,
                                      const DeviceContext& ctx, hipStream_t stream);
hipError_t launch_reduce_accumulator(const uint64_t* acc_lo_hi, uint64_t* out, const DeviceContext& ctx,
                                     hipStream_t stream);
// out[col][poly][L][N] = sum_k cts[k][poly][L][N] * pts[col][k][L][N]  (skip where present[col*count+k] == 0).
// max_lazy: the reference's reduction cadence (used as is by the 128-bit accumulator kernel for degree < 256);
// cadence: products between reductions of the carry-counting accumulator: <= max_lazy and sums below 2^127
// (0 = use the 128-bit kernel).  narrow_moduli: every modulus of ctx is below 2^56 (canonical operands then let the
// accumulator drop two of its three carry counts; the cadence is cut to kNarrowProductSumCadence).
// (W: uint64_t or uint32_t slabs)
template <typename W>
hipError_t launch_inner_product_plain(const W* cts, const W* pts, const uint8_t* present_device, W* out,
                                      const DeviceContext& ctx, uint32_t poly_count, size_t count, size_t columns,
                                      uint64_t max_lazy, uint64_t cadence, bool narrow_moduli, hipStream_t stream);

// ---- packed residue rows: the resident PIR database without the zero top bits of its words -------------------------
// A library-private layout (nothing in the reference's wire format): row r of a polynomial is a little-endian bit
// stream of N fields of width[r] = bits(q_r) bits -- coefficient i occupies stream bits [i width, (i + 1) width), stream
// word j is bits [64 j, 64 j + 64) -- and starts at 8-byte word word_offset[r] of the polynomial (degree a multiple of
// 64: whole words).  A 55-bit modulus stores 6.875 bytes per word instead of 8.
constexpr uint32_t kMaxPackedRows = 8;
struct PackedLayout {
    uint32_t rows;
    uint32_t width[kMaxPackedRows];
    uint32_t word_offset[kMaxPackedRows + 1];  // [rows] = 8-byte words per packed polynomial
};
// slab [polys][rows][N] -> packed [polys][word_offset[rows]] words (galois_kernels.hip)
hipError_t launch_pack_rows(const uint64_t* slab, uint64_t* packed, const PackedLayout& layout, uint32_t log_degree,
                            size_t polys, hipStream_t stream);
// launch_inner_product_plain with the plaintexts packed: pts [columns][count][word_offset[rows]] words.  poly_count 1..3,
// degree >= 256 (poly_kernels.hip).
hipError_t launch_inner_product_plain_packed(const uint64_t* cts, const uint64_t* packed_pts, const PackedLayout& layout,
                                             const uint8_t* present_device, uint64_t* out, const DeviceContext& ctx,
                                             uint32_t poly_count, size_t count, size_t columns, uint64_t cadence,
                                             bool narrow_moduli, hipStream_t stream);

// ---- copy_kernels.hip: the bridge between the two slab words, and the copies of 8-byte words ---------------------------------
// packed [UInt32] words <-> the zero-extended 8-byte words of the Bfv<UInt32> scheme layer (16-byte aligned slabs)
hipError_t launch_widen_words(const uint32_t* in, uint64_t* out, size_t words, hipStream_t stream);
hipError_t launch_narrow_words(const uint64_t* in, uint32_t* out, size_t words, hipStream_t stream);
// every word read once and written once, 8 bytes per lane: the reference point of the transforms' roofline figures
hipError_t launch_stream_copy(const uint64_t* in, uint64_t* out, size_t words, bool non_temporal, hipStream_t stream);
// `records` runs of record_words words from runs src_stride words apart to runs dst_stride apart (record_words a multiple of 2048,
// 16-byte aligned slabs, even strides; hipErrorInvalidValue otherwise)
hipError_t launch_copy_records(const uint64_t* in, size_t src_stride, uint64_t* out, size_t dst_stride, size_t record_words,
                               size_t records, hipStream_t stream);

// ---- seeded_kernels.hip: out[b] = PolyRq.random(context, NistAes128Ctr(seed: seeds[b])), seeds [batch][32] bytes
// scratch: seeded_uniform_scratch_bytes(ctx, batch) bytes (the per-chunk round keys of every seed's re-key chain)
// polynomial b starts at out + b * poly_stride words (W: uint64_t or uint32_t slabs; the reduction is the same, the store narrows)
size_t seeded_uniform_scratch_bytes(const DeviceContext& ctx, size_t batch);
template <typename W>
hipError_t launch_seeded_uniform(const uint8_t* seeds, W* out, size_t poly_stride, const DeviceContext& ctx, size_t batch,
                                 void* scratch, hipStream_t stream);

// ---- galois_kernels.hip: the wire format of a polynomial: per residue row, the serialized bit width and the byte offset of the row
constexpr uint32_t kMaxSerializedRows = 64;
struct SerializeLayout {
    uint32_t rows;
    uint32_t width[kMaxSerializedRows];            // ceilLog2(q_r) - skipLSBs
    uint64_t byte_offset[kMaxSerializedRows + 1];  // prefix sums of ceil(N width / 8); [rows] = bytes per polynomial
};
// (W: uint64_t or uint32_t slabs; 4-byte slabs take the word and byte forms, serialize_form.hpp)
template <typename W>
hipError_t launch_serialize(const W* slab, uint8_t* bytes, const SerializeLayout& layout, uint32_t log_degree,
                            uint32_t skip_lsbs, size_t batch, hipStream_t stream);
template <typename W>
hipError_t launch_deserialize(const uint8_t* bytes, W* slab, const SerializeLayout& layout, uint32_t log_degree,
                              uint32_t skip_lsbs, size_t bytes_per_poly, size_t batch, hipStream_t stream);

// ciphertext_wire_kernels.hip -- whole ciphertexts <-> the reference's wire records in one launch.
// Record i lies at records + i * record_stride and holds `header` bytes (2: the polynomial count as a little-endian UInt16;
// 0: a bare polynomial record) followed by the rows of its `polys` polynomials, each row bit-packed at its own width.
// Its words lie at slab + i * ct_words: [polys][rows][N].
constexpr uint32_t kMaxWirePolys = 3;
constexpr uint32_t kMaxWireRows = kMaxWirePolys * kMaxSerializedRows;
struct CiphertextWireLayout {
    uint32_t polys, rows;                   // rows per polynomial
    uint8_t skip[4];                        // skipLSBs per polynomial
    uint8_t width[kMaxWireRows];            // per (polynomial, row): ceilLog2(q_r) - skip[polynomial]
    uint64_t byte_offset[kMaxWireRows + 1];  // of each (polynomial, row) in the record; [0] = header, [polys rows] = record bytes
};
template <typename W>
hipError_t launch_ciphertexts_serialize(const W* slab, size_t ct_words, uint8_t* records, size_t record_stride,
                                        const CiphertextWireLayout& layout, uint32_t log_degree, size_t count,
                                        hipStream_t stream);
// mismatch (may be nullptr): set to 1 when a record's header differs from layout.polys (layouts with a header only)
template <typename W>
hipError_t launch_ciphertexts_deserialize(const uint8_t* records, size_t record_stride, W* slab, size_t ct_words,
                                          const CiphertextWireLayout& layout, uint32_t log_degree, size_t count,
                                          uint32_t* mismatch, hipStream_t stream);

// pir_database_file_kernels.hip -- the body of a ProcessedDatabase file (IndexPirProtocol.swift:302-378) <-> the database.
// Plaintext p of the range has its tag at records + p + S ranks[p] and, when present[p] != 0, its S = layout.byte_offset[rows]
// payload bytes behind it (layout: one polynomial, no header, skips 0); its words lie at database + p * rows * N.
// ranks [count + 1]: the present plaintexts before p, and their total
hipError_t launch_pir_database_file_ranks(const uint8_t* present, size_t count, uint32_t* ranks, hipStream_t stream);
// every word of the database is written (nil plaintexts: zeros); nothing outside [records, records + records_bytes) is read.
// mismatch (may be nullptr): bit 0 when the range needs more than records_bytes, bit 1 when a tag byte is not what present says
template <typename W>
hipError_t launch_pir_database_file_load(const uint8_t* records, uint64_t records_bytes, const uint8_t* present,
                                         const uint32_t* ranks, size_t count, W* database,
                                         const CiphertextWireLayout& layout, uint32_t log_degree, uint32_t* mismatch,
                                         hipStream_t stream);
// exactly the range's bytes below records_bytes are written, none is read; mismatch bit 0 as above
template <typename W>
hipError_t launch_pir_database_file_save(const W* database, const uint8_t* present, const uint32_t* ranks, size_t count,
                                         uint8_t* records, uint64_t records_bytes, const CiphertextWireLayout& layout,
                                         uint32_t log_degree, uint32_t* mismatch, hipStream_t stream);

// ---- galois_kernels.hip (in and out must not alias) ------------------------------------------------------------
// f(x) -> f(x^g) on Coeff rows; `inverse_element` = g^-1 mod 2N
// (W: uint64_t or uint32_t slabs)
template <typename W>
hipError_t launch_galois_coeff(const W* in, W* out, const DeviceContext& ctx, uint32_t inverse_element, size_t rows,
                               hipStream_t stream);
// f(x) -> f(x^g) on Eval (bit-reversed) rows
hipError_t launch_galois_eval(const uint64_t* in, uint64_t* out, const DeviceContext& ctx, uint32_t element,
                              size_t rows, hipStream_t stream);
// f(x) x^shift mod (x^N + 1), 0 <= shift < 2N
// PirUtil.expand, one level: children of `batch` parents interleaved into next (c1 + parent, (parent - c1) x^-shift')
hipError_t launch_expand_step(const uint64_t* parents, const uint64_t* c1, uint64_t* next, const DeviceContext& ctx,
                              uint32_t shift, size_t batch, hipStream_t stream);
// dst[table[2k+1] >> 1] = src[table[2k]] (doubled mod q when table[2k+1] & 1), whole ciphertexts [2][L][N]
// for `queries` expansions of one shape: query q moves src + q * src_stride -> dst + q * dst_stride (in ciphertexts)
hipError_t launch_expand_move(const uint64_t* src, uint64_t* dst, const uint32_t* table, const DeviceContext& ctx,
                              size_t count, size_t queries, size_t src_stride, size_t dst_stride, hipStream_t stream);
hipError_t launch_multiply_power_of_x(const uint64_t* in, uint64_t* out, const DeviceContext& ctx, uint32_t shift,
                                      size_t rows, hipStream_t stream);
// plaintext [batch][N] mod t -> centered lift into every row of [batch][L][N] (L = ctx.moduli_count)
template <typename W>
hipError_t launch_plaintext_lift(const W* plaintext, W* out, const DeviceContext& ctx, uint64_t t, size_t batch,
                                 hipStream_t stream);
// rows [words] over q0, Coeff form: undo the centered lift in place
template <typename W>
hipError_t launch_plaintext_unlift(W* rows, uint64_t q0, uint64_t t, size_t words, hipStream_t stream);
// residue row 0 of every polynomial: [batch][L][N] -> [batch][N]
template <typename W>
hipError_t launch_first_rows(const W* in, W* out, const DeviceContext& ctx, size_t batch, hipStream_t stream);

// ---- simple_pir_kernels.hip: SimplePirServer (PrivateInformationRetrieval/SimplePir/) -----------------------------------
// The database is [column_size][database_columns] row-major in elements of element_bytes = 1 / 2 / 4 / 8 bytes.
struct SimplePirLayout {
    size_t entry_count, entry_size_in_bytes, entry_size_in_scalar, padded_entry_size, column_size, database_columns;
    uint32_t plaintext_bits, element_bytes;
};
// process, the database half (SimplePir+Database.swift:252-275): entries [entry_count][entry_size_in_bytes] -> database
hipError_t launch_simple_pir_database(const SimplePirLayout& layout, const uint8_t* entries, void* database,
                                      hipStream_t stream);
// rows [first_row, first_row + rows) of the database as `blocks` zero-padded polynomials of N 8-byte coefficients each:
// staging [rows][blocks][N]
hipError_t launch_simple_pir_widen(const void* database, uint32_t element_bytes, size_t columns, size_t first_row, size_t rows,
                                   uint32_t blocks, uint32_t log_degree, uint64_t* staging, hipStream_t stream);
// out [rows][N] = sum_k staging[row][k] * a_eval[k] mod p, Eval form, reduced every `cadence` products (ctx: one modulus)
hipError_t launch_simple_pir_hint_mac(const uint64_t* staging, const uint64_t* a_eval, uint64_t* out, size_t rows,
                                      uint32_t blocks, uint64_t cadence, const DeviceContext& ctx, hipStream_t stream);
// out[0 .. count) = ctx.moduli[0]: the table that lets launch_seeded_uniform draw `count` polynomials from ONE stream
hipError_t launch_simple_pir_replicate_modulus(const DeviceContext& ctx, DeviceModulus* out, uint32_t count,
                                               hipStream_t stream);
// the reference's wide Array2d<Scalar> image <-> the narrow layout (pack keeps the low plaintext_bits of every word)
template <typename W>
hipError_t launch_simple_pir_pack(const W* wide, void* database, uint32_t element_bytes, uint32_t plaintext_bits,
                                  size_t elements, hipStream_t stream);
template <typename W>
hipError_t launch_simple_pir_unpack(const void* database, uint32_t element_bytes, W* wide, size_t elements,
                                    hipStream_t stream);
// computeResponse: responses [query_count][rows] = (database x requests[q]) & (2^ciphertext_bits - 1), requests
// [query_count][columns]
template <typename W>
hipError_t launch_simple_pir_response(const void* database, uint32_t element_bytes, size_t rows, size_t columns,
                                      const W* requests, size_t query_count, W* responses, uint32_t ciphertext_bits,
                                      hipStream_t stream);

// ---- simple_pir_matrix_kernels.hip: computeResponse for large batches on the int8 matrix cores ----------------------------
// The same product for 1-byte elements below 2^7 (database_limbs 1) or 2-byte elements below 2^14 (database_limbs 2), in
// passes of simple_pir_batch::requests_per_pass_of(classes) requests per read of the database.  fold_columns: the cadence at
// which the i32 accumulators are folded into words (0 or anything above the bound: the bound of simple_pir_batch_plan.hpp).
template <typename W>
hipError_t launch_simple_pir_matrix_response(const void* database, uint32_t database_limbs, size_t rows, size_t columns,
                                             const W* requests, size_t query_count, W* responses, uint32_t ciphertext_bits,
                                             size_t fold_columns, hipStream_t stream);

// ---- pnns_kernels.hip: the PNNS server database (PrivateNearestNeighborSearch/) ------------------------------------------
// normalizedScaledAndRounded (Util.swift:74-89), bit-exact: vectors [rows][cols] float32 -> out [rows][cols] int64
hipError_t launch_pnns_quantize_rows(const float* vectors, size_t rows, size_t cols, float scaling_factor, int64_t* out,
                                     hipStream_t stream);
// The diagonal packing of one [rows][cols] matrix (PlaintextMatrix.swift:417-483)
struct PnnsMatrixLayout {
    size_t rows, cols, padded_cols /* nextPowerOfTwo(cols) */, plaintexts_per_column /* ceil(rows / N) */;
    uint64_t plaintext_modulus;
    uint32_t log_degree, baby_step;
    int reduce;  // Modulus.reduce instead of centeredToRemainder
};
// Plaintexts [first, first + count) (index = diagonal * plaintexts_per_column + chunk) as the slabs encodeSimd hands to
// inverseNtt: staging [count][N] words mod t, every word written.  slot_of_word: the inverse of simdEncodingMatrix, [N].
// out_of_range (may be nullptr): set to 1 when reduce == 0 and a value is outside the centred range of t.
template <typename W>
hipError_t launch_pnns_diagonal_pack(const int64_t* values, const uint32_t* slot_of_word, const PnnsMatrixLayout& layout,
                                     size_t first, size_t count, W* staging, uint32_t* out_of_range, hipStream_t stream);

// The inner products of every giant step of PlaintextMatrix.mulTranspose(vector:using:) (MatrixMultiplication.swift:195-212)
// for `queries` (1..pnns_bsgs_queries_per_pass) queries in one pass over the matrix:
//   rot     [baby_step][..][2][L][N] Eval: step j of query q at rot + j * rot_step_words + q * 2 L N
//   matrix  [P * columns][L][N] Eval, plaintext (diagonal d, result c) at d * columns + c; 16-byte aligned
//   out     [giant_step][out_queries][group_columns][2][L][N] Eval, given from the launch's first query (giant-step major: a
//           step of rotateColumnsAndSum then adds one contiguous slab over all queries):
//           out[g][q][c] = sum_{j < min(baby_step, padded_cols - g baby_step)} rot[j][q] * matrix[(g baby_step + j) columns +
//           first_column + c]
// max_lazy / cadence / narrow_moduli: as launch_inner_product_plain.
constexpr size_t kPnnsBsgsTileLimit = size_t(128) << 10;  // LDS bytes of a workgroup's rotated rows (baby_step x queries x 2 KiB)
struct PnnsBsgsLayout {
    size_t rot_step_words;
    uint32_t log_degree, moduli_count, baby_step, giant_step, padded_cols, columns, first_column, group_columns;
    uint32_t out_queries;  // queries of the whole call (>= those of a launch)
    uint64_t max_lazy, cadence;
    bool narrow_moduli;
};
// how many of `queries` one launch takes (the tile must fit LDS; degrees below 64 lanes x 16 bytes: one)
unsigned pnns_bsgs_queries_per_pass(const PnnsBsgsLayout& layout, size_t word_bytes, size_t queries);
template <typename W>
hipError_t launch_pnns_bsgs_inner_product(const W* rot, const W* matrix, W* out, const DeviceContext& ctx,
                                          const PnnsBsgsLayout& layout, unsigned queries, hipStream_t stream);

// ---- pnns_kernels.hip: CiphertextMatrix.extractDenseRow (CiphertextMatrix.swift:252-370) for query matrices of several rows --
// The mask of a row on the SIMD slots: 1 on slot i iff lower <= i < min(N, lower + copies * period) and
// (i - lower) mod period < padded_cols (period a power of two).
struct PnnsRowMask {
    uint32_t lower, period, copies;
};
// The masks as the slabs encodeSimd hands to inverseNtt: staging [count][N] words (0 or 1), every word written.  The patterns
// travel in the kernel arguments, kPnnsRowsPerLaunch rows to a launch.
constexpr unsigned kPnnsRowsPerLaunch = 32;
template <typename W>
hipError_t launch_pnns_row_masks(const uint32_t* slot_of_word, const PnnsRowMask* rows, size_t count, uint32_t padded_cols,
                                 uint32_t log_degree, W* staging, hipStream_t stream);
// ciphertextEval *= plaintextMask (:340-341) for the `count` rows packed in query ciphertext `ciphertext` of every client:
//   queries  [clients][query_ciphertexts][2][L][N] Eval        masks  [..][L][N] Eval, row first_row + i for the i-th row
//   out      ciphertext positions[i] * clients + client is (client, i-th row), Eval
// Each 16 bytes of a query ciphertext are read once for all its rows.  All three 16-byte aligned.
struct PnnsExtractLayout {
    size_t clients, query_ciphertexts;
};
template <typename W>
hipError_t launch_pnns_extract_rows(const W* queries, const W* masks, W* out, const DeviceContext& ctx,
                                    const PnnsExtractLayout& layout, uint32_t ciphertext, uint32_t first_row,
                                    const uint32_t* positions, size_t count, hipStream_t stream);

// ---- pnns_client_kernels.hip: the PNNS client (PrivateNearestNeighborSearch/Client.swift:74-127) ------------------------------
// Context.encodeSimd up to inverseNtt (Encoding.swift:222-231): staging[b][w] = slots[b][slot_of_word[w]], [batch][N] each.
// out_of_range (may be nullptr): set to 1 when a value is not below t.
template <typename W>
hipError_t launch_pnns_simd_scatter(const W* slots, const uint32_t* slot_of_word, uint32_t log_degree, uint64_t t, size_t batch,
                                    W* staging, uint32_t* out_of_range, hipStream_t stream);
// Context.decodeSimd behind forwardNtt (Encoding.swift:242-244): out_slots[b][i] = transformed[b][word_of_slot[i]]
template <typename W>
hipError_t launch_pnns_simd_gather(const W* transformed, const uint32_t* word_of_slot, uint32_t log_degree, size_t batch,
                                   W* out_slots, hipStream_t stream);
// PlaintextMatrix.denseRowPlaintexts (PlaintextMatrix.swift:341-406) up to inverseNtt for all `count` plaintexts of one
// [rows][cols] matrix: staging [count][N] words mod t, every word written; reduce / out_of_range as launch_pnns_diagonal_pack.
struct PnnsDenseRowLayout {
    size_t rows, cols, padded_cols /* nextPowerOfTwo(cols) <= N / 2 */;
    uint64_t plaintext_modulus;
    uint32_t log_degree;
    bool reduce;
};
template <typename W>
hipError_t launch_pnns_dense_row_pack(const int64_t* values, const uint32_t* slot_of_word, const PnnsDenseRowLayout& layout,
                                      size_t count, W* staging, uint32_t* out_of_range, hipStream_t stream);
// PlaintextMatrix.unpackDenseColumn / unpackDenseRow (PlaintextMatrix.swift:515-590) behind forwardNtt: transformed
// [plaintext_count][N] -> out_values [rows][cols] row-major
struct PnnsUnpackLayout {
    size_t rows, cols, padded_cols;
    uint32_t log_degree;
    bool dense_row;
};
template <typename W>
hipError_t launch_pnns_unpack(const W* transformed, const uint32_t* word_of_slot, const PnnsUnpackLayout& layout,
                              uint64_t* out_values, hipStream_t stream);
// The end of Client.decrypt(response:) (Client.swift:104-117) for the dense-column packed distances of a rows x cols result:
// CrtComposer.compose (CrtComposer.swift:76-97) over `count` plaintext moduli, remainderToCentered, the float scaling.
//   transformed  context i's forwardNtt'ed plaintexts [first_plaintext, ..) at transformed + i * context_stride, [..][N]
//   elements     values of the column-major sequence from first_element on: exactly those the plaintexts given hold
//   out          [rows][cols] float32, the whole matrix
constexpr uint32_t kPnnsMaxClientContexts = 8;
struct PnnsComposeLayout {
    size_t rows, cols, first_plaintext, first_element, elements, context_stride;
    uint32_t log_degree;
};
struct PnnsComposeTables {
    uint64_t t[kPnnsMaxClientContexts], inverse[kPnnsMaxClientContexts] /* inversePuncturedProducts */,
        inverse_shoup[kPnnsMaxClientContexts], punctured[kPnnsMaxClientContexts] /* q / t_i */;
    uint64_t q;  // the product of the t_i
    uint32_t count;
};
template <typename W>
hipError_t launch_pnns_compose_distances(const W* transformed, const uint32_t* word_of_slot, const PnnsComposeLayout& layout,
                                         const PnnsComposeTables& tables, float scaling_factor, float* out, hipStream_t stream);

}  // namespace heamd
