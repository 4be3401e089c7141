// pir_database_file.cpp -- ProcessedDatabase.serialize() / init(from:context:) (reference Sources/PrivateInformationRetrieval/
// IndexPir/IndexPirProtocol.swift:248-379): the host walk of a processed-database file and the device entries that turn its
// body into the [count][L][N] Eval database of he_pir_process_database_device and back.
//
//   [version: 1 byte = 1 (:253-255, :305-311)][plaintext count: UInt32 little-endian (:313-315, :367)]
//   per plaintext, in array order: tag 0 (serializedZeroPlaintextTag :258-260) alone, or tag 1 (serializedPlaintextTag :263-265)
//   followed by the S = context.ciphertextContext.serializationByteCount() bytes of Plaintext<Eval>.serialize().poly (:317-328,
//   :369-376)
//
// The position of tag i depends on the tags before it, so the walk is a host step over the bytes the caller has just read from
// disk (he_pir_database_file_scan); it yields the present mask, and with the mask on the device every plaintext's position is
// i + S rank(i): one prefix count, then one load or save launch (pir_database_file_kernels.hip).
#include <string>

#include "api_internal.hpp"
#include "bfv_context.hpp"
#include "kernels.hpp"

using heamd::as_stream;
using heamd::invalid_argument;
using heamd::Scratch;

namespace {

constexpr uint8_t kSerializationVersion = 1;       // IndexPirProtocol.swift:253-255
constexpr uint8_t kSerializedZeroPlaintextTag = 0;  // :258-260
constexpr uint8_t kSerializedPlaintextTag = 1;      // :263-265
constexpr size_t kHeaderBytes = 5;                  // the version byte and the UInt32 plaintext count (:343-344)

// the payload of a present plaintext: a bare PolyRq record over the top-level ciphertext context, skipLSBs 0
int payload_layout(const he_bfv_context* ctx, heamd::CiphertextWireLayout& layout) {
    if (ctx == nullptr) return invalid_argument("null context");
    const he_poly_context* top = he_bfv_ciphertext_context(ctx, he_bfv_ciphertext_moduli_count(ctx));
    if (top == nullptr) return invalid_argument("context without a ciphertext level");
    return heamd::poly_wire_layout(*top->impl, layout);
}

int truncated(const std::string& where, size_t at, size_t byte_count) {
    heamd::set_last_error("invalid argument: the database file ends inside " + where + " (byte " +
                          std::to_string(at) + " of " + std::to_string(byte_count) + ")");
    return HE_ERR_INVALID_ARGUMENT;
}

// the checks both device entries share, in the order the header states; HE_OK with *run = false: nothing to do
template <typename W>
int check_device_call(const he_bfv_context* ctx, const void* records, size_t records_bytes, const uint8_t* present,
                      size_t count, const W* database, heamd::CiphertextWireLayout& layout, bool* run) {
    *run = false;
    const int status = payload_layout(ctx, layout);
    if (status != HE_OK) return status;
    const heamd::BfvContext& bfv = heamd::bfv_impl(ctx);
    if (sizeof(W) == 4 && bfv.word_bits() != 32) return invalid_argument("4-byte slabs need a Bfv<UInt32> context");
    if (count > 0xffffffffu) return invalid_argument("a database file holds at most UInt32.max plaintexts");
    if (count == 0) return HE_OK;
    if (records == nullptr || present == nullptr || database == nullptr) return invalid_argument("null buffer");
    const size_t slab_bytes = count * layout.rows * bfv.degree() * sizeof(W);
    if (heamd::ranges_overlap(records, records_bytes, database, slab_bytes)) return invalid_argument("database overlaps records");
    const he_poly_context* top = he_bfv_ciphertext_context(ctx, he_bfv_ciphertext_moduli_count(ctx));
    const int ready = top->impl->check_device();  // a host-only context: HE_ERR_DEVICE
    if (ready != HE_OK) return ready;
    *run = true;
    return HE_OK;
}

uint32_t log2_of(uint32_t degree) { return static_cast<uint32_t>(__builtin_ctz(degree)); }

template <typename W>
int database_load(const he_bfv_context* ctx, const uint8_t* records, size_t records_bytes, const uint8_t* present,
                  size_t count, W* database, uint32_t* device_mismatch, he_stream s) {
    heamd::CiphertextWireLayout layout{};
    bool run = false;
    const int status = check_device_call(ctx, records, records_bytes, present, count, database, layout, &run);
    if (status != HE_OK || !run) return status;
    hipStream_t stream = as_stream(s);
    Scratch ranks(stream);
    HEAMD_HIP_TRY(ranks.allocate((count + 1) * sizeof(uint32_t)));
    uint32_t* rank = static_cast<uint32_t*>(ranks.get());
    HEAMD_HIP_TRY(heamd::launch_pir_database_file_ranks(present, count, rank, stream));
    HEAMD_HIP_TRY(heamd::launch_pir_database_file_load(records, records_bytes, present, rank, count, database, layout,
                                                       log2_of(heamd::bfv_impl(ctx).degree()), device_mismatch, stream));
    return HE_OK;
}

template <typename W>
int database_save(const he_bfv_context* ctx, const W* database, const uint8_t* present, size_t count, uint8_t* records,
                  size_t records_bytes, uint32_t* device_mismatch, he_stream s) {
    heamd::CiphertextWireLayout layout{};
    bool run = false;
    const int status = check_device_call(ctx, records, records_bytes, present, count, database, layout, &run);
    if (status != HE_OK || !run) return status;
    hipStream_t stream = as_stream(s);
    Scratch ranks(stream);
    HEAMD_HIP_TRY(ranks.allocate((count + 1) * sizeof(uint32_t)));
    uint32_t* rank = static_cast<uint32_t*>(ranks.get());
    HEAMD_HIP_TRY(heamd::launch_pir_database_file_ranks(present, count, rank, stream));
    HEAMD_HIP_TRY(heamd::launch_pir_database_file_save(database, present, rank, count, records, records_bytes, layout,
                                                       log2_of(heamd::bfv_impl(ctx).degree()), device_mismatch, stream));
    return HE_OK;
}

}  // namespace

extern "C" int he_pir_database_file_scan(const he_bfv_context* ctx, const uint8_t* bytes, size_t byte_count,
                                         uint8_t* present_out, size_t capacity, size_t* out_count,
                                         size_t* out_present_count, size_t* out_bytes_consumed) {
    heamd::CiphertextWireLayout layout{};
    const int status = payload_layout(ctx, layout);
    if (status != HE_OK) return status;
    if (bytes == nullptr) return invalid_argument("null bytes");
    const size_t payload = static_cast<size_t>(layout.byte_offset[layout.rows]);
    if (byte_count < 1) return truncated("the header", 0, byte_count);
    if (bytes[0] != kSerializationVersion) {  // the version is read, and refused, before the count (:305-311)
        heamd::set_last_error("Invalid database: Invalid serialization version number " + std::to_string(bytes[0]) +
                              ", expected " + std::to_string(kSerializationVersion));
        return HE_ERR_INVALID_DATABASE_SERIALIZATION_VERSION;
    }
    if (byte_count < kHeaderBytes) return truncated("the header", byte_count, byte_count);
    const size_t count = size_t(bytes[1]) | size_t(bytes[2]) << 8 | size_t(bytes[3]) << 16 | size_t(bytes[4]) << 24;
    if (present_out != nullptr && capacity < count)
        return invalid_argument("the mask holds fewer bytes than the file has plaintexts");
    size_t at = kHeaderBytes, present_count = 0;
    for (size_t i = 0; i < count; ++i) {
        if (at >= byte_count) return truncated("plaintext " + std::to_string(i) + ", before its tag", at, byte_count);
        const uint8_t tag = bytes[at++];
        if (tag == kSerializedPlaintextTag) {
            if (byte_count - at < payload)
                return truncated("the payload of plaintext " + std::to_string(i), byte_count, byte_count);
            at += payload;
            ++present_count;
        } else if (tag != kSerializedZeroPlaintextTag) {
            heamd::set_last_error("Invalid database serialization plaintext tag: " + std::to_string(tag));
            return HE_ERR_INVALID_DATABASE_SERIALIZATION_PLAINTEXT_TAG;
        }
        if (present_out != nullptr) present_out[i] = tag;
    }
    if (out_count != nullptr) *out_count = count;
    if (out_present_count != nullptr) *out_present_count = present_count;
    if (out_bytes_consumed != nullptr) *out_bytes_consumed = at;
    return HE_OK;
}

extern "C" int he_pir_database_file_byte_count(const he_bfv_context* ctx, const uint8_t* present, size_t count, size_t* out) {
    heamd::CiphertextWireLayout layout{};
    const int status = payload_layout(ctx, layout);
    if (status != HE_OK) return status;
    if (out == nullptr) return invalid_argument("null out");
    if (count != 0 && present == nullptr) return invalid_argument("null mask");
    if (count > 0xffffffffu) return invalid_argument("a database file holds at most UInt32.max plaintexts");
    size_t present_count = 0;
    for (size_t i = 0; i < count; ++i) present_count += present[i] != 0;
    *out = kHeaderBytes + count + static_cast<size_t>(layout.byte_offset[layout.rows]) * present_count;  // :343-346
    return HE_OK;
}

extern "C" int he_pir_database_file_header(size_t count, uint8_t out[5]) {
    if (out == nullptr) return invalid_argument("null out");
    if (count > 0xffffffffu) return invalid_argument("a database file holds at most UInt32.max plaintexts");
    out[0] = kSerializationVersion;
    for (int b = 0; b < 4; ++b) out[1 + b] = static_cast<uint8_t>(count >> (8 * b));  // UInt32.littleEndianBytes (:367)
    return HE_OK;
}

extern "C" int he_pir_database_load_device(const he_bfv_context* ctx, const uint8_t* records, size_t records_bytes,
                                           const uint8_t* present, size_t count, uint64_t* database,
                                           uint32_t* device_mismatch, he_stream s) {
    return database_load(ctx, records, records_bytes, present, count, database, device_mismatch, s);
}
extern "C" int he_pir_database_load_device_u32(const he_bfv_context* ctx, const uint8_t* records, size_t records_bytes,
                                               const uint8_t* present, size_t count, uint32_t* database,
                                               uint32_t* device_mismatch, he_stream s) {
    return database_load(ctx, records, records_bytes, present, count, database, device_mismatch, s);
}
extern "C" int he_pir_database_save_device(const he_bfv_context* ctx, const uint64_t* database, const uint8_t* present,
                                           size_t count, uint8_t* records, size_t records_bytes, uint32_t* device_mismatch,
                                           he_stream s) {
    return database_save(ctx, database, present, count, records, records_bytes, device_mismatch, s);
}
extern "C" int he_pir_database_save_device_u32(const he_bfv_context* ctx, const uint32_t* database, const uint8_t* present,
                                               size_t count, uint8_t* records, size_t records_bytes,
                                               uint32_t* device_mismatch, he_stream s) {
    return database_save(ctx, database, present, count, records, records_bytes, device_mismatch, s);
}
