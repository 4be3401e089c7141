"""ProcessedDatabase.serialize() / init(from:context:) restated in Python integers (reference Sources/PrivateInformationRetrieval/
IndexPir/IndexPirProtocol.swift:248-379) over tests/wire_format_reference.py, which tests/test_wire_format_reference.py holds to
the oracle and to csrc/serialize_form.hpp.

A plaintext is None (nil) or its [L][N] rows of Python integers over the top-level ciphertext context; the payload of a present
plaintext is Plaintext<Eval>.serialize().poly = PolyRq.serialize with skipLSBs 0: wire_format_reference.pack_record at
ceilLog2(q_r) bits per coefficient."""
import wire_format_reference as W

SERIALIZATION_VERSION = 1      # IndexPirProtocol.swift:253-255 (serializationVersion)
ZERO_PLAINTEXT_TAG = 0         # :258-260 (serializedZeroPlaintextTag)
PLAINTEXT_TAG = 1              # :263-265 (serializedPlaintextTag)
VERSION_BYTES = 1              # :251, :306, :343 (SerializationVersionType = UInt8)
COUNT_BYTES = 4                # :313-315, :344, :367 (UInt32, little-endian)
HEADER_BYTES = VERSION_BYTES + COUNT_BYTES
TAG_BYTES = 1                  # :319-320, :346


class InvalidVersion(ValueError):
    """PirError.invalidDatabaseSerializationVersion (:307-311)"""


class InvalidTag(ValueError):
    """PirError.invalidDatabaseSerializationPlaintextTag (:329-330)"""


class Truncated(ValueError):
    """the reference's array subscripts trap (:305, :314, :319, :325)"""


def widths(moduli):
    """ceilLog2 of every modulus (ModularArithmetic/Scalar.swift:266-269): the bits per coefficient at skipLSBs 0"""
    return [(int(q) - 1).bit_length() for q in moduli]


def payload_bytes(degree, moduli):
    """context.ciphertextContext.serializationByteCount() (:317)"""
    return W.row_offsets(degree, widths(moduli))[-1]


def header(count):
    assert 0 <= count < 1 << 32
    return bytes([SERIALIZATION_VERSION]) + count.to_bytes(COUNT_BYTES, "little")  # :366-367


def serialize_body(plaintexts, moduli):
    """:369-376: per plaintext its tag and, when it is not nil, its payload"""
    out = bytearray()
    for plaintext in plaintexts:
        if plaintext is None:
            out.append(ZERO_PLAINTEXT_TAG)
        else:
            out.append(PLAINTEXT_TAG)
            out += W.pack_record(plaintext, widths(moduli))
    return bytes(out)


def serialize(plaintexts, moduli):
    """ProcessedDatabase.serialize() (:362-378)"""
    return header(len(plaintexts)) + serialize_body(plaintexts, moduli)


def byte_count(present, payload):
    """serializationByteCount (:338-349), for any database (the reference throws emptyDatabase when nothing is present: it
    takes the polynomial's size from the first plaintext)"""
    return HEADER_BYTES + TAG_BYTES * len(present) + payload * sum(1 for p in present if p)


def tag_offset(present, index, payload):
    """where the tag of plaintext `index` lies in the BODY: index + payload * rank(index)"""
    return TAG_BYTES * index + payload * sum(1 for p in present[:index] if p)


def scan(data, payload):
    """the walk of init(from:context:) (:303-334) without the payloads -> (present, bytes consumed)"""
    data = bytes(data)
    if len(data) < VERSION_BYTES:
        raise Truncated("no version byte")
    if data[0] != SERIALIZATION_VERSION:
        raise InvalidVersion(data[0])
    if len(data) < HEADER_BYTES:
        raise Truncated("inside the count")
    count = int.from_bytes(data[VERSION_BYTES:HEADER_BYTES], "little")
    offset, present = HEADER_BYTES, []
    for index in range(count):
        if offset >= len(data):
            raise Truncated(f"before the tag of plaintext {index}")
        tag = data[offset]
        offset += TAG_BYTES
        if tag == PLAINTEXT_TAG:
            if offset + payload > len(data):
                raise Truncated(f"inside the payload of plaintext {index}")
            offset += payload
        elif tag != ZERO_PLAINTEXT_TAG:
            raise InvalidTag(tag)
        present.append(tag)
    return present, offset


def deserialize(data, degree, moduli):
    """ProcessedDatabase.init(from:context:) (:303-334) -> the plaintexts, None for nil; fields are taken as they come
    (PolyRq(deserialize:) does not validate them)"""
    payload = payload_bytes(degree, moduli)
    present, _ = scan(data, payload)
    data = bytes(data)
    offset, out = HEADER_BYTES, []
    for tag in present:
        offset += TAG_BYTES
        if tag:
            out.append(W.unpack_record(data[offset:offset + payload], degree, widths(moduli)))
            offset += payload
        else:
            out.append(None)
    return out


def deserialize_body(body, present, degree, moduli):
    """a segment of the body under its mask (any byte != 0: present) -> plaintexts; bytes past the end read as zero"""
    payload = payload_bytes(degree, moduli)
    body = bytes(body)
    out = []
    for index, here in enumerate(present):
        if not here:
            out.append(None)
            continue
        start = tag_offset(present, index, payload) + TAG_BYTES
        out.append(W.unpack_record(body[start:start + payload].ljust(payload, b"\0"), degree, widths(moduli)))
    return out


def slab(plaintexts, rows, degree):
    """the device database of these plaintexts: [count][L][N] integers, a nil plaintext all zeros"""
    zero = [[0] * degree for _ in range(rows)]
    return [zero if p is None else p for p in plaintexts]
