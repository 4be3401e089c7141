"""Plain restatements of the ciphertext-level wire format, in Python integers:

  skip_lsbs_for_decryption  Bfv.skipLSBsForDecryption (Bfv/Bfv+Decrypt.swift:51-109)
  widths / record_bytes     the per-(polynomial, row) field widths and Serialize.serializePolysBufferSize
  pack_ciphertext           the `polys` bytes of SerializedCiphertext.full: the count as a little-endian UInt16, then
                            wire_format_reference.pack_record of each polynomial at its own skipLSBs (Serialize.swift:31-67)
  unpack_ciphertext         the inverse (Serialize.swift:70-94), nothing validated; also returns the header's count
  seeded_polynomial         PolyRq<_, Eval>.random(NistAes128Ctr(seed)): wire_format_reference.CtrDrbg in 4096-byte refills,
                            128 little-endian stream bits per coefficient mod q_r (PolyRq+Randomize.swift:56-75)
  ciphertext_form           csrc/ciphertext_wire_form.hpp restated
  poly_form                 csrc/serialize_form.hpp's for_serialize_narrow / for_deserialize_narrow restated (4-byte slabs:
                            word or byte, never tile)

tests/test_ciphertext_wire.py holds the library's host entries and the two headers to these without a device;
tests/test_gpu_ciphertext_wire.py compares every byte and word the device entries produce with them."""
import math

import wire_format_reference as W


def ceil_log2(x):
    return (int(x) - 1).bit_length()


def skip_lsbs_for_decryption(degree, q0, t, moduli_count=1):
    if moduli_count != 1:
        return [0, 0]
    l_prime = (q0 // t).bit_length() - 1 - 3 if q0 >= 2 * t else 0
    tmp = int(8.0 * math.sqrt(2.0 * degree / 9.0))
    poly1 = l_prime - (0 if tmp == 0 else ceil_log2(tmp))
    if poly1 <= 1:
        return [max(l_prime + 1, 0), 0]
    return [max(l_prime, 0), poly1]


def widths(moduli, skip):
    return [ceil_log2(q) - skip for q in moduli]


def record_bytes(degree, moduli, skips):
    return 2 + sum(W.row_offsets(degree, widths(moduli, skip))[-1] for skip in skips)


def pack_ciphertext(polys, degree, moduli, skips):
    """polys: [poly_count][L][N] integers -> bytes"""
    assert len(polys) == len(skips)
    out = len(polys).to_bytes(2, "little")
    for rows, skip in zip(polys, skips):
        out += W.pack_record(rows, widths(moduli, skip), skip)
    return out


def unpack_ciphertext(record, poly_count, degree, moduli, skips):
    """-> (the header's count, [poly_count][L][N] integers); the record is read as poly_count polynomials whatever its header"""
    record = bytes(record)
    at, polys = 2, []
    for skip in skips[:poly_count]:
        w = widths(moduli, skip)
        size = W.row_offsets(degree, w)[-1]
        polys.append(W.unpack_record(record[at:at + size], degree, w, skip))
        at += size
    return int.from_bytes(record[:2], "little"), polys


_SEEDED = {}


def seeded_polynomial(seed, degree, moduli):
    """[L][N] integers, Eval form as the reference stores them"""
    key = (bytes(seed), degree, tuple(moduli))
    if key not in _SEEDED:
        words = degree * len(moduli)
        drbg, stream = W.CtrDrbg(seed), b""
        while len(stream) < 16 * words:
            stream += drbg.generate(4096)  # BufferedRng(bufferCount: 4096): every refill is one generate() and one re-key
        flat = [int.from_bytes(stream[16 * i:16 * i + 16], "little") % moduli[i // degree] for i in range(words)]
        _SEEDED[key] = [flat[r * degree:(r + 1) * degree] for r in range(len(moduli))]
    return _SEEDED[key]


CHUNK = 8


def ciphertext_form(direction, degree, moduli_count, poly_count, record_byte_count, record_stride, records_address):
    """what he_ciphertexts_wire_plan reports for poly_count 1..3"""
    edge_free = records_address % CHUNK == 0 and record_stride % CHUNK == 0
    if direction == "serialize":
        # the most aligned 8-byte chunks a record can overlap: one that starts 7 bytes into a chunk
        return {"form": "chunk", "record_bytes": record_byte_count, "items_per_record": (record_byte_count + 7 + 7) // 8,
                "edge_free": edge_free}
    assert direction == "deserialize"
    return {"form": "field", "record_bytes": record_byte_count, "items_per_record": poly_count * moduli_count * degree,
            "edge_free": edge_free}


def poly_form(word_bytes, direction, degree, field_widths, bytes_address, slab_address, bytes_per_poly=None):
    if word_bytes == 8:
        return W.form(direction, degree, field_widths, bytes_address, slab_address, bytes_per_poly)
    offsets = W.row_offsets(degree, field_widths)
    stride = 0 if direction == "serialize" else (offsets[-1] if bytes_per_poly is None else bytes_per_poly)
    if bytes_address % 8 == 0 and all(o % 8 == 0 for o in offsets) and stride % 8 == 0:
        return "word"
    return "byte"
