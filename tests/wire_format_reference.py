"""Plain restatements of the wire-format path, in Python integers and independent of the oracle:

  Aes128           FIPS-197 block encryption and key expansion; the only table is the S-box, built from the field inverse
  CtrDrbg          NIST SP 800-90A CTR_DRBG, AES-128, no derivation function, as Random/NistCtrDrbg.swift:52-86 has it: the
                   counter V is a Python int and every addition is taken modulo 2^128
  seed_for_counter the 32-byte seed after whose init(entropy:) the counter V is a chosen value
  carry_cases      the seeds whose counter sits just below a 2^32, 2^64, 2^96 or 2^128 boundary
  pack / unpack    CoefficientPacking (CoefficientPacking.swift:79-213): a row is ONE big-endian integer of n fields
  form             which kernel form (byte, word, tile) csrc/serialize_form.hpp chooses for a call

tests/test_wire_format_reference.py holds these to the FIPS-197 and NIST vectors, to the golden packing vectors, and holds the
oracle and csrc/serialize_form.hpp to them; tests/test_gpu_wire_format_edges.py uses them next to the oracle."""

MASK128 = (1 << 128) - 1


# ---- AES-128 (FIPS-197) ------------------------------------------------------------------------------------------------------
def _xtime(a):
    a <<= 1
    return (a ^ 0x11b) if a & 0x100 else a


def _gf_mul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a = _xtime(a)
        b >>= 1
    return r


def _sbox_entry(x):
    # FIPS-197 5.1.1: the inverse in GF(2^8) (x^254; 0 -> 0), then the affine map
    inverse = 1
    for _ in range(254):
        inverse = _gf_mul(inverse, x)
    if x == 0:
        inverse = 0
    s = inverse
    for k in range(1, 5):
        s ^= ((inverse << k) | (inverse >> (8 - k))) & 0xff
    return s ^ 0x63


SBOX = tuple(_sbox_entry(x) for x in range(256))
# ShiftRows on a column-major state: byte (row r, column c) sits at 4 c + r and comes from column c + r
_SHIFT_ROWS = tuple(4 * ((c + r) % 4) + r for c in range(4) for r in range(4))


class Aes128:
    def __init__(self, key):
        key = bytes(key)
        assert len(key) == 16
        words = [list(key[4 * i:4 * i + 4]) for i in range(4)]  # FIPS-197 5.2
        rcon = 1
        for i in range(4, 44):
            t = list(words[i - 1])
            if i % 4 == 0:
                t = [SBOX[t[1]] ^ rcon, SBOX[t[2]], SBOX[t[3]], SBOX[t[0]]]
                rcon = _xtime(rcon)
            words.append([a ^ b for a, b in zip(words[i - 4], t)])
        self.round_keys = [sum((words[4 * r + c] for c in range(4)), []) for r in range(11)]

    def encrypt(self, block):
        """one 16-byte block (bytes, or an int taken big-endian) -> 16 bytes"""
        if isinstance(block, int):
            block = block.to_bytes(16, "big")
        assert len(block) == 16
        rk = self.round_keys
        s = [a ^ b for a, b in zip(block, rk[0])]
        for r in range(1, 10):
            s = [SBOX[s[i]] for i in _SHIFT_ROWS]
            mixed = []
            for c in range(0, 16, 4):
                a0, a1, a2, a3 = s[c:c + 4]
                t = a0 ^ a1 ^ a2 ^ a3  # FIPS-197 5.1.3: column times (2, 3, 1, 1) circulant
                mixed += [a0 ^ t ^ _xtime(a0 ^ a1), a1 ^ t ^ _xtime(a1 ^ a2), a2 ^ t ^ _xtime(a2 ^ a3), a3 ^ t ^ _xtime(a3 ^ a0)]
            s = [a ^ b for a, b in zip(mixed, rk[r])]
        return bytes(SBOX[s[i]] ^ k for i, k in zip(_SHIFT_ROWS, rk[10]))


# ---- CTR_DRBG ----------------------------------------------------------------------------------------------------------------
class CtrDrbg:
    """NistCtrDrbg.swift:52-86.  `blocks` counts the AES blocks restated so far (the tests budget them)."""

    def __init__(self, entropy):
        entropy = bytes(entropy)
        assert len(entropy) == 32
        self.blocks = 0
        self.v = 0
        self._set_key(bytes(16))
        self._update(entropy)

    def _set_key(self, key):
        self.key = key
        self._aes = Aes128(key)

    def _stream(self, block_count):
        self.blocks += block_count
        return b"".join(self._aes.encrypt((self.v + 1 + i) & MASK128) for i in range(block_count))

    def _update(self, provided):
        out = bytes(a ^ b for a, b in zip(self._stream(2), provided))
        self._set_key(out[:16])
        self.v = int.from_bytes(out[16:], "big")

    def state(self):
        return self.key, self.v.to_bytes(16, "big")

    def generate(self, count):
        block_count = -(-count // 16)
        out = self._stream(block_count)[:count]
        self.v = (self.v + block_count) & MASK128
        self._update(bytes(32))
        return out


_E0_OF_2 = int.from_bytes(Aes128(bytes(16)).encrypt(2), "big")


def seed_for_counter(v0, key_part=bytes(16)):
    """The seed after whose init the counter is v0: init runs update(entropy) from key 0, V 0, so V_0 = E_0(0...02) ^ entropy[16:32];
    entropy[0:16] stays free and sets the key (key_0 = E_0(0...01) ^ entropy[0:16])."""
    key_part = bytes(key_part)
    assert 0 <= v0 <= MASK128 and len(key_part) == 16
    return key_part + (_E0_OF_2 ^ v0).to_bytes(16, "big")


# The counter additions of a seeded polynomial (csrc/seeded_kernels.hip): chunk 0 draws its blocks from V + 1 .. V + 256, the
# counter then moves to V + 256 and the re-key draws from V + 257 and V + 258.  V_0 = B - k puts the boundary B at any of them.
CARRY_OFFSETS = (1, 2, 4, 5, 129, 253, 254, 255, 256, 257, 258, 259)
# boundary bits -> the bits of V_0 above the boundary: arbitrary, not all ones, and the word just above is not all ones either
# (a carry out of the words below stops there)
CARRY_UPPER = {
    32: 0x01234567_89abcdef_7fffff00,
    64: 0xdeadbeef_80000001,
    96: 0xfffffffe,
    128: 0,
}


def carry_cases():
    """[(boundary bits, k, V_0, seed)] with V_0 = upper * 2^bits + 2^bits - k; every seed has its own key part"""
    cases = []
    for bits, upper in CARRY_UPPER.items():
        for k in CARRY_OFFSETS:
            v0 = (upper << bits) + (1 << bits) - k
            key_part = bytes((37 * bits + 11 * k + 5 * i) & 0xff for i in range(16))
            cases.append((bits, k, v0, seed_for_counter(v0, key_part)))
    return cases


def carries(v, amount, bits):
    """v + amount carries out of the low `bits` bits"""
    return (v & ((1 << bits) - 1)) + amount >= (1 << bits)


# ---- coefficient packing -----------------------------------------------------------------------------------------------------
def row_byte_count(n, width):
    return (n * width + 7) // 8


def pack(values, width, skip=0):
    """n fields (value >> skip, its low `width` bits) as one big-endian integer, zero-padded at the end to a whole byte"""
    whole = 0
    for value in values:
        whole = (whole << width) | ((int(value) >> skip) & ((1 << width) - 1))
    count = row_byte_count(len(values), width)
    return (whole << (8 * count - len(values) * width)).to_bytes(count, "big")


def unpack(row_bytes, n, width, skip=0):
    """the n leading `width`-bit fields of the bytes taken as one big-endian integer (bytes past the end read as zero), each
    shifted left by skip; nothing is validated, pad bits and fields at or above a modulus included"""
    row_bytes = bytes(row_bytes)
    count = max(len(row_bytes), row_byte_count(n, width))
    whole = int.from_bytes(row_bytes.ljust(count, b"\0"), "big")
    top = 8 * count
    return [((whole >> (top - (k + 1) * width)) & ((1 << width) - 1)) << skip for k in range(n)]


def row_offsets(degree, widths):
    offsets = [0]
    for width in widths:
        offsets.append(offsets[-1] + row_byte_count(degree, width))
    return offsets


def pack_record(rows, widths, skip=0):
    return b"".join(pack(row, width, skip) for row, width in zip(rows, widths))


def unpack_record(record, degree, widths, skip=0):
    offsets = row_offsets(degree, widths)
    return [unpack(record[offsets[r]:offsets[r + 1]], degree, width, skip) for r, width in enumerate(widths)]


# ---- the kernel form ---------------------------------------------------------------------------------------------------------
def form(direction, degree, widths, bytes_address, slab_address, bytes_per_poly=None):
    """csrc/serialize_form.hpp restated: "tile" needs whole 128-coefficient tiles and 16-byte alignment of every row, of the
    record, of both buffers and (deserialize) of the record stride; "word" needs 8-byte alignment of every row, of the record,
    of the byte buffer and (deserialize) of the stride; "byte" is the rest.  widths are the field widths (skip taken off)."""
    assert direction in ("serialize", "deserialize")
    offsets = row_offsets(degree, widths)
    stride = 0 if direction == "serialize" else (offsets[-1] if bytes_per_poly is None else bytes_per_poly)
    if (degree >= 128 and all(1 <= w <= 64 for w in widths) and bytes_address % 16 == 0 and slab_address % 16 == 0
            and all(o % 16 == 0 for o in offsets) and stride % 16 == 0):
        return "tile"
    if bytes_address % 8 == 0 and all(o % 8 == 0 for o in offsets) and stride % 8 == 0:
        return "word"
    return "byte"
