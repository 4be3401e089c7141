"""The argument checks of every entry point that exists for 8-byte and for 4-byte slabs, twin by twin, without a device.

Both twins of a pair run one body; what differs between them on purpose -- the order of the word-size check, where the
4-byte polynomial entries look for their 4-byte tables, which of them record a last-error text -- is pinned here: the status
and, where the entry sets one, the text, for a null context, a moduli_count out of range, host-only contexts, moduli above
2^30 - 1 and a non-NTT modulus.  Host-only contexts come from he_*_create_host_only, which builds Bfv<UInt64> constants
only (a Bfv<UInt32> context needs a device), so "the other word size" is always an 8-byte context given to a 4-byte twin;
it is built once over 40-bit and once over 28-bit moduli.
"""
import ctypes

import pytest

import heamd
from heamd.binding import STATUS_NAMES, c_size, c_u32, c_u64, vp

DEGREE = 8
SOMEWHERE = 0x1000  # a non-null slab that no entry reaches: every call here fails or returns before its first launch

HOST_ONLY = "context was created host-only (no device tables)"
HOST_ONLY_POLY = HOST_ONLY + "; compute entry points need a GPU context"
OTHER_WORD = "invalid argument: 4-byte slabs need a Bfv<UInt32> context"

BFV_PAIRS = [
    "he_rns_lift_q_to_qbsk_device", "he_rns_floor_qbsk_to_q_device", "he_rns_scale_and_round_device",
    "he_bfv_plaintext_to_eval_device", "he_bfv_plaintext_to_coeff_device", "he_bfv_mod_switch_down_device",
    "he_bfv_mul_plain_device", "he_bfv_add_plain_device", "he_bfv_sub_plain_device",
    "he_bfv_inner_product_plain_resident_device", "he_bfv_inner_product_device", "he_bfv_inner_product_shared_device",
]
# the one 4-byte entry that looks at the word size before the level
WORD_SIZE_FIRST = "he_bfv_inner_product_plain_resident_device_u32"

def elsewhere(slab):
    """A second slab, far from the first: in and out of an out-of-place entry must not overlap (the in-place entries above it
    may take one slab as both operands: x + x, x - x, x * x)."""
    return None if slab is None else slab + 0x100000


# (entry, arguments between the context and the stream for a batch of `batch` with slabs at `slab`)
POLY_PAIRS = {
    "he_ntt_forward_device": lambda slab, batch: (slab, batch),
    "he_ntt_inverse_device": lambda slab, batch: (slab, batch),
    "he_poly_add_device": lambda slab, batch: (slab, slab, batch),
    "he_poly_sub_device": lambda slab, batch: (slab, slab, batch),
    "he_poly_neg_device": lambda slab, batch: (slab, batch),
    "he_poly_mul_device": lambda slab, batch: (slab, slab, batch),
    "he_poly_mul_scalar_device": lambda slab, batch: (slab, None, batch),  # the residues are filled in by poly_call
    "he_poly_divide_and_round_q_last_device": lambda slab, batch: (slab, elsewhere(slab), batch),
}
TRANSFORMS = ("he_ntt_forward_device", "he_ntt_inverse_device")


@pytest.fixture(scope="module")
def lib():
    return heamd.load_library()


def outcome(lib, status):
    return STATUS_NAMES[status], lib.he_last_error_message().decode()


def mark_last_error(lib):
    """Leaves a known last-error text behind, so that an entry that records none shows it unchanged."""
    assert STATUS_NAMES[lib.he_device_malloc(None, 0)] == "invalidArgument"
    return lib.he_last_error_message().decode()


def bfv_call(lib, name, handle, moduli_count):
    """The entry with benign arguments behind (context, moduli_count): counts of one, null slabs."""
    fn = getattr(lib, name)
    filler = {c_u32: 1, c_size: 1, c_u64: 0}
    rest = [filler.get(kind) for kind in fn.argtypes[2:]]
    mark_last_error(lib)
    return outcome(lib, fn(handle, moduli_count, *rest))


def poly_call(lib, name, handle, slab, batch):
    fn = getattr(lib, name)
    args = list(POLY_PAIRS[name.replace("_u32", "")](slab, batch))
    if "mul_scalar" in name:
        residues = ((ctypes.c_uint32 if name.endswith("_u32") else ctypes.c_uint64) * 4)(0, 0, 0, 0)
        args[1] = ctypes.cast(residues, fn.argtypes[2])
    mark_last_error(lib)
    return outcome(lib, fn(handle, *args, None))


@pytest.fixture(scope="module")
def bfv_contexts():
    t = heamd.generate_primes([17], True, DEGREE)[0]
    return [heamd.BfvContext(DEGREE, t, heamd.generate_primes(bits, False, DEGREE), host_only=True)
            for bits in ([40, 40, 41], [27, 28, 28])]


@pytest.mark.parametrize("pair", BFV_PAIRS)
def test_bfv_twins(lib, bfv_contexts, pair):
    for name in (pair, pair + "_u32"):
        assert bfv_call(lib, name, None, 1) == ("invalidArgument", "invalid argument: null context"), name
        for ctx in bfv_contexts:
            assert ctx.L == 2
            word_first = name == WORD_SIZE_FIRST
            expected = ("invalidArgument", OTHER_WORD if word_first else "invalid argument: moduli_count out of range")
            for count in (0, 3, 99):
                assert bfv_call(lib, name, ctx.h, count) == expected, (name, count)
            # a context of the other word size AND host-only: every 4-byte twin but one finds the missing tables first
            expected = ("invalidArgument", OTHER_WORD) if word_first else ("deviceError", HOST_ONLY)
            for count in (1, 2):
                assert bfv_call(lib, name, ctx.h, count) == expected, (name, count)


@pytest.fixture(scope="module")
def poly_contexts():
    make = lambda degree, moduli: heamd.PolyContext(degree, moduli, host_only=True)
    return {
        "narrow": make(DEGREE, heamd.generate_primes([28, 29], False, DEGREE)),
        "wide": make(DEGREE, heamd.generate_primes([28, 40], False, DEGREE)),
        "non_ntt": make(4, [2, 3, 5]),
    }


@pytest.mark.parametrize("pair", list(POLY_PAIRS))
def test_poly_twins_null_context(lib, pair):
    what = "null pointer" if "mul_scalar" in pair else "null context"
    for name in (pair, pair + "_u32"):
        for batch in (0, 1):
            assert poly_call(lib, name, None, SOMEWHERE, batch) == ("invalidArgument", "invalid argument: " + what), name


@pytest.mark.parametrize("pair", [p for p in POLY_PAIRS if p not in TRANSFORMS])
@pytest.mark.parametrize("which", ["narrow", "non_ntt"])
def test_poly_twins_host_only(lib, poly_contexts, pair, which):
    """8-byte: an empty batch is done, then the slabs, then the device.  4-byte: the device before either.  A non-NTT modulus
    is no obstacle to anything but a transform."""
    ctx = poly_contexts[which]
    nothing = mark_last_error(lib)
    device = ("deviceError", HOST_ONLY_POLY)
    assert poly_call(lib, pair, ctx.h, None, 0) == ("ok", nothing)
    assert poly_call(lib, pair, ctx.h, SOMEWHERE, 1) == device
    # (he_poly_mul_scalar_device never looked at its slab)
    assert poly_call(lib, pair, ctx.h, None, 1) == (device if "mul_scalar" in pair
                                                    else ("invalidArgument", "invalid argument: null slab"))
    for slab, batch in ((None, 0), (None, 1), (SOMEWHERE, 1)):
        assert poly_call(lib, pair + "_u32", ctx.h, slab, batch) == device, (slab, batch)


@pytest.mark.parametrize("pair", TRANSFORMS)
def test_transform_twins_host_only(lib, poly_contexts, pair):
    ctx = poly_contexts["narrow"]
    nothing = mark_last_error(lib)
    device = ("deviceError", HOST_ONLY_POLY)
    assert poly_call(lib, pair, ctx.h, None, 0) == ("ok", nothing)
    assert poly_call(lib, pair, ctx.h, None, 1) == ("invalidArgument", "invalid argument: null slab")
    assert poly_call(lib, pair, ctx.h, SOMEWHERE, 1) == device
    for slab, batch in ((None, 0), (None, 1), (SOMEWHERE, 1)):
        assert poly_call(lib, pair + "_u32", ctx.h, slab, batch) == device, (slab, batch)


@pytest.mark.parametrize("pair", TRANSFORMS)
def test_transform_twins_non_ntt_modulus(lib, poly_contexts, pair):
    """validateNttModuli comes before everything else; only the 8-byte entry says which degree."""
    ctx = poly_contexts["non_ntt"]
    nothing = mark_last_error(lib)
    for slab, batch in ((None, 0), (None, 1), (SOMEWHERE, 1)):
        assert poly_call(lib, pair, ctx.h, slab, batch) == (
            "invalidNttModulus", "a modulus of this context is not an NTT modulus for degree 4")
        assert poly_call(lib, pair + "_u32", ctx.h, slab, batch) == ("invalidNttModulus", nothing)


@pytest.mark.parametrize("pair", list(POLY_PAIRS))
def test_poly_twins_modulus_above_30_bits(lib, poly_contexts, pair):
    """A 4-byte twin refuses a modulus above 2^30 - 1 whatever the batch; the 8-byte twin has no such limit."""
    ctx = poly_contexts["wide"]
    wide = [m for m in ctx.moduli if m > 2 ** 30 - 1]
    assert len(wide) == 1
    nothing = mark_last_error(lib)
    assert poly_call(lib, pair, ctx.h, None, 0) == ("ok", nothing)
    assert poly_call(lib, pair, ctx.h, SOMEWHERE, 1) == ("deviceError", HOST_ONLY_POLY)
    for slab, batch in ((None, 0), (None, 1), (SOMEWHERE, 1)):
        assert poly_call(lib, pair + "_u32", ctx.h, slab, batch) == (
            "invalidModulus", "modulus %d does not fit UInt32 (max 2^30 - 1)" % wide[0]), (slab, batch)


def test_one_modulus_has_no_q_last(lib):
    ctx = heamd.PolyContext(DEGREE, heamd.generate_primes([28], False, DEGREE), host_only=True)
    nothing = mark_last_error(lib)
    for name in ("he_poly_divide_and_round_q_last_device", "he_poly_divide_and_round_q_last_device_u32"):
        for batch in (0, 1):
            assert poly_call(lib, name, ctx.h, SOMEWHERE, batch) == ("invalidPolyContext", nothing), name
