"""The memory footprint of one call, on memory the test owns: one contiguous byte arena that holds every slab of the call
between guard bytes, the image that arena must show after the call, and a verifier that names the first byte that differs.

Layout, in order: a head guard; the call's slabs in the order of their table row (tests/aliasing_cases.py), each starting on a
256-byte boundary and spanning exactly its stated bytes, so that the last byte of a slab abuts guard bytes (the padding up to the
next boundary is guard too); a tail guard behind the last slab.  Head and tail guard are each at least as long as the largest
slab the call writes: a store one whole slab off its target still lands in memory the test owns and is seen, not a fault.

Nothing here imports the device package.  An arena's bytes are whatever buffer the caller brings -- a numpy uint8 array or a
torch uint8 tensor: only slicing, `!=`, `.any()` and a copy are asked of it, and bytes reach the host only to word a failure.
"""
import collections

ALIGN = 256      # every slab starts on such a boundary (the library asks for 16; a cache line is 128)
MIN_GUARD = 4096  # of the head and the tail guard, whatever the call writes
GUARD_BYTE = 0x5A  # guard bytes, padding and read-only padding
POISONS = (0xA5, 0xFF)  # pure outputs and workspaces: once each (0xFF: words above every modulus)

Arena = collections.namedtuple("Arena", "offsets sizes written head tail total")


def _up(value, to=ALIGN):
    return (value + to - 1) // to * to


def layout(sizes, written):
    """sizes: {slab: bytes} in table order; written: the slabs the call writes -> Arena (offsets from the arena's first byte,
    which the caller puts on an ALIGN boundary)"""
    sizes = collections.OrderedDict(sizes)
    guard = _up(max([MIN_GUARD] + [sizes[name] for name in written]))
    offsets, at = collections.OrderedDict(), guard
    for name, size in sizes.items():
        offsets[name] = at
        at = _up(at + size + 1)  # at least one guard byte behind every slab
    last = list(sizes)[-1]
    end = offsets[last] + sizes[last]
    return Arena(offsets, sizes, tuple(written), guard, guard, end + guard)


def span(arena, name):
    return arena.offsets[name], arena.offsets[name] + arena.sizes[name]


def locate(arena, byte):
    """-> (region, slab, offset): region is "slab", "head guard", "padding" or "tail guard"; guard and padding bytes are counted
    from the nearer slab (the one before it on a tie): an offset below 0 lies before the slab's first byte, one at or above its
    size behind its last"""
    names = list(arena.offsets)
    if byte < arena.offsets[names[0]]:
        return "head guard", names[0], byte - arena.offsets[names[0]]
    for i, name in enumerate(names):
        begin, end = span(arena, name)
        if begin <= byte < end:
            return "slab", name, byte - begin
        following = arena.offsets[names[i + 1]] if i + 1 < len(names) else None
        if following is None:
            return "tail guard", name, byte - begin
        if byte < following:
            if byte - (end - 1) <= following - byte:
                return "padding", name, byte - begin
            return "padding", names[i + 1], byte - following
    raise AssertionError("byte %d is not in the arena" % byte)


def _copy(buffer):
    return buffer.clone() if hasattr(buffer, "clone") else buffer.copy()


def expected_image(arena, filled):
    """The whole arena as it must read after the call -> (image, masked): guard bytes and the slabs the call only reads as they
    were filled; `masked` lists the [begin, end) of the written slabs, whose bytes in `image` mean nothing"""
    assert len(filled) == arena.total
    return _copy(filled), [span(arena, name) for name in arena.written]


def first_difference(arena, got, image, masked):
    """-> None, or (byte, region, slab, offset) of the first byte outside the masked ranges at which `got` is not `image`"""
    differs = got != image
    for begin, end in masked:
        differs[begin:end] = False
    if not bool(differs.any()):
        return None
    byte = int(differs.nonzero()[0][0]) if not hasattr(differs, "cpu") else int(differs.nonzero()[0, 0].cpu())
    return (byte,) + locate(arena, byte)


def verify(arena, got, image, masked, what=""):
    """Asserts that `got` equals `image` outside the masked ranges; the failure names the first differing byte by region, slab
    and offset, and counts the rest"""
    found = first_difference(arena, got, image, masked)
    if found is None:
        return
    byte, region, slab, offset = found
    differs = got != image
    for begin, end in masked:
        differs[begin:end] = False
    count = int(differs.sum())
    raise AssertionError("%s: %d byte(s) changed outside the written slabs; the first is arena byte %d, %s, %s%+d (%s spans %d "
                         "bytes): 0x%02x -> 0x%02x" % (what, count, byte, region, slab, offset, slab, arena.sizes[slab],
                                                       int(image[byte]), int(got[byte])))
