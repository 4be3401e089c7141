"""tests/footprint_cases.py held to tests/aliasing_cases.py and to include/he_amd.h, and tests/footprint.py -- the arena and its
verifier -- exercised on numpy buffers.  No device: tests/test_gpu_footprint.py runs the rows on one."""
import numpy as np
import pytest

import aliasing_cases as A
import footprint
import footprint_cases as F
from test_aliasing_contract import prototypes


def ring_moduli(shp, word_bytes):
    return [(1 << bits) - 1 for bits in shp.bits[8 * word_bytes]]  # (sizes depend on the bit lengths alone)


def every_layout():
    for row in A.CASES:
        for shp in F.shapes(row):
            for word_bytes in F.words_of(row, shp):
                env = F.environment(row, shp, ring_moduli(shp, word_bytes), word_bytes)
                if row.name in F.WORKSPACE:
                    env["workspace_bytes"] = 4096 + 16 * len(row.slabs)  # (the device test asks the library)
                yield row, shp, word_bytes, env, A.slab_bytes(row, env)


def test_the_table_has_exactly_the_rows_of_the_aliasing_table():
    assert sorted(F.FILLS) == sorted(row.name for row in A.CASES)
    assert set(F.WORKSPACE) == {row.name for row in A.CASES if "workspace" in row.slabs}
    assert set(F.FORMS) <= set(F.WORKSPACE) and set(F.ORACLE_ROWS) == set(F.FORMS)
    assert set(F.DERIVED) <= set(F.FILLS)


def test_every_slab_has_a_fill_kind():
    kinds = {"q", "all", "qbsk", "t", "seeds", "bytes", "words32", "flags", "acc", "zero", "packed", "out", "workspace"}
    for row in A.CASES:
        fills = F.FILLS[row.name]
        assert list(fills) == list(row.slabs), row.name
        assert set(fills.values()) <= kinds, row.name
        for slab, kind in fills.items():
            assert (kind == "workspace") == (slab == "workspace"), (row.name, slab)
            if kind in F.POISONED:
                assert slab in row.written, (row.name, slab, "a poisoned slab is one the call writes")
            if slab not in row.written:
                assert kind not in F.POISONED, (row.name, slab)


def test_every_workspace_row_names_a_size_function_of_the_header():
    declared = prototypes()
    for row in A.CASES:
        if "workspace" not in row.slabs:
            continue
        function, arguments = F.WORKSPACE[row.name]
        assert function in declared and function.endswith("_workspace_bytes"), (row.name, function)
        parameters = declared[function]
        assert "he_bfv_context" in parameters[0][0], (function, parameters)
        assert len(parameters) == 1 + len(arguments.split()), (function, parameters, arguments)
        assert not any(pointer for _, pointer, _ in parameters[1:]), (function, parameters)
        env = F.environment(row, F.SMALL, ring_moduli(F.SMALL, 8), 8)
        name, values = F.workspace_arguments(row, env)
        assert name == function and all(isinstance(v, int) and v >= 0 for v in values)
        for word_bytes in (8, 4):
            if row.words == "twin" and word_bytes == 4:
                assert (function + "_u32") not in declared  # the twins use the same function (half its bytes)


def test_shapes_are_the_stated_ones():
    assert F.SMALL.degree is None and F.TILED.degree == 4096 and F.TILED.overrides["batch"] == 3
    assert F.TILED.bits == {64: (55, 55, 55, 55), 32: (27, 28, 28, 29)}
    for name, forms in F.FORMS.items():
        row = next(row for row in A.CASES if row.name == name)
        names = [shp.name for shp in F.shapes(row)]
        assert len(set(names)) == len(names), name
        for shp in forms:
            assert shp.why and shp.overrides["L"] <= len(shp.bits[64]) - 1, (name, shp.name)
            if shp.alias is not None:
                written, read = shp.alias
                assert A.may_be_same(row, written, read, shp.overrides), (name, shp.name)
    mul = {shp.name: shp for shp in F.FORMS["he_bfv_mul_device"]}
    parts = mul["N4096-side-lane-floor-in-parts"]
    assert parts.overrides["batch"] * parts.overrides["L"] >= 1024 and parts.overrides["batch"] // 2 >= 256 and 32 not in parts.bits
    assert mul["N4096-row-fused"].setenv == {"HEAMD_BEHZ_FUSED_ABOVE": "0"}
    assert mul["N16384"].overrides["batch"] == 2
    galois = {shp.name: shp for shp in F.FORMS["he_bfv_apply_galois_device"]}
    assert galois["N4096-in-place"].alias == ("out", "ct") and galois["N4096-fused-end"].alias is None


def test_arenas_are_disjoint_aligned_and_guarded():
    count = 0
    for row, shp, word_bytes, env, sizes in every_layout():
        arena = footprint.layout(sizes, row.written)
        what = (row.name, shp.name, word_bytes)
        assert list(arena.offsets) == list(row.slabs), what
        largest = max(sizes[slab] for slab in row.written)
        assert arena.head >= largest and arena.tail >= largest and arena.head >= footprint.MIN_GUARD, what
        at = arena.head
        assert arena.offsets[list(sizes)[0]] == at and at % footprint.ALIGN == 0, what
        previous_end = 0
        for slab, size in sizes.items():
            begin, end = footprint.span(arena, slab)
            assert size > 0 and end - begin == size == arena.sizes[slab], what
            assert begin % footprint.ALIGN == 0 and begin > previous_end, what  # at least one guard byte between two slabs
            previous_end = end
        assert arena.total == previous_end + arena.tail, what
        count += 1
    assert count > 2 * len(A.CASES)


def small_arena():
    row = next(row for row in A.CASES if row.name == "he_bfv_mul_device")
    env = F.environment(row, F.SMALL, ring_moduli(F.SMALL, 8), 8)
    env["workspace_bytes"] = 7 * 5 * 8 * 8 * env["batch"]
    arena = footprint.layout(A.slab_bytes(row, env), row.written)
    filled = np.full(arena.total, footprint.GUARD_BYTE, dtype=np.uint8)
    rng = np.random.default_rng(3)
    for slab in ("lhs", "rhs"):
        filled[slice(*footprint.span(arena, slab))] = rng.integers(0, 256, size=arena.sizes[slab], dtype=np.uint8)
    for slab in arena.written:
        filled[slice(*footprint.span(arena, slab))] = footprint.POISONS[0]
    return arena, filled


def test_the_verifier_passes_when_only_written_slabs_change():
    arena, filled = small_arena()
    image, masked = footprint.expected_image(arena, filled)
    assert image is not filled and masked == [footprint.span(arena, "out"), footprint.span(arena, "workspace")]
    after = filled.copy()
    for slab in arena.written:
        after[slice(*footprint.span(arena, slab))] ^= 0x3C
    footprint.verify(arena, after, image, masked, "every byte of the written slabs")
    footprint.verify(arena, filled, image, masked, "nothing")
    assert footprint.first_difference(arena, after, image, masked) is None


def stray_bytes(arena):
    """(what, arena byte, region, slab, offset) of the single bytes a stray store may hit"""
    out_begin, out_end = footprint.span(arena, "out")
    rhs_begin, rhs_end = footprint.span(arena, "rhs")
    ws_begin, ws_end = footprint.span(arena, "workspace")
    lhs_begin, _ = footprint.span(arena, "lhs")
    return [
        ("just before a slab", out_begin - 1, "padding", "out", -1),
        ("just before the first slab", lhs_begin - 1, "head guard", "lhs", -1),
        ("just after a slab", out_end, "padding", "out", arena.sizes["out"]),
        ("just after a read-only slab", rhs_end, "padding", "rhs", arena.sizes["rhs"]),
        ("inside a read-only slab", rhs_begin + 17, "slab", "rhs", 17),
        ("the last byte of the tail guard", arena.total - 1, "tail guard", "workspace", arena.sizes["workspace"] + arena.tail - 1),
        ("behind the workspace's stated end", ws_end, "tail guard", "workspace", arena.sizes["workspace"]),
        ("a 16-byte lane behind the workspace", ws_end + 15, "tail guard", "workspace", arena.sizes["workspace"] + 15),
        ("the first byte of the arena", 0, "head guard", "lhs", -arena.head),
    ]


def test_the_verifier_names_slab_and_offset_of_a_single_changed_byte():
    arena, filled = small_arena()
    image, masked = footprint.expected_image(arena, filled)
    for what, byte, region, slab, offset in stray_bytes(arena):
        after = filled.copy()
        for written in arena.written:  # the call did its work as well
            after[slice(*footprint.span(arena, written))] ^= 0x3C
        after[byte] ^= 0x01
        assert footprint.first_difference(arena, after, image, masked) == (byte, region, slab, offset), what
        with pytest.raises(AssertionError) as failure:
            footprint.verify(arena, after, image, masked, "probe")
        text = str(failure.value)
        assert "1 byte(s)" in text and "arena byte %d," % byte in text and "%s, %s%+d " % (region, slab, offset) in text, (what, text)


def test_the_verifier_reports_the_first_of_several_bytes():
    arena, filled = small_arena()
    image, masked = footprint.expected_image(arena, filled)
    after = filled.copy()
    end = footprint.span(arena, "workspace")[1]
    after[end: end + 64] = 0  # a row behind the workspace
    assert footprint.first_difference(arena, after, image, masked)[1:] == ("tail guard", "workspace", arena.sizes["workspace"])
    with pytest.raises(AssertionError, match=r"64 byte\(s\)"):
        footprint.verify(arena, after, image, masked, "probe")


def test_locate_splits_padding_between_its_neighbours():
    arena, _ = small_arena()
    names = list(arena.offsets)
    for before, after in zip(names, names[1:]):
        end, following = footprint.span(arena, before)[1], arena.offsets[after]
        assert footprint.locate(arena, end) == ("padding", before, arena.sizes[before])
        assert footprint.locate(arena, following - 1) == ("padding", after, -1)
        assert footprint.locate(arena, following) == ("slab", after, 0)
        assert footprint.locate(arena, end - 1) == ("slab", before, arena.sizes[before] - 1)
