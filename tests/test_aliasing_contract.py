"""The pointer contract of include/he_amd.h, held without a device: tests/aliasing_cases.py says per entry which slabs a call
takes, how many bytes each spans, which it writes and which may be the same memory; here every 8-byte entry of that table is
called on a host-only context with addresses that are no memory.

For every (written slab, other slab) of an entry: the same first byte (unless the table allows it), the written slab beginning
on the other's last byte and ending on its first byte are HE_ERR_INVALID_ARGUMENT with a text that names both arguments;
abutting on either side, and every allowed form, gets as far as the context's HE_ERR_DEVICE -- the arguments were accepted.
Entries without a context (the word-size bridge) would launch on what they accept: only their refusals are called here, the
accepted forms run on memory in tests/test_gpu_aliasing.py.  The table itself is held to the header: every prototype with
two data pointers of which one is written has a row, is deferred, or is known to take host memory.
"""
import os
import re

import pytest

import aliasing_cases as A
import heamd
from heamd.binding import STATUS_NAMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE, GAP = 1 << 32, 1 << 24  # slab i of a call lies at BASE + i GAP: far from one another and from zero


@pytest.fixture(scope="module")
def lib():
    return heamd.load_library()


@pytest.fixture(scope="module")
def contexts():
    """(kind, ring) -> host-only context, with the ring's moduli"""
    made = {}
    for ring, (degree, bits) in A.RINGS.items():
        moduli = heamd.generate_primes(list(bits), False, degree)
        t = heamd.generate_primes([A.PLAINTEXT_BITS], True, degree)[0]
        made["poly", ring] = (heamd.PolyContext(degree, moduli, host_only=True), moduli)
        made["bfv", ring] = (heamd.BfvContext(degree, t, moduli, host_only=True), moduli)
    return made


def call(lib, row, name, handle, env, where):
    """The entry `name` of a row with its slabs at the addresses of `where` -> (status name, last-error text)."""
    status, text = A.invoke(lib, row, name, handle, env, where)
    return STATUS_NAMES[status], text


def layout(sizes):
    return {name: BASE + i * GAP for i, name in enumerate(sizes)}


def variants(row):
    """The parameter sets a row is laid out under: its defaults, and each set under which the table allows an alias."""
    seen = [{}]
    for _, _, need in row.same:
        if need not in seen:
            seen.append(need)
    return seen


@pytest.mark.parametrize("row", A.CASES, ids=lambda row: row.name)
def test_overlaps_are_refused_and_abutting_slabs_accepted(lib, contexts, row):
    handle, moduli = contexts[row.context or "poly", row.ring]
    for overrides in variants(row):
        env = A.environment(row, moduli, 8, overrides)
        sizes = A.slab_bytes(row, env)
        assert all(0 < size < GAP // 2 for size in sizes.values()), sizes
        apart = layout(sizes)
        if row.context is not None:  # slabs apart: the arguments are fine, the host-only context is what stops the call
            assert call(lib, row, row.name, handle.h, env, apart)[0] == "deviceError", (row.name, overrides)
        for written, other in A.pairs(row):
            refused, accepted = A.overlap_positions(apart[other], sizes[other], sizes[written])
            for position, address in refused.items():
                status, text = call(lib, row, row.name, handle.h, env, dict(apart, **{written: address}))
                what = (row.name, overrides, written, other, position)
                if position == "same" and A.may_be_same(row, written, other, overrides):
                    if row.context is not None:
                        assert status == "deviceError", what
                    continue
                assert status == "invalidArgument", what
                assert "overlaps" in text and all(row.says.get(n, n) in text for n in (written, other)), (what, text)
            if row.context is None:
                continue
            for position, address in accepted.items():
                status, text = call(lib, row, row.name, handle.h, env, dict(apart, **{written: address}))
                assert status == "deviceError", (row.name, overrides, written, other, position, text)


@pytest.mark.parametrize("row", [row for row in A.CASES if row.zero is not None], ids=lambda row: row.name)
def test_an_empty_call_overlaps_nothing(lib, contexts, row):
    """every slab at one address and a batch of 0: HE_OK where the entry looks at its batch before its device (the scheme
    entries look at the device first and say so; none calls the arguments invalid)"""
    handle, moduli = contexts[row.context or "poly", row.ring]
    env = A.environment(row, moduli, 8, {row.zero: 0})
    status, text = call(lib, row, row.name, handle.h, env, {name: BASE for name in row.slabs})
    device_first = row.context == "bfv" and row.words != "arg" or row.name.startswith(("he_bfv_secret", "he_bfv_decrypt",
                                                                                        "he_bfv_noise", "he_bfv_is_"))
    assert status == ("deviceError" if device_first else "ok"), (row.name, status, text)


# ---- the table against the header ------------------------------------------------------------------------------------------
HANDLES = ("he_poly_context", "he_bfv_context", "he_pnns_context", "he_simple_pir_context", "he_keyword_pir_table",
           "he_keyword_database", "he_device_group", "he_cuckoo_table_config", "he_keyword_sharding")


def prototypes():
    """name -> [(parameter text, is a data pointer, is const)] for every function the header declares"""
    text = open(os.path.join(ROOT, "include", "he_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    found = {}
    for match in re.finditer(r"\b(he_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        name, parameters = match.group(1), match.group(2)
        rows = []
        for parameter in parameters.split(","):
            parameter = " ".join(parameter.split())
            pointer = "*" in parameter and not any(re.search(r"\b%s\b" % h, parameter) for h in HANDLES)
            rows.append((parameter, pointer, pointer and bool(re.match(r"const\b", parameter))))
        found[name] = rows
    return found


def test_every_entry_with_a_written_and_a_second_slab_is_in_the_table():
    declared = prototypes()
    assert len(declared) > 150 and "he_bfv_mul_device" in declared and "he_poly_add_device_u32" in declared
    rows = {name for row in A.CASES for name in A.entry_names(row)}
    assert len(rows) == sum(len(A.entry_names(row)) for row in A.CASES), "an entry has two rows"
    known = rows | set(A.HOST_OPERAND) | {name + "_u32" for name in A.HOST_OPERAND} | set(A.HOST_ONLY)
    assert known <= set(declared), sorted(known - set(declared))  # the table names nothing the header does not declare
    for name in known:
        assert A.deferred_reason(name) is None, name + " is both listed and deferred"
    missing = []
    for name, parameters in declared.items():
        pointers = [p for p in parameters if p[1]]
        if len(pointers) >= 2 and any(not p[2] for p in pointers) and name not in known and A.deferred_reason(name) is None:
            missing.append(name)
    assert not missing, "entries without a row in tests/aliasing_cases.py: %s" % sorted(missing)
    assert all(reason for reason in list(A.DEFERRED.values()) + list(A.HOST_ONLY.values()) + list(A.HOST_OPERAND.values()))


def test_rows_follow_the_prototypes():
    """a row's arguments are the prototype's, in its order: a slab for a pointer, the context first, the stream last"""
    declared = prototypes()
    for row in A.CASES:
        for name in A.entry_names(row):
            parameters = declared[name]
            expected = len(row.args) + (row.context is not None) + 1
            assert len(parameters) == expected, (name, parameters)
            offset = 1 if row.context is not None else 0
            for token, (text, pointer, const) in zip(row.args, parameters[offset:-1]):
                if token in row.slabs:
                    assert pointer and text.split()[-1].lstrip("*") == token, (name, token, text)
                    assert const == (token not in row.written), (name, token, text)
                elif token.endswith("[]"):
                    assert pointer and text.split()[-1].lstrip("*") == token[:-2], (name, token, text)
                elif token != "None":
                    assert not pointer, (name, token, text)
            assert set(row.written) <= set(row.slabs) and all(a in row.slabs and b in row.slabs for a, b, _ in row.same), name
