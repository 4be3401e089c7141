"""The SimplePIR client entries (he_simple_pir_client_plan, he_simple_pir_client_workspace_bytes and the six device entries)
without a device: declared in both headers with the prototypes the binding mirrors, exported, no _u32 twins; the plan against
tests/simple_pir_client_reference.py on a host-only build, with every error it returns; and of the device entries what can be said
without a context -- a he_simple_pir_context needs a device, so the errors behind a valid context (the other word size, the
standard deviation, the workspace, the hint's alignment, batch 0) are checked in tests/test_gpu_simple_pir_client.py."""
import ctypes
import os
import subprocess

import heamd
import simple_pir_client_cases as cases
import simple_pir_client_reference as C
from test_aliasing_contract import prototypes
from test_pnns_client_abi import name_of, slab
from test_pnns_response_abi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_ENTRIES = ["he_simple_pir_a_polynomials_device", "he_simple_pir_encrypt_zero_device",
                  "he_simple_pir_secret_times_hint_device", "he_simple_pir_precompute_queries_device",
                  "he_simple_pir_add_indices_device", "he_simple_pir_decrypt_responses_device"]
ENTRIES = ["he_simple_pir_client_plan", "he_simple_pir_client_workspace_bytes"] + DEVICE_ENTRIES


def test_entries_are_declared_exported_and_mirrored():
    lib = heamd.load_library()
    declared, parameters = declared_functions(), prototypes()
    out = subprocess.run(["nm", "-D", "--defined-only", heamd.binding.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    signatures = {name: argtypes for name, _, argtypes in heamd.binding.SIGNATURES}
    for name in ENTRIES:
        assert name in declared and name in exported and hasattr(lib, name), name
        assert not hasattr(lib, name + "_u32") and name + "_u32" not in declared, name  # the word is an argument
        assert len(parameters[name]) == len(signatures[name]), name
        for (text, pointer, _), argtype in zip(parameters[name], signatures[name]):
            is_pointer = argtype is ctypes.c_void_p or hasattr(argtype, "contents")
            assert is_pointer == ("*" in text or text.startswith("he_stream")), (name, text, argtype)
    for name in DEVICE_ENTRIES:
        first, second = parameters[name][0][0], parameters[name][1][0]
        assert first == "const he_simple_pir_context* ctx" and second == "uint32_t word_bits", name
        assert parameters[name][-1][0] == "he_stream s", name
    for method in ("a_polynomials", "precompute", "add_indices", "decrypt", "encrypt_zero", "secret_times_hint", "plan",
                   "workspace_bytes"):
        assert callable(getattr(heamd.SimplePirClient, method))
    with open(os.path.join(ROOT, "include", "he_amd.h")) as ours, \
            open(os.path.join(ROOT, "swift", "Sources", "CHeAmd", "include", "he_amd.h")) as copy:
        assert ours.read() == copy.read()


def test_plan_on_a_host_only_build():
    import oracle

    for name, shape in cases.SHAPES.items():
        params = cases.params_of(oracle, name)
        for std_dev in cases.STD_DEVS:
            for batch in (0, 1, 3, 128):
                got = heamd.simple_pir_client_plan(shape[2], shape[3], shape[4], shape[0], shape[1], std_dev, batch, shape[5])
                assert got == C.plan(params, std_dev, batch, shape[5]), (name, std_dev, batch)
    bench = heamd.simple_pir_client_plan(14, 42, 1024, 32768, 32768 * 14 // 8, "stdDev64", 128)
    assert bench["query_words"] == 32768 and bench["row_block"] == 128 and bench["error_stream_bytes"] == 32
    assert bench["secret_rows_per_pass"] == 16 and bench["fold_terms"] >= (1 << 21)


def test_plan_row_block_override(monkeypatch):
    import oracle

    params = cases.params_of(oracle, "ref-large-u32")
    shape = cases.SHAPES["ref-large-u32"]
    for forced in ("1", "2", "1000000", "0", "x"):
        monkeypatch.setenv("HEAMD_SIMPLE_PIR_CLIENT_ROW_BLOCK", forced)
        got = heamd.simple_pir_client_plan(shape[2], shape[3], shape[4], shape[0], shape[1], "stdDev32", 3, shape[5])
        wanted = int(forced) if forced.isdigit() else 0
        assert got == C.plan(params, "stdDev32", 3, shape[5], wanted), forced
        assert got["row_block"] == (wanted if wanted in (1, 2) else 15)  # lowered, never raised: 3 queries of 5 chunks


def test_plan_errors():
    lib = heamd.load_library()

    def plan(pbits=14, cbits=42, n=1024, bits=64, count=600, size=20, std_dev=0, batch=1):
        return name_of(lib.he_simple_pir_client_plan(pbits, cbits, n, bits, count, size, std_dev, batch, *[None] * 13))

    assert plan() == "ok"  # every out pointer may be NULL, and no device is needed
    # he_simple_pir_shape's
    assert plan(bits=16) == "invalidArgument" and plan(pbits=0) == "invalidArgument" and plan(cbits=14) == "invalidArgument"
    assert plan(cbits=61) == "invalidArgument" and plan(bits=32, cbits=30, pbits=7) == "invalidArgument"
    assert plan(n=1000) == "invalidArgument" and plan(count=0) == "invalidArgument" and plan(size=0) == "invalidArgument"
    # the client's own
    assert plan(std_dev=2) == "invalidArgument" and plan(std_dev=-1) == "invalidArgument"
    assert plan(std_dev=1) == "ok"
    assert plan(batch=0) == "ok" and plan(batch=1 << 20) == "ok" and plan(batch=(1 << 20) + 1) == "invalidArgument"
    assert plan(std_dev=2, bits=16) == "invalidArgument"
    assert lib.he_last_error_message()


def test_device_entries_without_a_context():
    lib = heamd.load_library()
    calls = {
        "he_simple_pir_a_polynomials_device": lambda ctx, bits: lib.he_simple_pir_a_polynomials_device(
            ctx, bits, slab(0), slab(1), slab(2), 1 << 20, None),
        "he_simple_pir_encrypt_zero_device": lambda ctx, bits: lib.he_simple_pir_encrypt_zero_device(
            ctx, bits, 0, slab(0), slab(1), slab(2), slab(3), 1, slab(4), 1 << 20, None),
        "he_simple_pir_secret_times_hint_device": lambda ctx, bits: lib.he_simple_pir_secret_times_hint_device(
            ctx, bits, slab(0), 1, slab(1), 5, slab(2), slab(3), 1 << 20, None),
        "he_simple_pir_precompute_queries_device": lambda ctx, bits: lib.he_simple_pir_precompute_queries_device(
            ctx, bits, 0, slab(0), slab(1), slab(2), slab(3), slab(4), slab(5), 1, slab(6), 1 << 20, None),
        "he_simple_pir_add_indices_device": lambda ctx, bits: lib.he_simple_pir_add_indices_device(
            ctx, bits, slab(0), slab(1), slab(2), 1, None),
        "he_simple_pir_decrypt_responses_device": lambda ctx, bits: lib.he_simple_pir_decrypt_responses_device(
            ctx, bits, slab(0), slab(1), slab(2), slab(3), slab(4), 1, slab(5), 1 << 20, None),
    }
    assert sorted(calls) == sorted(DEVICE_ENTRIES)
    for name, call in calls.items():
        assert name_of(call(None, 64)) == "invalidArgument", name  # a null context
        assert name_of(call(None, 16)) == "invalidArgument", name  # the word comes first
        assert b"word_bits" in lib.he_last_error_message(), name
    for operation in range(6):
        assert lib.he_simple_pir_client_workspace_bytes(None, operation, 0, 1) == 0
