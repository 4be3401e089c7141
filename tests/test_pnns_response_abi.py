"""he_pnns_mul_transpose_device / he_pnns_compute_response_device and their UInt32 twins without a device: the symbols are
declared, exported and mirrored in Python, and every argument error is returned before anything is enqueued (host-only
contexts: a call that passes validation ends in deviceError)."""
import ctypes
import os
import re
import subprocess

import pytest

import heamd
import pnns_reference as pnns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["he_pnns_mul_transpose_device", "he_pnns_mul_transpose_device_u32", "he_pnns_compute_response_device",
           "he_pnns_compute_response_device_u32"]
DUMMY = ctypes.c_void_p(0x1000)  # 16-byte aligned, never dereferenced: no call here gets as far as the device


def host_context(degree=64):
    t = heamd.generate_primes([17], True, degree)[0]
    return heamd.BfvContext(degree, t, heamd.generate_primes([40, 40, 41], False, degree), host_only=True)


def declared_functions():
    text = open(os.path.join(ROOT, "include", "he_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(he_[a-z0-9_]+)\s*\(", text))


def test_new_entries_are_declared_exported_and_mirrored():
    lib = heamd.load_library()
    declared = declared_functions()
    out = subprocess.run(["nm", "-D", "--defined-only", heamd.binding.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ENTRIES:
        assert name in declared and name in exported and hasattr(lib, name), name
    assert declared == exported, (sorted(declared - exported), sorted(exported - declared))
    assert callable(heamd.PnnsContext.mul_transpose) and callable(heamd.PnnsContext.compute_response)
    with open(os.path.join(ROOT, "include", "he_amd.h")) as ours, \
            open(os.path.join(ROOT, "swift", "Sources", "CHeAmd", "include", "he_amd.h")) as copy:
        assert ours.read() == copy.read()


def call(lib, name, ctx, plaintext_count, rows, cols, baby_step, queries, keys, matrix=DUMMY, query=DUMMY, out=DUMMY):
    return heamd.binding.STATUS_NAMES[getattr(lib, name)(ctx.h, matrix, plaintext_count, rows, cols, baby_step, query,
                                                         queries, keys, out, None)]


@pytest.mark.parametrize("name", ["he_pnns_mul_transpose_device", "he_pnns_compute_response_device"])
def test_argument_errors_need_no_device(name):
    lib = heamd.load_library()
    bfv = host_context()
    ctx = heamd.PnnsContext(bfv)
    pair = (ctypes.c_void_p * 2)(0x2000, 0x3000)
    # 50 x 16 at N = 64: P = 16, C = 1, default baby step 4, G = 4
    assert call(lib, name, ctx, 16, 50, 16, 4, 1, pair) == "deviceError"  # valid: only the device is missing
    assert heamd.binding.STATUS_NAMES[getattr(lib, name)(None, DUMMY, 16, 50, 16, 4, DUMMY, 1, pair, DUMMY, None)] == \
        "invalidArgument"
    assert call(lib, name, ctx, 16, 50, 16, 0, 1, pair) == "invalidArgument"   # baby_step 0: the packing carries it
    assert call(lib, name, ctx, 16, 50, 16, 3, 1, pair) == "invalidArgument"   # babyStep < giantStep (3 < 6)
    assert call(lib, name, ctx, 16, 0, 16, 4, 1, pair) == "invalidArgument"    # invalidMatrixDimensions
    assert call(lib, name, ctx, 16, 50, 0, 4, 1, pair) == "invalidArgument"
    assert call(lib, name, ctx, 64, 50, 33, 8, 1, pair) == "invalidArgument"   # cols above N / 2
    # cols not matching the matrix: 50 x 32 would be 32 plaintexts, 50 x 8 eight, 150 x 16 forty-eight
    assert call(lib, name, ctx, 16, 50, 32, 6, 1, pair) == "invalidArgument"
    assert call(lib, name, ctx, 16, 50, 8, 4, 1, pair) == "invalidArgument"
    assert call(lib, name, ctx, 16, 150, 16, 4, 1, pair) == "invalidArgument"
    assert call(lib, name, ctx, 48, 150, 16, 4, 1, pair) == "deviceError"
    # Q = 0: an empty batch is answered with nothing, once the shape has been checked
    assert call(lib, name, ctx, 16, 50, 16, 4, 0, None, query=None, out=None) == "ok"
    assert call(lib, name, ctx, 16, 50, 16, 0, 0, None) == "invalidArgument"
    # keys: both needed here (baby_step 4 > 1, G = 4 > 1)
    assert call(lib, name, ctx, 16, 50, 16, 4, 1, None) == "missingGaloisKey"
    assert call(lib, name, ctx, 16, 50, 16, 4, 1, (ctypes.c_void_p * 2)(None, 0x3000)) == "missingGaloisKey"
    assert call(lib, name, ctx, 16, 50, 16, 4, 1, (ctypes.c_void_p * 2)(0x2000, None)) == "missingGaloisKey"
    two = (ctypes.c_void_p * 4)(0x2000, 0x3000, 0x2000, None)
    assert call(lib, name, ctx, 16, 50, 16, 4, 2, two) == "missingGaloisKey"   # the second query's
    # G = 1 (baby_step = P): the key of -baby_step is not needed; baby_step = 1 (cols = 1): neither is
    assert call(lib, name, ctx, 16, 50, 16, 16, 1, (ctypes.c_void_p * 2)(0x2000, None)) == "deviceError"
    assert call(lib, name, ctx, 16, 50, 16, 16, 1, (ctypes.c_void_p * 2)(None, 0x3000)) == "missingGaloisKey"
    assert call(lib, name, ctx, 1, 50, 1, 1, 1, None) == "deviceError"
    # null and misaligned buffers
    assert call(lib, name, ctx, 16, 50, 16, 4, 1, pair, matrix=None) == "invalidArgument"
    assert call(lib, name, ctx, 16, 50, 16, 4, 1, pair, query=None) == "invalidArgument"
    assert call(lib, name, ctx, 16, 50, 16, 4, 1, pair, out=None) == "invalidArgument"
    assert call(lib, name, ctx, 16, 50, 16, 4, 1, pair, matrix=ctypes.c_void_p(0x1008)) == "invalidArgument"
    # the other word size
    assert call(lib, name + "_u32", ctx, 16, 50, 16, 4, 1, pair) == "invalidArgument"
    assert lib.he_last_error_message()


def test_giant_steps_always_cover_the_padded_columns():
    """G is ceil(P / baby_step) by construction (BabyStepGiantStep.init), so G b < P cannot be handed to the entry: every
    baby step it accepts covers P, and one below the giant step is refused."""
    ctx = heamd.PnnsContext(host_context(8192))
    lib = heamd.load_library()
    pair = (ctypes.c_void_p * 2)(0x2000, 0x3000)
    for cols in (1, 2, 3, 5, 16, 100, 128, 1000, 4096):
        padded = pnns.next_power_of_two(cols)
        for baby_step in range(1, min(padded, 70) + 1):
            try:
                _, giant = pnns.baby_step_giant_step(cols, baby_step)
            except ValueError:
                assert call(lib, "he_pnns_mul_transpose_device", ctx, padded, 10, cols, baby_step, 1, pair) == "invalidArgument"
                continue
            shape = ctx.matrix_shape(10, cols, "diagonal", baby_step)
            assert shape["giant_step"] == giant and giant * baby_step >= padded > (giant - 1) * baby_step
            assert call(lib, "he_pnns_mul_transpose_device", ctx, padded, 10, cols, baby_step, 1, pair) == "deviceError"
