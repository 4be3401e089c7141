"""he_pnns_query_matrix_shape and the several-rows response entries without a device: the symbols are declared in both headers,
exported and mirrored in Python; the shape entry equals tests/pnns_matrix_reference.py's counts and needs over a sweep; every
argument error of the response entries is returned before anything is enqueued (host-only context: a call that passes
validation ends in deviceError)."""
import ctypes
import os
import subprocess

import pytest

import heamd
import pnns_matrix_reference as pm
import pnns_reference as pnns
from test_pnns_response_abi import DUMMY, declared_functions, host_context

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["he_pnns_query_matrix_shape", "he_pnns_mul_transpose_matrix_device", "he_pnns_mul_transpose_matrix_device_u32",
           "he_pnns_compute_response_matrix_device", "he_pnns_compute_response_matrix_device_u32"]


def test_new_entries_are_declared_exported_and_mirrored():
    lib = heamd.load_library()
    declared = declared_functions()
    out = subprocess.run(["nm", "-D", "--defined-only", heamd.binding.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ENTRIES:
        assert name in declared and name in exported and hasattr(lib, name), name
    for name in ("query_matrix_shape", "mul_transpose_matrix", "compute_response_matrix"):
        assert callable(getattr(heamd.PnnsContext, name))
    with open(os.path.join(ROOT, "include", "he_amd.h")) as ours, \
            open(os.path.join(ROOT, "swift", "Sources", "CHeAmd", "include", "he_amd.h")) as copy:
        text = ours.read()
        assert text == copy.read()
    assert "he_pnns_pack_step" in text


@pytest.mark.parametrize("degree", [16, 64])
def test_shape_equals_the_restatement(degree):
    ctx = heamd.PnnsContext(host_context(degree))
    for rows in (1, 3, degree // 4, degree // 2, degree // 2 + 1, degree + 6):
        for cols in range(1, degree // 2 + 1):
            for row_count in (1, 2, 3, 5, 8, 20, 40):
                shape = ctx.query_matrix_shape(rows, cols, row_count)
                label = (degree, rows, cols, row_count)
                assert shape["query_ciphertexts"] == pnns.plaintext_count(degree, row_count, cols, "denseRow"), label
                assert shape["result_ciphertexts"] == pm.result_ciphertext_count(degree, rows, row_count), label
                assert shape["needs"] == pm.needs(degree, rows, cols, row_count), label


def test_shape_errors():
    ctx = heamd.PnnsContext(host_context(64))
    lib = heamd.load_library()
    for args in ((10, 33, 3), (0, 4, 3), (10, 0, 3), (10, 4, 0)):
        with pytest.raises(heamd.HeError) as err:
            ctx.query_matrix_shape(*args)
        assert err.value.name == "invalidArgument", args
    assert heamd.binding.STATUS_NAMES[lib.he_pnns_query_matrix_shape(None, 10, 4, 3, None, None, None)] == "invalidArgument"
    assert heamd.binding.STATUS_NAMES[lib.he_pnns_query_matrix_shape(ctx.h, 10, 4, 3, None, None, None)] == "ok"


def plan_of(*pairs):
    plan = (heamd.binding.PnnsPackStep * max(len(pairs), 1))()
    for i, (step, count) in enumerate(pairs):
        plan[i].step, plan[i].count = step, count
    return plan


def keys_of(*pointers):
    return (ctypes.c_void_p * len(pointers))(*pointers)


@pytest.mark.parametrize("name", ["he_pnns_mul_transpose_matrix_device", "he_pnns_compute_response_matrix_device"])
def test_argument_errors_need_no_device(name):
    lib = heamd.load_library()
    ctx = heamd.PnnsContext(host_context())

    def call(rows=10, cols=4, baby_step=2, query_rows=5, queries=1, plan=((10, 1),), keys=(1, 1, 1, 1, 1), count=4, ctx_h=ctx.h,
             matrix=DUMMY, query=DUMMY, out=DUMMY, entry=name):
        pointers = None if keys is None else keys_of(*[0x2000 if k else None for k in keys])
        return heamd.binding.STATUS_NAMES[getattr(lib, entry)(ctx_h, matrix, count, rows, cols, baby_step, query, query_rows,
                                                              queries, plan_of(*plan) if plan else None, len(plan), pointers,
                                                              out, None)]

    # 10 x 4 at N = 64: P = 4, baby step 2, G = 2, cps = 3; R = 5 needs every slot and the plan
    assert call() == "deviceError"  # valid: only the device is missing
    assert call(ctx_h=None) == "invalidArgument"
    assert call(baby_step=0) == "invalidArgument"
    assert call(rows=0) == "invalidArgument"
    assert call(cols=33, count=64, baby_step=8) == "invalidArgument"  # cols above N / 2
    assert call(count=8) == "invalidArgument"                          # not P C plaintexts
    assert call(query_rows=0) == "invalidArgument"
    assert call(queries=0, keys=None, query=None, out=None) == "ok"
    assert call(query_rows=0, queries=0) == "invalidArgument"          # the shape is checked first
    assert call(entry=name + "_u32") == "invalidArgument"              # the other word size
    # the plan: not rows mod N / 2, a step outside [1, N / 2 - 1], none at all
    assert call(plan=((9, 1),)) == "invalidArgument"
    assert call(plan=((32, 1), (10, 1)), keys=(1,) * 6) == "invalidArgument"
    assert call(plan=((0, 5), (10, 1)), keys=(1,) * 6) == "invalidArgument"
    assert call(plan=(), keys=(1,) * 4) == "invalidArgument"
    assert call(plan=((8, 1), (2, 1)), keys=(1,) * 6) == "deviceError"
    assert call(plan=((21, 2),)) == "deviceError"                      # 42 = 10 mod 32
    # keys: each needed slot
    assert call(keys=None) == "missingGaloisKey"
    for slot in range(5):
        assert call(keys=tuple(int(k != slot) for k in range(5))) == "missingGaloisKey", slot
    assert call(queries=2, keys=(1,) * 9 + (0,)) == "missingGaloisKey"  # the second client's
    # keys a shape does not need are not read: R = 1 (slots 2, 3, plan), cps = 1 (plan), cps = 0, P = N / 2 (slot 3)
    assert call(query_rows=1, plan=(), keys=(1, 1, 0, 0)) == "deviceError"
    assert call(query_rows=1, keys=(1, 1, 0, 0, 0)) == "deviceError"   # a plan that is not read does not move the slots
    assert call(query_rows=1, plan=(), keys=(0, 1, 0, 0)) == "missingGaloisKey"
    assert call(rows=32, query_rows=3, plan=(), keys=(1, 1, 1, 1)) == "deviceError"
    assert call(rows=32, query_rows=3, plan=(), keys=(1, 1, 0, 1)) == "missingGaloisKey"
    assert call(rows=70, count=8, query_rows=3, plan=(), keys=(1, 1, 1, 1)) == "deviceError"
    assert call(cols=32, count=32, baby_step=6, query_rows=3, keys=(1, 1, 1, 0, 1)) == "deviceError"
    assert call(cols=32, count=32, baby_step=6, query_rows=3, keys=(1, 1, 1, 0, 0)) == "missingGaloisKey"
    # null and misaligned buffers
    assert call(matrix=None) == "invalidArgument"
    assert call(query=None) == "invalidArgument"
    assert call(out=None) == "invalidArgument"
    assert call(matrix=ctypes.c_void_p(0x1008)) == "invalidArgument"
    assert lib.he_last_error_message()
