"""he_pnns_matrix_shape against tests/pnns_reference.py for the three packings, its error cases, the status of a plaintext
modulus without SIMD encoding, and host-only contexts.  CPU only: no kernel is launched."""
import ctypes

import numpy as np
import pytest

import heamd
import pnns_reference as pnns


def host_context(degree, t_bits=17, word32=False, t=None):
    t = t or heamd.generate_primes([t_bits], True, degree)[0]
    if word32:
        return heamd.BfvContext32(degree, t, heamd.generate_primes([28, 28, 29], False, degree), host_only=True)
    return heamd.BfvContext(degree, t, heamd.generate_primes([40, 40, 41], False, degree), host_only=True)


@pytest.mark.parametrize("degree", [8, 64, 1024, 8192])
def test_plaintext_counts_match_the_restatement(degree):
    ctx = heamd.PnnsContext(host_context(degree))
    rows = sorted({1, 2, 3, degree // 2 - 1, degree // 2, degree - 1, degree, degree + 1, 3 * degree + 5})
    cols = sorted({1, 2, 3, 5, 16, 100, degree // 2 - 1, degree // 2, degree // 2 + 1, degree, 2 * degree + 3})
    checked = 0
    for packing in pnns.PACKINGS:
        for r in rows:
            for c in cols:
                try:
                    expected = pnns.plaintext_count(degree, r, c, packing)
                except ValueError:
                    with pytest.raises(heamd.HeError) as err:
                        ctx.matrix_shape(r, c, packing)
                    assert err.value.name == "invalidArgument", (packing, r, c)
                    continue
                shape = ctx.matrix_shape(r, c, packing)
                assert shape["plaintext_count"] == expected, (packing, r, c)
                assert (shape["baby_step"], shape["giant_step"]) == pnns.baby_step_giant_step(c), (packing, r, c)
                checked += 1
    assert checked > 100


def test_reference_shapes(kats=None):
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnns_plaintext_matrix_kats.json")) as f:
        cases = json.load(f)
    ctx = heamd.PnnsContext(host_context(cases["degree"], t=cases["plaintext_modulus"]))
    for packing in pnns.PACKINGS:
        for case in cases[packing]:
            assert ctx.matrix_shape(case["rows"], case["cols"], packing)["plaintext_count"] == case["plaintext_count"]


def test_baby_steps():
    ctx = heamd.PnnsContext(host_context(8192))
    for cols in range(1, 1025):
        shape = ctx.matrix_shape(10, cols, "diagonal")
        assert (shape["baby_step"], shape["giant_step"]) == pnns.baby_step_giant_step(cols), cols
    for cols, baby_step in ((128, 16), (128, 128), (100, 12), (5, 8), (5, 3), (4096, 64), (1, 1)):
        shape = ctx.matrix_shape(10, cols, "diagonal", baby_step)
        assert (shape["baby_step"], shape["giant_step"]) == pnns.baby_step_giant_step(cols, baby_step)
    for cols, baby_step in ((128, 8), (128, 11), (5, 2), (4096, 63), (2, 1)):  # babyStep < giantStep: the reference traps
        with pytest.raises(ValueError):
            pnns.baby_step_giant_step(cols, baby_step)
        with pytest.raises(heamd.HeError) as err:
            ctx.matrix_shape(10, cols, "diagonal", baby_step)
        assert err.value.name == "invalidArgument"


def test_error_cases_and_null_outs():
    ctx = heamd.PnnsContext(host_context(64))
    for rows, cols, packing in ((0, 4, "diagonal"), (4, 0, "diagonal"), (0, 0, "denseColumn"), (4, 33, "diagonal"),
                                (4, 33, "denseRow"), (4, 4, 3), (4, 4, -1)):
        with pytest.raises(heamd.HeError) as err:
            ctx.matrix_shape(rows, cols, packing)
        assert err.value.name == "invalidArgument", (rows, cols, packing)
    assert ctx.matrix_shape(4, 32, "diagonal")["plaintext_count"] == 32
    assert ctx.matrix_shape(4, 33, "denseColumn")["plaintext_count"] == 3  # no column bound under denseColumn
    lib = heamd.load_library()
    assert lib.he_pnns_matrix_shape(ctx.h, 4, 4, 2, 0, None, None, None) == 0
    count = ctypes.c_size_t()
    assert lib.he_pnns_matrix_shape(ctx.h, 130, 4, 2, 0, ctypes.byref(count), None, None) == 0 and count.value == 12
    assert heamd.binding.STATUS_NAMES[lib.he_pnns_matrix_shape(None, 4, 4, 2, 0, None, None, None)] == "invalidArgument"


def test_plaintext_modulus_without_simd_encoding():
    degree = 64
    q = heamd.generate_primes([40, 40, 41], False, degree)
    bfv = heamd.BfvContext(degree, 65539, q, host_only=True)  # a prime that is not 1 mod 2N
    assert 65539 % (2 * degree) != 1
    with pytest.raises(heamd.HeError) as err:
        heamd.PnnsContext(bfv)
    assert err.value.name == "simdEncodingNotSupported" and err.value.code == 22
    assert heamd.load_library().he_status_string(22) == b"simdEncodingNotSupported"
    # an NTT modulus for a smaller degree only: 1153 = 1 mod 128, not 1 mod 256
    with pytest.raises(heamd.HeError) as err:
        heamd.PnnsContext(heamd.BfvContext(128, 1153, heamd.generate_primes([40, 41], False, 128), host_only=True))
    assert err.value.name == "simdEncodingNotSupported"
    heamd.PnnsContext(heamd.BfvContext(64, 1153, q, host_only=True))


def test_host_only_contexts_and_word_sizes():
    lib = heamd.load_library()
    for word32 in (False,):  # (the ABI has no host-only Bfv<UInt32> context: that pairing is tests/test_gpu_pnns.py's)
        bfv = host_context(64, word32=word32)
        ctx = heamd.PnnsContext(bfv)
        assert ctx.matrix_shape(100, 5)["plaintext_count"] == 16
        entry = lib.he_pnns_diagonal_matrix_device_u32 if word32 else lib.he_pnns_diagonal_matrix_device
        status = entry(ctx.h, ctypes.c_void_p(0x1000), 100, 5, 0, 0, bfv.L, ctypes.c_void_p(0x1000), None, None)
        assert heamd.binding.STATUS_NAMES[status] == "deviceError"
        # argument errors come first, and the other word size is one
        status = entry(ctx.h, ctypes.c_void_p(0x1000), 100, 33, 0, 0, bfv.L, ctypes.c_void_p(0x1000), None, None)
        assert heamd.binding.STATUS_NAMES[status] == "invalidArgument"
        other = lib.he_pnns_diagonal_matrix_device if word32 else lib.he_pnns_diagonal_matrix_device_u32
        status = other(ctx.h, ctypes.c_void_p(0x1000), 100, 5, 0, 0, bfv.L, ctypes.c_void_p(0x1000), None, None)
        assert heamd.binding.STATUS_NAMES[status] == "invalidArgument"
        handle = ctypes.c_void_p()
        create = lib.he_pnns_context_create if word32 else lib.he_pnns_context_create_u32
        assert heamd.binding.STATUS_NAMES[create(bfv.h, ctypes.byref(handle))] == "invalidArgument"
    handle = ctypes.c_void_p()
    assert heamd.binding.STATUS_NAMES[lib.he_pnns_context_create(None, ctypes.byref(handle))] == "invalidArgument"
    assert heamd.binding.STATUS_NAMES[lib.he_pnns_context_create(bfv.h, None)] == "invalidArgument"
    lib.he_pnns_context_destroy(None)
