"""fold_mul_signed on the device (both UNIFORM forms, tests/device_probe/fold_signed_probe.hip) against the limb-by-limb
Python model of tests/fold_signed_model.py, word for word, over the edge list of tests/test_fold_signed_bounds.py: the
benchmark's 55-bit primes and the eligibility edges b = 41 / 55 with d = 1 and the largest eligible d; the ends of
[-2^62, 2^62), low words 0 and 0xFFFFFFFF; constants whose second word has the low limb 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF."""
import ctypes
import os
import random

import numpy as np
import pytest

import fold_signed_model as M
from test_fold_signed_bounds import _edges, constants_for, multiplicands

pytestmark = pytest.mark.gpu

PROBE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "device_probe", "libfold_signed_probe.so")


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(PROBE), "tests/device_probe/libfold_signed_probe.so is built by __graft_entry__.build()"
    # PyTorch ships its own HIP runtime: import it first, as heamd.load_library() does, so that the probe binds to that instance
    import torch  # noqa: F401

    lib = ctypes.CDLL(PROBE)
    lib.fold_signed_probe_product.restype = ctypes.c_int
    lib.fold_signed_probe_product.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_size_t, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def moduli():
    import oracle

    return [int(p) for p in oracle.generate_primes([55, 55, 55, 55], False, 8192)] + _edges()


def _run(lib, uniform, p, ys, ws, limbs):
    operand = np.array([y & M.M64 for y in ys], dtype=np.uint64)
    w = np.array(ws, dtype=np.uint64)
    wt = np.array(limbs, dtype=np.uint64)
    out = np.zeros(len(ys), dtype=np.uint64)
    status = lib.fold_signed_probe_product(uniform, p, operand.ctypes.data, w.ctypes.data, wt.ctypes.data, len(ys), out.ctypes.data)
    assert status == 0, status
    return [M.s64(int(v)) for v in out]


def test_gathered_constants_match_the_model(probe, moduli):
    """one lane per (word, constant): every constant of the edge list against every edge word and 64 random ones"""
    for p in moduli:
        c = M.Constants(p)
        ys, ws, limbs = [], [], []
        for w, l in constants_for(p):
            for y in multiplicands(random.Random(p ^ w), 64):
                ys.append(y), ws.append(w), limbs.append(l)
        got = _run(probe, 0, p, ys, ws, limbs)
        want = [M.fold_mul_signed(y, w, l, c) for y, w, l in zip(ys, ws, limbs)]
        wrong = [(p, y, w, g, e) for y, w, g, e in zip(ys, ws, got, want) if g != e]
        assert not wrong, wrong[:4]


def test_uniform_constants_match_the_model(probe, moduli):
    """the constant's words in scalar registers, K in a VGPR pair: one launch per constant, 64 lanes x 5 waves"""
    for p in moduli:
        c = M.Constants(p)
        for w, l in constants_for(p):
            ys = multiplicands(random.Random(p ^ w ^ 1), 300)
            got = _run(probe, 1, p, ys, [w] * len(ys), [l] * len(ys))
            want = [M.fold_mul_signed(y, w, l, c) for y in ys]
            wrong = [(p, y, w, g, e) for y, g, e in zip(ys, got, want) if g != e]
            assert not wrong, wrong[:4]
