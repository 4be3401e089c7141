"""he_simple_pir_batch_response_plan and the batch entries' boundary, without a GPU: the library's plan against its
restatement (tests/simple_pir_batch_plan.py), the fold bound, the override, the argument checks, the ABI, and the matrix
kernels' scratch (read from the built object with the mechanism of tests/test_kernel_scratch.py)."""
import ctypes
import os
import re

import pytest

import heamd
import simple_pir_batch_plan as P
import test_kernel_scratch as mechanism

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("he_simple_pir_compute_response_batch_device", "he_simple_pir_compute_response_batch_device_u32",
           "he_simple_pir_batch_response_plan")
PLAINTEXT_BITS = list(range(1, 17)) + [20, 40]


def _grid():
    for word_bits in (32, 64):
        for pbits in PLAINTEXT_BITS:
            for cbits in range(pbits + 1, word_bits + 1):
                yield pbits, cbits, word_bits


def test_plan_equals_the_restatement(monkeypatch):
    monkeypatch.delenv("HEAMD_SIMPLE_PIR_FOLD_COLUMNS", raising=False)
    seen = set()
    for pbits, cbits, word_bits in _grid():
        ours = heamd.simple_pir_batch_plan(pbits, cbits, 32768, 64, word_bits)
        assert ours == P.plan(pbits, cbits, word_bits), (pbits, cbits, word_bits)
        assert ours["request_limbs"] == -(-cbits // 7) and ours["workspace_bytes"] == 0
        assert ours["matrix_path"] == (1 if pbits <= 7 or 9 <= pbits <= 14 else 0)
        if ours["matrix_path"]:
            assert ours["database_limbs"] == (1 if pbits <= 7 else 2)
            assert ours["requests_per_pass"] in (16, 32)
        seen.add((ours["matrix_path"], ours["database_limbs"], ours["requests_per_pass"], word_bits))
    # both paths, both limb counts and both pass widths occur at both word sizes
    assert len(seen) == 10, seen


def test_fold_bound(monkeypatch):
    monkeypatch.delenv("HEAMD_SIMPLE_PIR_FOLD_COLUMNS", raising=False)
    for pbits, cbits, word_bits in _grid():
        plan = heamd.simple_pir_batch_plan(pbits, cbits, 1, 1, word_bits)
        if not plan["matrix_path"]:
            assert plan["fold_columns"] == 0
            continue
        fold, limbs = plan["fold_columns"], plan["database_limbs"]
        assert fold % P.K_STEP == 0 and fold > 0
        assert fold * limbs * 16129 <= 2**31 - 1
        assert (fold + 64) * limbs * 16129 > 2**31 - 1
    assert heamd.simple_pir_batch_plan(7, 28, 1, 1, 32)["fold_columns"] == 133120
    assert heamd.simple_pir_batch_plan(14, 42, 1, 1, 64)["fold_columns"] == 66560


@pytest.mark.parametrize("forced,one_limb,two_limbs", [
    ("128", 128, 128), ("127", 64, 64), ("1", 64, 64), ("200", 192, 192), ("66560", 66560, 66560), ("66561", 66560, 66560),
    ("100000", 99968, 66560), ("133120", 133120, 66560), ("133184", 133120, 66560), ("4000000000", 133120, 66560),
    ("99999999999999999999999", 133120, 66560), ("0", 133120, 66560), ("", 133120, 66560), ("x", 133120, 66560)])
def test_override_lowers_and_never_raises(monkeypatch, forced, one_limb, two_limbs):
    monkeypatch.setenv("HEAMD_SIMPLE_PIR_FOLD_COLUMNS", forced)
    assert heamd.simple_pir_batch_plan(7, 28, 1, 1, 32)["fold_columns"] == one_limb
    assert heamd.simple_pir_batch_plan(5, 64, 1, 1, 64)["fold_columns"] == one_limb
    assert heamd.simple_pir_batch_plan(14, 42, 1, 1, 64)["fold_columns"] == two_limbs
    assert heamd.simple_pir_batch_plan(9, 32, 1, 1, 32)["fold_columns"] == two_limbs
    assert heamd.simple_pir_batch_plan(20, 42, 1, 1, 64)["fold_columns"] == 0
    if forced.isdigit():
        assert P.plan(7, 28, 32)["fold_columns"] == one_limb and P.plan(14, 42, 64)["fold_columns"] == two_limbs


def test_invalid_arguments_give_the_existing_entrys_errors():
    lib = heamd.load_library()
    for args in ((7, 28, 16), (7, 28, 0), (0, 28, 32), (7, 7, 32), (7, 6, 32), (7, 33, 32), (14, 65, 64), (40, 55, 32)):
        with pytest.raises(heamd.HeError) as err:
            heamd.simple_pir_batch_plan(args[0], args[1], 64, 4, args[2])
        assert err.value.name == "invalidArgument", args
    # the width checks come before anything touches a buffer, as in he_simple_pir_compute_response_device
    for pbits, cbits, suffix in ((0, 28, ""), (7, 7, ""), (7, 65, ""), (7, 33, "_u32"), (30, 20, "_u32")):
        for name in ("he_simple_pir_compute_response_device", "he_simple_pir_compute_response_batch_device"):
            status = getattr(lib, name + suffix)(pbits, cbits, None, 4, 4, None, 1, None, None)
            assert heamd.binding.STATUS_NAMES[status] == "invalidArgument", (name, pbits, cbits)
    for name in ENTRIES[:2]:
        entry = getattr(lib, name)
        assert entry(7, 28, None, 0, 4, None, 1, None, None) == 0      # nothing to do
        assert entry(7, 28, None, 4, 4, None, 0, None, None) == 0
        assert heamd.binding.STATUS_NAMES[entry(7, 28, None, 4, 4, None, 1, None, None)] == "invalidArgument"  # null buffer
        assert b"null buffer" in lib.he_last_error_message()
        status = entry(14, 28, ctypes.c_void_p(0x1001), 4, 4, ctypes.c_void_p(0x1000), 1, ctypes.c_void_p(0x1000), None)
        assert heamd.binding.STATUS_NAMES[status] == "invalidArgument"
        assert b"aligned" in lib.he_last_error_message()


def test_every_out_pointer_may_be_null():
    lib = heamd.load_library()
    assert lib.he_simple_pir_batch_response_plan(7, 28, 32, 100, 3, None, None, None, None, None, None) == 0
    path = ctypes.c_uint32(7)
    assert lib.he_simple_pir_batch_response_plan(8, 28, 32, 100, 3, ctypes.byref(path), None, None, None, None, None) == 0
    assert path.value == 0


def test_entries_are_declared_exported_and_bound():
    lib = heamd.load_library()
    bound = {name for name, _, _ in heamd.binding.SIGNATURES}
    headers = [os.path.join(ROOT, "include", "he_amd.h"),
               os.path.join(ROOT, "swift", "Sources", "CHeAmd", "include", "he_amd.h")]
    for header in headers:
        text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
        for name in ENTRIES:
            assert re.search(r"\bint\s+" + name + r"\s*\(", text), (header, name)
    for name in ENTRIES:
        assert hasattr(lib, name) and name in bound
    assert callable(heamd.simple_pir_batch_plan)
    assert heamd.SimplePirServer32.compute_response_batch is heamd.SimplePirServer.compute_response_batch


def test_batch_entries_fail_loudly_without_a_device():
    try:
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:  # pragma: no cover
        has_gpu = False
    if has_gpu:
        pytest.skip("a GPU is present")
    lib = heamd.load_library()
    fake = ctypes.c_void_p(0x1000)
    # the matrix path and the fallback alike: the launch is refused, nothing is computed on the host instead
    for pbits, cbits, suffix in ((7, 28, "_u32"), (14, 42, ""), (8, 28, "_u32"), (40, 55, "")):
        status = getattr(lib, "he_simple_pir_compute_response_batch_device" + suffix)(pbits, cbits, fake, 16, 64, fake, 2, fake,
                                                                                      None)
        assert heamd.binding.STATUS_NAMES[status] == "deviceError", (pbits, cbits)
        assert lib.he_last_error_message()


def test_matrix_kernels_keep_nothing_in_scratch():
    if not mechanism.library_built():
        pytest.skip("the library's objects are built by __graft_entry__.build()")
    assert os.path.exists(os.path.join(mechanism.BUILD, "simple_pir_matrix_kernels.o"))
    kernels = mechanism._kernels("simple_pir_matrix_kernels.o")
    assert kernels and all(name.startswith("simple_pir_matrix_response_kernel<") for name, _ in kernels), kernels
    # <word, database_limbs, classes, request tiles>: every (word, limbs) pair, every class count the word allows
    found = set()
    for name, _ in kernels:
        word, limbs, classes, tiles = re.match(r"simple_pir_matrix_response_kernel<([^,]+), (\d+)u?, (\d+)u?, (\d+)u?>",
                                               name).groups()
        found.add((8 if "long" in word else 4, int(limbs), int(classes), int(tiles)))
    for word, most in ((4, 5), (8, 10)):
        for limbs in (1, 2):
            assert {c for w, l, c, _ in found if (w, l) == (word, limbs)} == set(range(1, most + 1)), (word, limbs)
            for classes in range(1, most + 1):
                tiles = {t for w, l, c, t in found if (w, l, c) == (word, limbs, classes)}
                assert tiles == ({1, 2} if classes <= (4 if word == 4 else 6) else {1}), (word, limbs, classes)
    offenders = [(name, scratch) for name, scratch in kernels if scratch != 0]
    assert not offenders, offenders
