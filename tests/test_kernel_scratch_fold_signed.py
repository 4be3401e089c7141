"""The headline pair on the signed shift-folded butterflies (ntt_common.hpp kModeFoldSigned, mode 8; N = 8192, two rows per
workgroup) fits the 64 registers of two workgroups per CU without a byte of scratch, like the mode-4 kernels it replaces
(tests/test_kernel_scratch.py); so do the one-row kernels small launches take.  Read from the built object's kernel metadata
(bench_tools/kernel_metadata.py); no GPU involved."""
import os
import re
import subprocess
import sys
import tempfile

import test_kernel_scratch as mechanism

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "swift-homomorphic-encryption_amd", "csrc", "build")
sys.path.insert(0, os.path.join(ROOT, "bench_tools"))


def test_signed_fold_kernels_fit_64_registers_without_scratch():
    import kernel_metadata

    assert mechanism.library_built(), "the library's objects are built by __graft_entry__.build()"
    rows = []
    with tempfile.TemporaryDirectory() as workdir:
        for obj in mechanism.ntt_objects():  # the union of the NTT units (the routing unit alone holds no device code)
            code = kernel_metadata.code_object(os.path.join(BUILD, obj), workdir)
            kernels = list(kernel_metadata.kernels(code)) if code is not None else []
            assert kernels or obj == mechanism.ROUTING_OBJECT, f"{obj}: no kernel read from its code object"
            rows += kernels
    names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True, text=True,
                           check=True).stdout.split("\n")
    found = {kernel_metadata.short_name(name): r for r, name in zip(rows, names)}
    wanted = ["ntt_forward_tiled<13, 10, 8, 0, 2>", "ntt_inverse_tiled<13, 10, 8, 0, 2>",
              "ntt_forward_tiled<13, 10, 8, 0, 1>", "ntt_inverse_tiled<13, 10, 8, 0, 1>"]
    for name in wanted:
        assert name in found, (name, sorted(n for n in found if ", 8, " in n))
        assert found[name]["vgpr"] <= 64 and found[name]["scratch"] == 0 and found[name]["spills"] == 0, (name, found[name])
    # the mode is instantiated for the plain-slab pair at N = 8192 and nowhere else
    assert sorted(n for n in found if re.match(r"ntt_(forward|inverse)_tiled<\d+, \d+, 8,", n)) == sorted(wanted)
