"""The wire format at both ends of a server path, timed on the device.  One JSON line, also written to --out:

    python bench_tools/ciphertext_wire_bench.py [--lib PATH/libhe_amd.so] [--composition] [--windows 7] [--out FILE]

Shapes:
  replies-u64   256 reply ciphertexts, N = 8192, one 55-bit modulus, skips [22, 13], 8-byte words   -> records
  replies-u32   256 reply ciphertexts, N = 4096, one 27-bit modulus, skips [11, 3], 4-byte words    -> records
  key           28 seeded Eval ciphertexts, N = 4096, three moduli (27, 28, 28 bits), 8-byte words  <- poly0 bytes + seeds
  query         2 seeded Coeff ciphertexts, N = 4096, two moduli (27, 28 bits), 8-byte words        <- poly0 bytes + seeds

Default: the ciphertext-level entries (he_ciphertexts_serialize_device(_u32), he_ciphertexts_deserialize_seeded_device), one
call per shape.  --composition: the same work from the polynomial-level entries alone -- per reply ciphertext two
he_poly_serialize_device calls (4-byte words: one he_words_widen_u32_device of the whole batch first, the library having no
4-byte wire entry before), per seeded ciphertext one he_poly_deserialize_device, one he_poly_random_from_seeds_device and, in
Coeff, one he_ntt_inverse_device; the 2-byte headers are not written (in the composition's favour).  --composition uses only
entries an older build of the library has, so --lib may name one: that is the yardstick.  Without --composition the tool
also checks, untimed, that the composition on the same inputs gives the same bytes and words.

Timing: the library is driven through ctypes directly (no binding: an older library lacks its newer symbols).  A window is
`reps` back-to-back calls between two host clock reads, the second after a device synchronise; reps is sized so that a window
lasts about 0.25 s; --windows windows per shape after one warm-up window; the median, the smallest and the largest are
reported.  bytes = words read + record bytes written (or the reverse), rate = bytes / median.  The copy rate the rates are
set against is measured in the same run, the way bench.py measures the one it prints: the library's own streaming copy
(he_words_copy_device, non-temporal) of a 1 GiB slab, read + written bytes over the best of the windows; every shape reports
its fraction of it, and the JSON names the source."""
import argparse
import ctypes
import json
import os
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "swift-homomorphic-encryption_amd", "lib", "libhe_amd.so")
vp, c_size, c_int, c_u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
INT_P = ctypes.POINTER(ctypes.c_int)

SIGNATURES = {
    "he_poly_context_create": (c_int, [c_u32, ctypes.POINTER(ctypes.c_uint64), c_u32, ctypes.POINTER(vp)]),
    "he_poly_serialization_byte_count": (c_size, [vp, c_int]),
    "he_poly_serialize_device": (c_int, [vp, vp, c_size, c_int, vp, vp]),
    "he_poly_deserialize_device": (c_int, [vp, vp, c_size, c_size, c_int, vp, vp]),
    "he_poly_random_from_seeds_device": (c_int, [vp, vp, c_size, vp, vp]),
    "he_ntt_inverse_device": (c_int, [vp, vp, c_size, vp]),
    "he_words_widen_u32_device": (c_int, [vp, vp, c_size, vp]),
    "he_words_copy_device": (c_int, [vp, vp, c_size, c_int, vp]),
}
NEW_SIGNATURES = {
    "he_ciphertexts_serialization_byte_count": (c_size, [vp, c_u32, INT_P]),
    "he_ciphertexts_serialize_device": (c_int, [vp, vp, c_size, c_u32, INT_P, vp, c_size, vp]),
    "he_ciphertexts_serialize_device_u32": (c_int, [vp, vp, c_size, c_u32, INT_P, vp, c_size, vp]),
    "he_ciphertexts_deserialize_seeded_device": (c_int, [vp, vp, c_size, vp, c_size, c_int, vp, vp]),
}

# the reference's n_8192_logq_3x55 and n_4096_logq_27_28_28 coefficient moduli (EncryptionParameters.swift)
Q55 = (1 << 55) - 311295
Q27_28_28 = [(1 << 27) - 40959, (1 << 28) - 65535, (1 << 28) - 73727]


def load(path, names):
    lib = ctypes.CDLL(path)
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = {**SIGNATURES, **NEW_SIGNATURES}[name]
    return lib


def check(status, what):
    if status != 0:
        raise RuntimeError(f"{what}: status {status}")


def context(lib, degree, moduli):
    handle = vp()
    array = (ctypes.c_uint64 * len(moduli))(*moduli)
    check(lib.he_poly_context_create(degree, array, len(moduli), ctypes.byref(handle)), "he_poly_context_create")
    return handle


def ptr(tensor, offset_bytes=0):
    return vp(tensor.data_ptr() + offset_bytes)


def windows(torch, call, count):
    """median / min / max seconds per call over `count` windows of about 0.25 s each"""
    call()
    torch.cuda.synchronize()
    start = time.perf_counter()
    call()
    torch.cuda.synchronize()
    once = max(time.perf_counter() - start, 1e-6)
    reps = max(3, min(20000, int(0.25 / once)))
    times = []
    for window in range(count + 1):
        torch.cuda.synchronize()
        start = time.perf_counter()
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
        if window:  # the first window is the warm-up
            times.append((time.perf_counter() - start) / reps)
    return {"median_us": 1e6 * float(np.median(times)), "min_us": 1e6 * min(times), "max_us": 1e6 * max(times), "reps": reps}


def copy_rate(torch, lib, window_count):
    """GB/s read + written by he_words_copy_device (non-temporal) over a 1 GiB slab: bench.py's copy_rate"""
    words = 1 << 27
    source = torch.zeros(words, dtype=torch.int64, device="cuda")
    target = torch.empty_like(source)
    result = windows(torch, lambda: check(lib.he_words_copy_device(ptr(source), ptr(target), words, 1, None), "copy"),
                     window_count)
    return 2 * words * 8 / result["min_us"] / 1e3


def replies(torch, lib, composition, word_bits, degree, modulus, skips, count, window_count, verify):
    ctx = context(lib, degree, [modulus])
    generator = torch.Generator("cuda").manual_seed(degree + word_bits)
    wide = torch.randint(0, modulus, (count, 2, 1, degree), dtype=torch.int64, device="cuda", generator=generator)
    cts = wide if word_bits == 64 else wide.to(torch.int32)
    sizes = [lib.he_poly_serialization_byte_count(ctx, s) for s in skips]
    record = 2 + sum(sizes)
    out = torch.zeros(count * record, dtype=torch.uint8, device="cuda")
    skip_array = (ctypes.c_int * 2)(*skips)
    widened = torch.empty_like(wide) if word_bits == 32 else None

    def composed():
        source = cts
        if word_bits == 32:
            check(lib.he_words_widen_u32_device(ptr(cts), ptr(widened), cts.numel(), None), "widen")
            source = widened
        for i in range(count):
            base = i * record + 2
            check(lib.he_poly_serialize_device(ctx, ptr(source, (2 * i) * degree * 8), 1, skips[0], ptr(out, base), None), "poly0")
            check(lib.he_poly_serialize_device(ctx, ptr(source, (2 * i + 1) * degree * 8), 1, skips[1], ptr(out, base + sizes[0]),
                                               None), "poly1")

    def whole():
        fn = lib.he_ciphertexts_serialize_device_u32 if word_bits == 32 else lib.he_ciphertexts_serialize_device
        check(fn(ctx, ptr(cts), count, 2, skip_array, ptr(out), record, None), "he_ciphertexts_serialize_device")

    if verify:
        composed()
        theirs = out.clone().view(count, record)[:, 2:]
        out.zero_()
        whole()
        mine = out.view(count, record)
        assert torch.equal(mine[:, 2:], theirs) and bool((mine[:, 0] == 2).all()) and bool((mine[:, 1] == 0).all())
    result = windows(torch, composed if composition else whole, window_count)
    moved = cts.numel() * (word_bits // 8) + count * record
    result.update(bytes=moved, gbps=moved / result["median_us"] / 1e3, launches=(2 * count + (word_bits == 32)) if composition else 1)
    return result


def seeded(torch, lib, composition, degree, moduli, count, coeff_format, window_count, verify):
    ctx = context(lib, degree, moduli)
    record = lib.he_poly_serialization_byte_count(ctx, 0)
    generator = torch.Generator("cuda").manual_seed(count)
    poly0 = torch.randint(0, 256, (count * record,), dtype=torch.uint8, device="cuda", generator=generator)
    seeds = torch.randint(0, 256, (count * 32,), dtype=torch.uint8, device="cuda", generator=generator)
    rows = len(moduli)
    cts = torch.zeros((count, 2, rows, degree), dtype=torch.int64, device="cuda")
    poly_bytes = rows * degree * 8

    def composed():
        for i in range(count):
            check(lib.he_poly_deserialize_device(ctx, ptr(poly0, i * record), record, 1, 0, ptr(cts, 2 * i * poly_bytes), None),
                  "deserialize")
            check(lib.he_poly_random_from_seeds_device(ctx, ptr(seeds, 32 * i), 1, ptr(cts, (2 * i + 1) * poly_bytes), None),
                  "sampler")
            if coeff_format:
                check(lib.he_ntt_inverse_device(ctx, ptr(cts, (2 * i + 1) * poly_bytes), 1, None), "inverse NTT")

    def whole():
        check(lib.he_ciphertexts_deserialize_seeded_device(ctx, ptr(poly0), record, ptr(seeds), count, coeff_format, ptr(cts),
                                                           None), "he_ciphertexts_deserialize_seeded_device")

    if verify:
        composed()
        theirs = cts.clone()
        cts.zero_()
        whole()
        assert torch.equal(cts, theirs)
    result = windows(torch, composed if composition else whole, window_count)
    moved = count * (record + 32) + cts.numel() * 8
    per = 3 + (1 if coeff_format else 0)  # deserialize, the sampler's two kernels, the transform
    result.update(bytes=moved, gbps=moved / result["median_us"] / 1e3,
                  launches=count * per if composition else 3 + (count if coeff_format else 0))
    return result


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--lib", default=DEFAULT_LIB)
    parser.add_argument("--composition", action="store_true")
    parser.add_argument("--windows", type=int, default=7)
    parser.add_argument("--count-scale", type=float, default=1.0, help="scale the ciphertext counts (rehearsals)")
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    import torch

    names = list(SIGNATURES) if args.composition else list(SIGNATURES) + list(NEW_SIGNATURES)
    lib = load(args.lib, names)
    verify = not args.composition
    scale = lambda n: max(1, int(n * args.count_scale))  # noqa: E731
    shapes = {
        "replies-u64": replies(torch, lib, args.composition, 64, 8192, Q55, [22, 13], scale(256), args.windows, verify),
        "replies-u32": replies(torch, lib, args.composition, 32, 4096, Q27_28_28[0], [11, 3], scale(256), args.windows, verify),
        "key": seeded(torch, lib, args.composition, 4096, Q27_28_28, scale(28), 0, args.windows, verify),
        "query": seeded(torch, lib, args.composition, 4096, Q27_28_28[:2], 2, 1, args.windows, verify),
    }
    copy_gbps = copy_rate(torch, lib, args.windows)
    for shape in shapes.values():
        shape["fraction_of_copy_rate"] = shape["gbps"] / copy_gbps
    result = {"tool": "ciphertext_wire_bench", "mode": "composition" if args.composition else "ciphertext entries",
              "library": "this build" if os.path.abspath(args.lib) == DEFAULT_LIB else "given by --lib",
              "copy_rate_gbps": copy_gbps,
              "copy_rate_source": "he_words_copy_device (non-temporal) of a 1 GiB slab in this run, read + write, best window",
              "shapes": shapes}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
