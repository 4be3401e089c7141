"""Processed-database files on the device, timed.  One JSON line, also written to --out:

    python bench_tools/pir_database_file_bench.py [--yardstick-lib PATH/libhe_amd.so] [--plaintexts 16384] [--out FILE]

Shapes: `--plaintexts` plaintexts at the PIR benchmark's ring, N = 8192 with L = 4 moduli of 55 bits (five primes, the last the
key-switching one; as bench_tools/pir_database_bench.py) on 8-byte words -- no modulus of that set fits UInt32, so the 4-byte
entries are timed on the reference's n_4096_logq_27_28_28 set (N = 4096, L = 2).  Presence patterns: all present, one nil in
16, alternating.

Per shape, pattern and direction:
  device     he_pir_database_load_device(_u32) / he_pir_database_save_device(_u32): one call for the whole body;
  yardstick  the same bytes from the polynomial-level entries, which is all a caller had before: load is one
             he_poly_deserialize_device(_u32) per run of present plaintexts (records S + 1 bytes apart: the tag in between),
             save one he_poly_serialize_device(_u32) per present plaintext (that entry packs its records tightly, so a run
             cannot keep room for its tags).  Tags are not written and nil slabs not zeroed: in the yardstick's favour.
             --yardstick-lib names an older build of the library (these entries exist in it unchanged); without it the
             yardstick is this build's own polynomial-level entries, and the JSON says so.
Both are timed in three alternating rounds; a round is the median of --windows windows (after one warm-up window) of `reps`
back-to-back calls between two host clock reads, the second after a device synchronise, reps sized for about 0.25 s.  The
figure of a path is the median of its three rounds and its spread their largest minus their smallest.  Before timing, untimed:
the device entries and the yardstick give the same words for every present plaintext and the same payload bytes.
bytes = file bytes + slab bytes of the present plaintexts (+ the zeros written for nil ones on load); rate = bytes / time, set
against the copy rate measured in this run (he_words_copy_device, non-temporal, a 1 GiB slab, read + written, best window).
  host scan  he_pir_database_file_scan over the file's host image, median of 5 runs, as a time per plaintext.
A server's start-up moves the file over PCIe first: that, not these kernels, bounds it; this tool does not time the upload."""
import argparse
import ctypes
import json
import os
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "swift-homomorphic-encryption_amd", "lib", "libhe_amd.so")
vp, c_size, c_int, c_u32, c_u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64
SIZE_P = ctypes.POINTER(c_size)

OLD = {
    "he_poly_context_create": (c_int, [c_u32, ctypes.POINTER(c_u64), c_u32, ctypes.POINTER(vp)]),
    "he_poly_serialization_byte_count": (c_size, [vp, c_int]),
    "he_poly_serialize_device": (c_int, [vp, vp, c_size, c_int, vp, vp]),
    "he_poly_deserialize_device": (c_int, [vp, vp, c_size, c_size, c_int, vp, vp]),
    "he_poly_serialize_device_u32": (c_int, [vp, vp, c_size, c_int, vp, vp]),
    "he_poly_deserialize_device_u32": (c_int, [vp, vp, c_size, c_size, c_int, vp, vp]),
    "he_words_copy_device": (c_int, [vp, vp, c_size, c_int, vp]),
    "he_set_scratch_cache": (c_int, [c_u64]),
}
NEW = {
    "he_bfv_context_create": (c_int, [c_u32, c_u64, ctypes.POINTER(c_u64), c_u32, ctypes.POINTER(vp)]),
    "he_bfv_context_create_u32": (c_int, [c_u32, c_u64, ctypes.POINTER(c_u64), c_u32, ctypes.POINTER(vp)]),
    "he_pir_database_file_scan": (c_int, [vp, vp, c_size, vp, c_size, SIZE_P, SIZE_P, SIZE_P]),
    "he_pir_database_file_header": (c_int, [c_size, vp]),
    "he_pir_database_load_device": (c_int, [vp, vp, c_size, vp, c_size, vp, vp, vp]),
    "he_pir_database_load_device_u32": (c_int, [vp, vp, c_size, vp, c_size, vp, vp, vp]),
    "he_pir_database_save_device": (c_int, [vp, vp, vp, c_size, vp, c_size, vp, vp]),
    "he_pir_database_save_device_u32": (c_int, [vp, vp, vp, c_size, vp, c_size, vp, vp]),
}
# the reference's n_4096_logq_27_28_28 coefficient moduli (EncryptionParameters.swift)
Q27_28_28 = [(1 << 27) - 40959, (1 << 28) - 65535, (1 << 28) - 73727]
PATTERNS = ("all", "one-nil-in-16", "alternating")


def load(path, table):
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


def check(status, what):
    if status != 0:
        raise RuntimeError(f"{what}: status {status}")


def ptr(tensor, offset_bytes=0):
    return vp(tensor.data_ptr() + offset_bytes)


def windows(torch, call, count):
    """the median seconds per call over `count` windows of about 0.25 s each, after a warm-up window"""
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
        if window:
            times.append((time.perf_counter() - start) / reps)
    return float(np.median(times)), min(times)


def alternate(torch, paths, window_count, rounds=3):
    """{name: call} -> {name: {median_us, spread_us, rounds_us}}, the paths taking turns round by round"""
    seen = {name: [] for name in paths}
    for _ in range(rounds):
        for name, call in paths.items():
            seen[name].append(1e6 * windows(torch, call, window_count)[0])
    return {name: {"median_us": float(np.median(v)), "spread_us": max(v) - min(v), "rounds_us": v} for name, v in seen.items()}


def mask_of(pattern, count):
    mask = np.ones(count, dtype=np.uint8)
    if pattern == "one-nil-in-16":
        mask[7::16] = 0
    elif pattern == "alternating":
        mask[1::2] = 0
    return mask


def runs_of(mask):
    """[(first, length)] of the runs of present plaintexts"""
    edges = np.flatnonzero(np.diff(np.concatenate(([0], mask != 0, [0])).astype(np.int8)))
    return [(int(a), int(b - a)) for a, b in zip(edges[0::2], edges[1::2])]


def shape(torch, lib, old, word_bits, degree, t, moduli, count, window_count):
    suffix = "_u32" if word_bits == 32 else ""
    word = word_bits // 8
    handle = vp()
    array = (c_u64 * len(moduli))(*moduli)
    create = lib.he_bfv_context_create_u32 if word_bits == 32 else lib.he_bfv_context_create
    check(create(degree, t, array, len(moduli), ctypes.byref(handle)), "he_bfv_context_create")
    rows = len(moduli) - 1
    poly = vp()
    check(old.he_poly_context_create(degree, array, rows, ctypes.byref(poly)), "he_poly_context_create")
    payload = old.he_poly_serialization_byte_count(poly, 0)
    words = rows * degree
    generator = torch.Generator("cuda").manual_seed(degree + word_bits)
    slab = torch.stack([torch.randint(0, q, (count, degree), dtype=torch.int64, device="cuda", generator=generator)
                        for q in moduli[:rows]], dim=1).contiguous()
    if word_bits == 32:
        slab = slab.to(torch.int32)
    load_fn, save_fn = getattr(lib, "he_pir_database_load_device" + suffix), getattr(lib, "he_pir_database_save_device" + suffix)
    poly_load, poly_save = getattr(old, "he_poly_deserialize_device" + suffix), getattr(old, "he_poly_serialize_device" + suffix)
    out = {"word_bits": word_bits, "degree": degree, "rows": rows, "plaintexts": count, "payload_bytes": payload, "patterns": {}}
    for pattern in PATTERNS:
        mask = mask_of(pattern, count)
        present = torch.from_numpy(mask).cuda()
        live = int(mask.sum())
        body_bytes = count + payload * live
        ranks = np.concatenate(([0], np.cumsum(mask != 0)))[:-1]
        offsets = (np.arange(count) + payload * ranks).tolist()  # of every tag in the body
        body = torch.zeros(body_bytes + 16, dtype=torch.uint8, device="cuda")
        theirs = torch.zeros_like(body)
        loaded = torch.empty_like(slab)
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        runs = runs_of(mask)
        present_index = np.flatnonzero(mask).tolist()

        def device_save():
            check(save_fn(handle, ptr(slab), ptr(present), count, ptr(body), body_bytes, ptr(flag), None), "save")

        def device_load():
            check(load_fn(handle, ptr(body), body_bytes, ptr(present), count, ptr(loaded), ptr(flag), None), "load")

        def yardstick_save():
            for p in present_index:
                check(poly_save(poly, ptr(slab, p * words * word), 1, 0, ptr(theirs, offsets[p] + 1), None), "poly save")

        def yardstick_load():
            for first, length in runs:
                check(poly_load(poly, ptr(body, offsets[first] + 1), payload + 1, length, 0, ptr(loaded, first * words * word),
                                None), "poly load")

        # untimed: both paths give the same payload bytes and the same words
        device_save()
        yardstick_save()
        select = torch.from_numpy(mask.astype(bool)).cuda()
        tags = torch.tensor(offsets, device="cuda")
        assert int(flag.item()) == 0 and torch.equal(body[tags], (present != 0).to(torch.uint8))
        theirs[tags] = body[tags]  # the yardstick writes no tags
        assert torch.equal(body, theirs)
        loaded.fill_(-1)
        device_load()
        assert int(flag.item()) == 0 and torch.equal(loaded[select], slab[select]) and not bool(loaded[~select].any())
        loaded.fill_(-1)
        yardstick_load()
        assert torch.equal(loaded[select], slab[select])

        timed = {"load": alternate(torch, {"device": device_load, "yardstick": yardstick_load}, window_count),
                 "save": alternate(torch, {"device": device_save, "yardstick": yardstick_save}, window_count)}
        moved = {"load": body_bytes + count * words * word, "save": body_bytes + live * words * word}
        for direction, paths in timed.items():
            for path in paths.values():
                path["bytes"] = moved[direction]
                path["gbps"] = moved[direction] / path["median_us"] / 1e3
            paths["yardstick"]["calls"] = len(runs) if direction == "load" else live
            paths["device_over_yardstick"] = paths["device"]["median_us"] / paths["yardstick"]["median_us"]
            paths["within_yardstick_spread"] = bool(paths["device"]["median_us"] <=
                                                    paths["yardstick"]["median_us"] + paths["yardstick"]["spread_us"])
        # the host walk over the file's image
        header = (ctypes.c_uint8 * 5)()
        check(lib.he_pir_database_file_header(count, header), "header")
        image = np.empty(5 + body_bytes, dtype=np.uint8)
        image[:5] = np.frombuffer(bytes(header), dtype=np.uint8)
        image[5:] = body[:body_bytes].cpu().numpy()
        host_mask = np.zeros(count, dtype=np.uint8)
        outs = [c_size() for _ in range(3)]
        scans = []
        for _ in range(5):
            start = time.perf_counter()
            check(lib.he_pir_database_file_scan(handle, vp(image.ctypes.data), image.size, vp(host_mask.ctypes.data), count,
                                                *[ctypes.byref(o) for o in outs]), "scan")
            scans.append(time.perf_counter() - start)
        assert outs[0].value == count and outs[1].value == live and outs[2].value == image.size
        assert np.array_equal(host_mask, (mask != 0).astype(np.uint8))
        timed["host_scan"] = {"median_us": 1e6 * float(np.median(scans)), "ns_per_plaintext": 1e9 * float(np.median(scans)) / count}
        timed["file_bytes"] = 5 + body_bytes
        out["patterns"][pattern] = timed
        del body, theirs, loaded, image
        torch.cuda.empty_cache()
    return out


def copy_rate(torch, lib, window_count):
    """GB/s read + written by he_words_copy_device (non-temporal) over a 1 GiB slab: bench.py's copy_rate"""
    words = 1 << 27
    source = torch.zeros(words, dtype=torch.int64, device="cuda")
    target = torch.empty_like(source)
    best = windows(torch, lambda: check(lib.he_words_copy_device(ptr(source), ptr(target), words, 1, None), "copy"),
                   window_count)[1]
    return 2 * words * 8 / best / 1e9


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--lib", default=DEFAULT_LIB)
    parser.add_argument("--yardstick-lib", default=None)
    parser.add_argument("--plaintexts", type=int, default=16384)
    parser.add_argument("--windows", type=int, default=7)
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    import sys

    sys.path.insert(0, os.path.join(ROOT, "swift-homomorphic-encryption_amd"))
    import torch

    import heamd  # (prime generation only; the timed calls go through ctypes)

    lib = load(args.lib, {**OLD, **NEW})
    old = load(args.yardstick_lib, OLD) if args.yardstick_lib else lib
    for each in {id(lib): lib, id(old): old}.values():  # enqueue-only calls, as a server sets it
        check(each.he_set_scratch_cache(2**64 - 1), "he_set_scratch_cache")
    t8192 = int(heamd.generate_primes([17], True, 8192)[0])
    q8192 = [int(q) for q in heamd.generate_primes([55] * 5, False, 8192)]
    shapes = {
        "u64-n8192-4x55": shape(torch, lib, old, 64, 8192, t8192, q8192, args.plaintexts, args.windows),
        "u32-n4096-27-28": shape(torch, lib, old, 32, 4096, (1 << 16) + 1, Q27_28_28, args.plaintexts, args.windows),
    }
    copy_gbps = copy_rate(torch, lib, args.windows)
    for entry in shapes.values():
        for timed in entry["patterns"].values():
            for direction in ("load", "save"):
                for name in ("device", "yardstick"):
                    timed[direction][name]["fraction_of_copy_rate"] = timed[direction][name]["gbps"] / copy_gbps
    result = {"tool": "pir_database_file_bench",
              "yardstick_library": "given by --yardstick-lib" if args.yardstick_lib else "this build's polynomial-level entries",
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
