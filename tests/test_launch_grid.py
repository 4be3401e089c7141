"""csrc/launch_grid.hpp without a device: the grid arithmetic at HIP's limit of 2^32 - 1 lanes per launch (a host program compiled
against the header answers, Python's integers check), the HEAMD_GRID_CAP override, and a scan of csrc/ that keeps the table of
tests/test_gpu_grid_stride.py complete and the kernel files free of grid caps of their own."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "swift-homomorphic-encryption_amd", "csrc")
LIMIT = 2**32 - 1
SIZE_MAX = 2**64 - 1


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    binary = tmp_path_factory.mktemp("launch_grid") / "launch_grid_probe"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "c", "launch_grid_probe.cpp"), "-o", str(binary)], check=True)

    def ask(*queries, cap=None):
        env = {k: v for k, v in os.environ.items() if k != "HEAMD_GRID_CAP"}
        if cap is not None:
            env["HEAMD_GRID_CAP"] = cap
        args = [str(a) for query in queries for a in query]
        result = subprocess.run([str(binary), *args], capture_output=True, text=True, env=env, check=True)
        answers = [int(line) for line in result.stdout.split()]
        assert len(answers) == len(queries)
        return answers

    return ask


def ceil_div(a, b):
    return -(-a // b)


THREADS = (64, 256, 1024)


def work_items(threads):
    return [0, 1, threads - 1, threads, threads + 1, 2**32 - 1, 2**32, 2**32 + 1, 2**40, SIZE_MAX]


def test_header_includes_nothing_of_hip():
    text = open(os.path.join(CSRC, "launch_grid.hpp")).read()
    includes = re.findall(r'#include\s*[<"]([^>"]+)[>"]', text)
    assert includes and all(name in ("cstddef", "cstdint", "cstdlib") for name in includes), includes


def test_grids_are_exact_and_stay_within_the_lane_limit(probe):
    cases = [(threads, items) for threads in THREADS for items in work_items(threads)]
    grids = probe(*[("for", items, threads) for threads, items in cases])
    limits = probe(*[("max", threads) for threads in THREADS])
    assert limits == [LIMIT // threads for threads in THREADS] and limits[1] == 16777215
    for (threads, items), grid in zip(cases, grids):
        assert grid >= 1, (threads, items)
        assert grid * threads <= LIMIT, (threads, items, grid)
        exact = max(1, ceil_div(items, threads))
        assert grid == min(exact, LIMIT // threads), (threads, items, grid)
    # the pure arithmetic, at caps other than the launch limit: SIZE_MAX items must not wrap to a small grid
    pure = [(items, threads, cap) for threads in THREADS for items in work_items(threads) for cap in (1, 3, 2048, 2**20, SIZE_MAX)]
    for (items, threads, cap), blocks in zip(pure, probe(*[("blocks", *c) for c in pure])):
        assert blocks == min(max(1, ceil_div(items, threads)), cap), (items, threads, cap)


def test_one_item_per_lane_grids_never_cover_part_of_the_items(probe):
    """exact_grid (kernels without a loop): the exact count, and beyond what HIP launches a grid HIP refuses -- never fewer
    workgroups than the items need and a launch that succeeds"""
    cases = [(items, threads) for threads in THREADS for items in work_items(threads)]
    for (items, threads), grid in zip(cases, probe(*[("exact", *c) for c in cases])):
        exact = max(1, ceil_div(items, threads))
        assert grid == exact or (exact > LIMIT // threads and grid * threads > LIMIT), (items, threads, grid)


def test_launch_fits_on_both_sides_of_the_limit(probe):
    assert probe(("fits", 16777215, 256), ("fits", 16777216, 256), ("fits", 0, 256), ("fits", 2**31 - 1, 256),
                 ("fits", 2**32 - 1, 1), ("fits", 2**32, 1), ("fits", LIMIT // 1024, 1024), ("fits", LIMIT // 1024 + 1, 1024),
                 ("fits", SIZE_MAX, 64)) == [1, 0, 1, 0, 1, 0, 1, 0, 0]


def test_override_lowers_and_never_raises(probe):
    items = 256 * 1000 + 5  # 1001 workgroups uncapped
    for cap, want in (("1", 1), ("3", 3), ("1000", 1000), ("1001", 1001), ("1002", 1001), ("4000000000", 1001),
                      (str(SIZE_MAX), 1001), ("99999999999999999999999999", 1001)):
        assert probe(("for", items, 256), cap=cap) == [want], cap
    # never beyond the lane limit either
    assert probe(("for", SIZE_MAX, 256), cap=str(2**40)) == [16777215]
    # a single small launch stays what it was
    assert probe(("for", 5, 256), ("for", 0, 256), cap="3") == [1, 1]


@pytest.mark.parametrize("junk", ["", "0", "00", "abc", "-3", "3x", " 3", "3 ", "+3", "0x10", "1e3", "3.0"])
def test_junk_overrides_are_ignored(probe, junk):
    assert probe(("for", 256 * 1000 + 5, 256), ("for", 256 * 1000 + 5, 256, 2048), cap=junk) == [1001, 1001]


def test_override_and_own_cap_combine_by_minimum(probe):
    items = 256 * 5000
    assert probe(("for", items, 256, 2048)) == [2048]
    assert probe(("for", items, 256, 2048), cap="3") == [3]
    assert probe(("for", items, 256, 2048), cap="2047") == [2047]
    assert probe(("for", items, 256, 2048), cap="100000") == [2048]
    assert probe(("for", items, 256, 2), cap="3") == [2]
    assert probe(("for", SIZE_MAX, 256, SIZE_MAX)) == [16777215]
    # one workgroup per item (the kernels that stride by gridDim.x alone): the limit still counts the workgroup's lanes
    assert probe(("for_blocks", 5, 256, 2**20), ("for_blocks", 2**21, 256, 2**20), ("for_blocks", SIZE_MAX, 256)) == \
        [5, 2**20, 16777215]
    assert probe(("for_blocks", 2**21, 256, 2**20), ("for_blocks", 2, 256, 2**20), cap="3") == [3, 2]


# ---- the scan ------------------------------------------------------------------------------------------------------------------------
def _hip_sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _balanced(text, start, open_char, close_char):
    """index just past the bracket that closes the one at text[start]"""
    depth = 0
    for i in range(start, len(text)):
        if text[i] == open_char:
            depth += 1
        elif text[i] == close_char:
            depth -= 1
            if depth == 0:
                return i + 1
    raise AssertionError("unbalanced source")


def global_functions(text):
    """(name, body) of every __global__ function definition"""
    text = _strip_comments(text)
    found = []
    for match in re.finditer(r"__global__", text):
        brace = text.index("{", match.end())
        head = text[match.end():brace]
        bounds = head.find("__launch_bounds__")
        if bounds >= 0:
            open_paren = head.index("(", bounds)
            head = head[:bounds] + head[_balanced(head, open_paren, "(", ")"):]
        name = re.search(r"(\w+)\s*\(", head)
        assert name, head
        found.append((name.group(1), text[brace:_balanced(text, brace, "{", "}")]))
    return found


def strides_by_grid(body):
    """the body uses gridDim.x as a stride (anything but dividing it: the transforms split their grid into replicas with
    gridDim.x / count)"""
    return re.search(r"gridDim\.x(?!\s*/)", body) is not None


def test_scan_reads_kernels_the_way_it_claims():
    sample = """
    template <int L> __global__ void __launch_bounds__(kThreads, min_waves(L - 1, 2))
        first_kernel(const W* in, size_t n) { for (size_t i = blockIdx.x; i < n; i += size_t(gridDim.x) * 256) { in[i]; } }
    __global__ __launch_bounds__((kBsgs<W, 2>)) void second_kernel(int a) { locate(blockIdx.x, gridDim.x / 4); }
    __global__ void third_kernel(int a) { const size_t stride = gridDim.x * 256; // gridDim.x / 2
    }
    """
    kernels = global_functions(sample)
    assert [name for name, _ in kernels] == ["first_kernel", "second_kernel", "third_kernel"]
    assert [strides_by_grid(body) for _, body in kernels] == [True, False, True]


def test_every_strided_kernel_is_in_the_gpu_table():
    import test_gpu_grid_stride as table

    strided = {}
    for source in _hip_sources():
        for name, body in global_functions(open(os.path.join(CSRC, source)).read()):
            if strides_by_grid(body):
                strided[name] = source
    assert len(strided) >= 35  # the scan has not gone blind
    missing = {name: source for name, source in strided.items() if name not in table.COVERED_KERNELS}
    assert not missing, f"strided kernels without a row in tests/test_gpu_grid_stride.py: {missing}"
    stale = [name for name in table.COVERED_KERNELS if name not in strided]
    assert not stale, f"rows of tests/test_gpu_grid_stride.py name kernels that do not stride (or no longer exist): {stale}"


def private_grid_caps(text):
    """What a kernel file may not hold any more: a launch guard or cap written with << 31 or 0x7fffffff, a grid cap constant that does not reach
    launch_grid, a grid helper that computes its own, or a grid clamped by hand."""
    text = _strip_comments(text)
    found = [m.group(0) for m in re.finditer(r"<<\s*31\b", text)]
    found += [m.group(0) for m in re.finditer(r"0x7fffffff\w*", text, flags=re.I)]
    found += [m.group(0) for m in re.finditer(r"\bkGridCap\b", text)]
    for match in re.finditer(r"\b(k\w*GridCap)\b\s*=", text):
        uses = [m for m in re.finditer(r"launch_grid::grid_for(?:_blocks)?\s*\(", text)
                if match.group(1) in text[m.end():_balanced(text, m.end() - 1, "(", ")")]]
        if not uses:
            found.append(match.group(0))
    for match in re.finditer(r"\binline\s+unsigned\s+(\w*grid\w*)\s*\([^)]*\)\s*\{", text):
        body = text[match.end() - 1:_balanced(text, match.end() - 1, "{", "}")]
        if "launch_grid::" not in body:
            found.append(match.group(1))
    found += [m.group(0) for m in re.finditer(r"<\s*(\w*[Cc]ap)\s*\?[^;]*?:\s*\1\b", text)]
    return found


def test_no_kernel_file_keeps_a_grid_cap_of_its_own():
    for source in _hip_sources():
        text = open(os.path.join(CSRC, source)).read()
        assert private_grid_caps(text) == [], source
        launches_strided = any(strides_by_grid(body) for _, body in global_functions(text))
        if launches_strided:
            assert '#include "launch_grid.hpp"' in text, source


def test_scan_catches_the_caps_this_project_had():
    old_helper = """
    constexpr size_t kGridCap = (size_t(1) << 31) - 1;
    inline unsigned grid_for(size_t work_items) {
        const size_t blocks = (work_items + kThreads - 1) / kThreads;
        const size_t cap = kGridCap;
        return static_cast<unsigned>(blocks < cap ? (blocks ? blocks : 1) : cap);
    }"""
    assert len(private_grid_caps(old_helper)) >= 3
    assert private_grid_caps("if (blocks >= (size_t(1) << 31)) return hipErrorInvalidValue;")
    assert private_grid_caps("if (rows > 0x7fffffffull) return hipErrorInvalidValue;")
    assert private_grid_caps("constexpr size_t kUnpackGridCap = size_t(1) << 20;\n"
                             "const unsigned grid = static_cast<unsigned>(slots < kUnpackGridCap ? slots : kUnpackGridCap);")
    assert private_grid_caps("inline unsigned flat_grid(size_t items) { return (items + 255) / 256; }")
    assert private_grid_caps("constexpr size_t kUnpackGridCap = size_t(1) << 20;\n"
                             "const unsigned grid = launch_grid::grid_for_blocks(slots, 256, kUnpackGridCap);") == []
