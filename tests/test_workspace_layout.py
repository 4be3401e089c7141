"""csrc/workspace_layout.hpp without a device: a host program compiled against the header lays parts out, Python's integers check
-- every offset a multiple of 16, the offsets the running sum of the rounded parts, an empty part without room of its own, the
total behind the last part -- and the same program once more under the address and undefined-behaviour sanitizers.  A scan of
csrc/ keeps round16 defined in this header alone."""
import os
import random
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "swift-homomorphic-encryption_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"]


def _build(directory, name, extra=()):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    binary = directory / name
    subprocess.run(["g++", *FLAGS, *extra, "-I", CSRC, os.path.join(ROOT, "tests", "c", "workspace_layout_probe.cpp"), "-o",
                    str(binary)], check=True)

    def ask(*parts):
        out = subprocess.run([str(binary), *map(str, parts)], capture_output=True, text=True, check=True)
        assert out.stderr == ""
        return [int(word) for word in out.stdout.split()]

    return ask


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("workspace_layout"), "workspace_layout_probe")


def round16(value):
    return -(-value // 16) * 16


def layouts():
    rng = random.Random(16)
    cases = [[], [0], [1], [16], [17], [0, 0, 0], [0, 5, 0, 0, 33, 0], [15, 16, 17, 31, 32, 33], [1] * 40,
             [2**40 + 1, 3, 2**33 - 7], [384, 1152, 0, 98304]]
    cases += [[rng.choice((0, 0, rng.randrange(1, 64), rng.randrange(1, 2**20), 16 * rng.randrange(1, 2**16)))
               for _ in range(rng.randrange(1, 12))] for _ in range(40)]
    return cases


def check(ask):
    for parts in layouts():
        *offsets, total = ask(*parts)
        assert len(offsets) == len(parts)
        running = 0
        for part, offset in zip(parts, offsets):
            assert offset % 16 == 0 and offset == running, (parts, offsets)
            running += round16(part)
        assert total == running, (parts, total)
        # an empty part takes no room and shares its offset with the next; the total is the last offset plus the last rounded part
        for i, part in enumerate(parts[:-1]):
            assert (offsets[i + 1] == offsets[i]) == (part == 0), (parts, offsets)
        if parts:
            assert total == offsets[-1] + round16(parts[-1])
    for value in (0, 1, 15, 16, 17, 2**32 - 1, 2**32, 2**63 + 1):
        assert ask("round", value) == [round16(value)]


def test_header_includes_nothing_of_hip():
    text = open(os.path.join(CSRC, "workspace_layout.hpp")).read()
    includes = re.findall(r'#include\s*[<"]([^>"]+)[>"]', text)
    assert includes and all(name in ("cstddef", "cstdint") for name in includes), includes


def test_offsets_are_the_running_sum_of_the_rounded_parts(probe):
    check(probe)


def test_the_same_under_the_sanitizers(tmp_path):
    # (the runtimes linked into the program: it stands alone, whatever else the machine loads into its processes)
    check(_build(tmp_path, "workspace_layout_probe_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                          "-static-libasan", "-static-libubsan"]))


def test_round16_is_defined_once():
    found = []
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hpp", ".cpp", ".hip")):
            text = open(os.path.join(CSRC, name)).read()
            found += [name for _ in re.finditer(r"\bsize_t\s+round16\s*\(", text)]
    assert found == ["workspace_layout.hpp"], found
