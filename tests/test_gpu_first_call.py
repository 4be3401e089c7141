"""What a process's FIRST calls return, one fresh process per case (tests/c/first_call.c over the C ABI: no Python, no PyTorch
and no HIP call of its own in the process -- the shape of the real caller, which the long-lived pytest process never has).

Every other GPU test shares one process, where "the first call" happens once per suite run for whichever entry comes first.
Here each cell of

    entry or order  x  ring (N = 256 batch 3, N = 8, N = 4096 batch 3 L = 3)  x  scratch (the library's default, its block
    cache told to keep what is released, a caller workspace of exactly the advertised bytes)  x  stream (the legacy default
    stream, one from he_stream_create)

starts a child that makes the calls and compares every output word with the CPU oracle's (tests/first_call_fixture.py).  The
default cells run once more with HEAMD_SCRATCH_POISON set (csrc/scratch_cache.cpp).  The six entries of
footprint_cases.ORACLE_ROWS run alone; relinearize, the call tests/c/abi_scheme.c once got wrong words from, also runs in
orders that tell "the first call of this entry" from "the n-th block the library takes" and "after a wait" from "behind work
still running":

    relin                    alone: the product uploaded from the fixture
    mul check relin          the order of abi_scheme.c: a readback and a wait between the two
    mul relin                nothing waits between them
    relin relin              both results compared
    mul check mul            the second product compared: the second block after a wait, no relinearize at all
    unsettled ...            the first two without the wait that otherwise follows the uploads (abi_scheme.c has none)

A child that ends by a signal, an abort, a failed library call (a HIP error is one) or the time limit stops the module: every
later case fails without starting a process.
On a mismatch the child's own report is the assertion message (the count of wrong words, where they lie, what they hold)."""
import os
import shutil
import subprocess

import pytest

import first_call_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "swift-homomorphic-encryption_amd", "lib")
ENTRIES = ("mul", "relin", "galois", "grouped", "inner", "dot")  # footprint_cases.ORACLE_ROWS, as first_call.c names them
ORDERS = {entry: "settle " + entry for entry in ENTRIES}
ORDERS.update({
    "mul-check-relin": "settle mul check relin",
    "mul-relin": "settle mul relin",
    "relin-relin": "settle relin relin",
    "mul-check-mul": "settle mul check mul",
    "unsettled-relin": "relin",
    "unsettled-mul-check-relin": "mul check relin",
})
SCRATCH = ("default", "cache", "workspace")
STREAMS = ("null", "own")
POISON = "0xA5"
# (order, ring, scratch, stream, poison)
CELLS = [(order, ring, scratch, stream, None) for order in ORDERS for ring in first_call_fixture.RINGS for scratch in SCRATCH
         for stream in STREAMS]
CELLS += [(order, ring, "default", stream, POISON) for order in ORDERS for ring in first_call_fixture.RINGS for stream in STREAMS]


def cell_id(cell):
    order, ring, scratch, stream, poison = cell
    return "%s-%s-%s-%s%s" % (order, ring.name, scratch, stream, "-poison" if poison else "")


def build_driver(directory, libdir=LIBDIR):
    binary = os.path.join(str(directory), "first_call")
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c", "first_call.c"), "-I", INCLUDE,
                    "-L", libdir, "-lhe_amd", "-Wl,-rpath," + libdir, "-o", binary], check=True)
    return binary


def run_cell(binary, fixture, cell, libdir=LIBDIR):
    """One child process, run once"""
    order, _, scratch, stream, poison = cell
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = libdir + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    env.pop("HEAMD_SCRATCH_POISON", None)
    if poison is not None:
        env["HEAMD_SCRATCH_POISON"] = poison
    return subprocess.run([binary, str(fixture), scratch, stream, *ORDERS[order].split()], capture_output=True, text=True, env=env,
                          timeout=120)


pytestmark = pytest.mark.gpu
_stopped = []  # why no further child may start: a child died or hung on the device


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not installed")
    return build_driver(tmp_path_factory.mktemp("first_call"))


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory, oracle):
    from conftest import host_threads

    directory = tmp_path_factory.mktemp("first_call_fixtures")
    paths = {}
    for ring in first_call_fixture.RINGS:
        paths[ring.name] = directory / (ring.name + ".bin")
        first_call_fixture.write(paths[ring.name], oracle, ring, threads=host_threads())
    return paths


@pytest.mark.parametrize("cell", CELLS, ids=[cell_id(cell) for cell in CELLS])
def test_first_calls_of_a_process(driver, fixtures, cell):
    assert not _stopped, "not started: " + _stopped[0]
    try:
        result = run_cell(driver, fixtures[cell[1].name], cell)
    except subprocess.TimeoutExpired:
        _stopped.append("%s ran into its time limit" % cell_id(cell))
        raise
    # (status 3: a call of the library failed -- a HIP error among them, after which nothing more may start on the card)
    if result.returncode < 0 or result.returncode in (3, 134, 139):
        _stopped.append("%s ended with status %d: %s" % (cell_id(cell), result.returncode, result.stderr.strip()[-300:]))
    assert result.returncode == 0, "status %d\n%s%s" % (result.returncode, result.stdout, result.stderr)
    assert "first call ok" in result.stdout
