"""csrc/scratch_ledger.hpp without a device: the policy of the scratch block cache -- which block a request gets, what is evicted
and in what order, what a forgotten stream means, how events are recycled -- held line by line to a restatement in Python.  A host
program compiled against the header (tests/c/scratch_ledger_probe.cpp, once plainly and once with ASan + UBSan) runs scripts of
operations and prints every decision with the ledger's whole state; `Model` below answers the same scripts."""
import os
import random
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "swift-homomorphic-encryption_amd", "csrc")
KIB, MIB = 1 << 10, 1 << 20
FORGOTTEN = 2**64 - 1


def block_size(size):
    grain = MIB if size >= MIB else 64 * KIB
    return -(-size // grain) * grain


class Model:
    """The policy as the issue that introduced the ledger states it, on Python lists; `run` answers one script line."""

    def __init__(self):
        self.free = []  # [ptr, bytes, stream, event, tick] in the order of release
        self.lent = {}
        self.spare = []
        self.tick = 0
        self.limit = 0
        self.allocations = 0
        self.complete = set()

    def cached_bytes(self):
        return sum(block[1] for block in self.free)

    def leave(self, block):
        """a block's event returns to the spare list only when the block leaves the free list"""
        self.free.remove(block)
        self.spare.append(block[3])

    def evict(self, keep):
        """among blocks whose release has completed, the oldest tick first, until at most `keep` bytes stay; completion is
        asked once per pass"""
        done = [block for block in self.free if block[3] in self.complete]
        victims = []
        for block in sorted(done, key=lambda block: block[4]):
            if self.cached_bytes() <= keep:
                break
            self.leave(block)
            victims.append(block[0])
        return " ".join(["victims", *map(str, victims)])

    def request(self, size, stream):
        if self.limit == 0:
            return "pool"
        want = block_size(size)
        fits = [block for block in self.free if want <= block[1] <= 2 * want]
        if not fits:
            self.allocations += 1
            self.lent[self.allocations * 0x10000] = want
            return f"miss {self.allocations * 0x10000}"
        # released on the requesting stream before any other, then the smaller, then the earlier in the list (min is stable)
        block = min(fits, key=lambda block: (block[2] != stream, block[1]))
        self.leave(block)
        self.lent[block[0]] = block[1]
        return f"hit {block[0]} wait={int(block[2] != stream)}"

    def release(self, ptr, stream, event):
        if ptr not in self.lent:
            return "notmine"
        size = self.lent.pop(ptr)
        if event is None:  # the record failed: the block goes back to the driver, a spare event stays spare
            return "freed"
        if self.spare:
            event = self.spare.pop()
        self.complete.discard(event)
        self.tick += 1
        self.free.append([ptr, size, stream, event, self.tick])
        return f"cached {event} " + self.evict(self.limit)

    def run(self, line):
        op, *args = line.split()
        args = [int(a, 0) for a in args]
        if op == "reset":
            self.__init__()
            decision = "ok"
        elif op == "limit":
            self.limit = args[0]
            decision = self.evict(args[0])
        elif op == "request":
            decision = self.request(*args)
        elif op == "release":
            decision = self.release(*args)
        elif op == "release_fail":
            decision = self.release(*args, None)
        elif op == "complete":
            self.complete.update(args)
            decision = "ok"
        elif op == "evict":
            decision = self.evict(args[0])
        elif op == "forget":
            for block in self.free:
                if block[2] == args[0]:
                    block[2] = FORGOTTEN
            decision = "ok"
        else:
            raise AssertionError(line)
        return f"{decision} | {self.state()}"

    def state(self):
        free = " ".join(":".join(map(str, block)) for block in self.free)
        lent = " ".join(f"{ptr}:{size}" for ptr, size in sorted(self.lent.items()))
        return f"cached={self.cached_bytes()} free=[{free}] lent=[{lent}] spare=[{' '.join(map(str, self.spare))}]"


def check_invariants(line):
    """on the PROBE's line: cached_bytes is the sum over the free list, no pointer is lent and cached, no event is in two places"""
    cached, free, lent, spare = re.fullmatch(r".* \| cached=(\d+) free=\[(.*)\] lent=\[(.*)\] spare=\[(.*)\]", line).groups()
    blocks = [tuple(map(int, block.split(":"))) for block in free.split()]
    assert int(cached) == sum(block[1] for block in blocks), line
    held = [block[0] for block in blocks] + [int(entry.split(":")[0]) for entry in lent.split()]
    assert len(held) == len(set(held)), line
    events = [block[3] for block in blocks] + [int(event) for event in spare.split()]
    assert len(events) == len(set(events)) and 0 not in events, line
    ticks = [block[4] for block in blocks]
    assert ticks == sorted(set(ticks)), line


def compile_probe(directory, name, extra):
    binary = directory / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I", CSRC,
                    os.path.join(ROOT, "tests", "c", "scratch_ledger_probe.cpp"), "-o", str(binary)], check=True)
    return binary


def sanitizers_link(directory):
    """the ASan and UBSan runtimes are installed: a trivial program links with them"""
    unit = directory / "empty.cpp"
    unit.write_text("int main() { return 0; }\n")
    return subprocess.run(["g++", "-fsanitize=address,undefined", str(unit), "-o", str(directory / "empty")],
                          capture_output=True).returncode == 0


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not installed")
    directory = tmp_path_factory.mktemp("scratch_ledger_" + request.param)
    if request.param == "plain":
        binary = compile_probe(directory, "scratch_ledger_probe", [])
    elif sanitizers_link(directory):
        binary = compile_probe(directory, "scratch_ledger_probe_san",
                               ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    else:
        pytest.skip("the sanitizer runtimes are not installed")
    count = [0]

    def run(lines):
        count[0] += 1
        script = directory / f"script{count[0]}.txt"
        script.write_text("\n".join(lines) + "\n")
        result = subprocess.run([str(binary), str(script)], capture_output=True, text=True)
        assert result.returncode == 0, result.stderr
        return result.stdout.splitlines()

    return run


def hold(probe, lines):
    """the probe's answers to `lines`, after comparing every one with the model's and checking the invariants on it"""
    model = Model()
    answers = probe(lines)
    assert len(answers) == len(lines)
    for number, (line, answer) in enumerate(zip(lines, answers)):
        assert answer == model.run(line), f"line {number}: {line}\n" + "\n".join(lines[:number + 1])
        check_invariants(answer)
    return [answer.split(" | ")[0] for answer in answers]


def test_header_includes_standard_headers_only():
    text = open(os.path.join(CSRC, "scratch_ledger.hpp")).read()
    includes = re.findall(r'#include\s*([<"][^>"]+[>"])', text)
    assert includes and all(name in ("<cstddef>", "<cstdint>", "<map>", "<vector>") for name in includes), includes
    assert "hip" not in re.sub(r"//[^\n]*", "", text).lower()


def test_block_sizes(probe):
    sizes = [1, 64 * KIB - 1, 64 * KIB, 64 * KIB + 1, MIB - 64 * KIB, MIB - 64 * KIB + 1, MIB - 1, MIB, MIB + 1, 5 * MIB - 1]
    lines = ["limit 1000000000"] + [f"request {size} 1" for size in sizes]
    hold(probe, lines)
    lent = probe(lines)[-1].split("lent=[")[1].split("]")[0].split()
    assert [int(entry.split(":")[1]) for entry in lent] == \
        [64 * KIB, 64 * KIB, 64 * KIB, 128 * KIB, MIB - 64 * KIB, MIB, MIB, MIB, 2 * MIB, 5 * MIB]


def cached_blocks(sizes, stream=1, first_event=100):
    """script: one cached block per size, released in this order on `stream`; their pointers are 0x10000, 0x20000, ..."""
    lines = ["limit 1000000000"] + [f"request {size} {stream}" for size in sizes]
    return lines + [f"release {(k + 1) * 0x10000} {stream} {first_event + k}" for k in range(len(sizes))]


def test_a_block_of_up_to_twice_the_request_is_taken_and_no_other(probe):
    setup = cached_blocks([128 * KIB])
    assert hold(probe, setup + ["request 131072 1"])[-1] == "hit 65536 wait=0"  # bytes == want
    assert hold(probe, setup + ["request 65536 1"])[-1] == "hit 65536 wait=0"  # bytes == 2 * want
    assert hold(probe, setup + ["request 65535 1"])[-1] == "hit 65536 wait=0"
    assert hold(probe, setup + ["request 131073 1"])[-1] == "miss 131072"  # bytes < want
    setup = cached_blocks([192 * KIB])
    assert hold(probe, setup + ["request 65536 1"])[-1] == "miss 131072"  # bytes == 2 * want + one grain
    assert hold(probe, setup + ["request 98304 1"])[-1] == "hit 65536 wait=0"  # want rounds to 128 KiB


def test_same_stream_comes_before_smaller(probe):
    lines = ["limit 1000000000", "request 65536 2", "request 131072 1", "release 65536 2 100", "release 131072 1 101"]
    assert hold(probe, lines + ["request 65536 1"])[-1] == "hit 131072 wait=0"  # the larger one, released on stream 1
    assert hold(probe, lines + ["request 65536 2"])[-1] == "hit 65536 wait=0"
    assert hold(probe, lines + ["request 65536 3"])[-1] == "hit 65536 wait=1"  # neither: the smaller one, behind its event
    # among two of the requesting stream, the smaller one
    lines = cached_blocks([128 * KIB, 64 * KIB, 128 * KIB])
    assert hold(probe, lines + ["request 65536 1"])[-1] == "hit 131072 wait=0"


def test_a_tie_is_kept_by_list_order(probe):
    lines = cached_blocks([64 * KIB, 64 * KIB, 64 * KIB])
    assert hold(probe, lines + ["request 1 1", "request 1 1", "request 1 1", "request 1 1"])[-4:] == \
        ["hit 65536 wait=0", "hit 131072 wait=0", "hit 196608 wait=0", "miss 262144"]
    # the list order is the order of release, not of allocation
    lines = ["limit 1000000000", "request 1 1", "request 1 1", "release 131072 1 100", "release 65536 1 101"]
    assert hold(probe, lines + ["request 1 7"])[-1] == "hit 131072 wait=1"


def test_blocks_in_flight_survive_an_eviction_to_nothing(probe):
    lines = cached_blocks([64 * KIB, 128 * KIB, 64 * KIB, MIB])
    decisions = hold(probe, lines + ["evict 0", "complete 102 100", "evict 0", "complete 101 103", "evict 1048576", "evict 0"])
    assert decisions[-6:] == ["victims", "ok", "victims 65536 196608", "ok", "victims 131072", "victims 262144"]
    # the oldest RELEASE goes first, whatever the order of allocation; eviction stops as soon as `keep` is met
    lines = ["limit 1000000000", "request 1 1", "request 1 1", "request 1 1", "release 196608 1 100", "release 65536 1 101",
             "release 131072 1 102", "complete 100 101 102"]
    assert hold(probe, lines + ["evict 131072", "evict 65536"])[-2:] == ["victims 196608", "victims 65536"]
    # a release over the limit evicts what has completed and keeps itself: it is still in flight
    lines = ["limit 65536", "request 1 1", "request 1 1", "release 65536 1 100", "complete 100", "release 131072 1 101"]
    assert hold(probe, lines)[-1] == "cached 101 victims 65536"
    # an event recorded anew is no longer complete
    lines = cached_blocks([64 * KIB]) + ["complete 100", "request 1 1", "release 65536 1 999", "evict 0"]
    assert hold(probe, lines)[-2:] == ["cached 100 victims", "victims"]


def test_a_forgotten_stream_is_no_longer_the_requesting_stream(probe):
    lines = cached_blocks([64 * KIB, 64 * KIB], stream=5)
    assert hold(probe, lines + ["request 1 5"])[-1] == "hit 65536 wait=0"
    assert hold(probe, lines + ["forget 5", "request 1 5"])[-1] == "hit 65536 wait=1"
    assert hold(probe, lines + ["forget 4", "request 1 5"])[-1] == "hit 65536 wait=0"
    # what the new holder of the handle releases is its own again, and comes before the forgotten stream's
    assert hold(probe, lines + ["forget 5", "request 1 5", "release 65536 5 300", "request 1 5"])[-1] == "hit 65536 wait=0"


def test_a_foreign_pointer_is_not_mine(probe):
    lines = ["limit 1000000000", "request 1 1", "release 4096 1 100", "release_fail 4096 1", "release 65536 1 100",
             "release 65536 1 101", "request 1 1", "release_fail 65536 1", "release 65536 1 102"]
    assert hold(probe, lines) == ["victims", "miss 65536", "notmine", "notmine", "cached 100 victims", "notmine",
                                  "hit 65536 wait=0", "freed", "notmine"]


def test_the_cache_set_to_nothing_with_blocks_still_lent(probe):
    lines = ["limit 1000000000", "request 1 1", "request 1 1", "request 1 1", "release 65536 1 100", "complete 100", "limit 0",
             "request 1 1", "release 131072 1 101", "complete 100", "release 196608 1 102", "evict 0"]
    assert hold(probe, lines)[-6:] == ["victims 65536", "pool", "cached 100 victims", "ok", "cached 102 victims 131072",
                                       "victims"]


def random_script(seed):
    """a couple of hundred operations a server could issue; the model only tells the generator what is lent and cached"""
    rng = random.Random(seed)
    model = Model()
    streams = [1, 2, 3, 4]
    sizes = [1, 60 * KIB, 64 * KIB, 100 * KIB, 128 * KIB, 200 * KIB, 256 * KIB, 900 * KIB, MIB, MIB + 1, 2 * MIB, 3 * MIB + 5]
    lines = ["reset", f"limit {rng.choice([64 * KIB, 512 * KIB, 4 * MIB, 64 * MIB])}"]
    next_event = 1000
    for line in lines:
        model.run(line)
    for _ in range(200):
        roll = rng.random()
        if roll < 0.36:
            line = f"request {rng.choice(sizes)} {rng.choice(streams)}"
        elif roll < 0.70 and model.lent:
            next_event += 1
            line = f"release {rng.choice(sorted(model.lent))} {rng.choice(streams)} {next_event}"
        elif roll < 0.73:
            foreign = rng.choice([4096] + [block[0] for block in model.free])  # never lent, or cached right now
            line = f"release {foreign} {rng.choice(streams)} 7"
        elif roll < 0.76 and model.lent:
            line = f"release_fail {rng.choice(sorted(model.lent))} {rng.choice(streams)}"
        elif roll < 0.88:
            events = [block[3] for block in model.free] + model.spare
            line = "complete " + " ".join(str(e) for e in events if rng.random() < 0.4)
        elif roll < 0.92:
            line = f"evict {rng.choice([0, 64 * KIB, 256 * KIB, MIB, 16 * MIB])}"
        elif roll < 0.95:
            line = f"limit {rng.choice([0, 64 * KIB, 512 * KIB, 4 * MIB, 64 * MIB])}"
        elif roll < 0.99:
            line = f"forget {rng.choice(streams)}"
        else:
            line = "complete"
        lines.append(line)
        model.run(line)
    return lines


def test_random_scripts(probe):
    lines = [line for seed in range(300) for line in random_script(seed)]
    decisions = hold(probe, lines)
    # the scripts reach every kind of decision, often
    for kind in ("hit", "miss", "pool", "notmine", "freed", "cached"):
        assert sum(decision.startswith(kind) for decision in decisions) >= 100, kind
    assert sum("wait=1" in decision for decision in decisions) >= 100
    assert sum("wait=0" in decision for decision in decisions) >= 100
    assert sum(re.search(r"victims \d+ \d+", decision) is not None for decision in decisions) >= 100  # two victims and more
