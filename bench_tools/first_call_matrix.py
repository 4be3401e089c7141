"""The fresh-process matrix of tests/test_gpu_first_call.py against any build of the library, cell by cell.

    python bench_tools/first_call_matrix.py [--lib DIR] [--out FILE] [--only SUBSTRING]

--lib DIR  the directory of the libhe_amd.so to link and run against (default: the tree's own) -- a parent commit's build, to set
           its failing cells beside the tree's.
One child process per cell, run once; one line per cell (ok / WRONG / the status), and under a wrong cell the child's own
report: how many words, where, what they hold.  The run ends at the first child that dies by a signal, aborts, hangs or
reports a failed library call.
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "swift-homomorphic-encryption_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    import first_call_fixture
    import oracle
    import test_gpu_first_call as T

    parser = argparse.ArgumentParser()
    parser.add_argument("--lib", default=T.LIBDIR)
    parser.add_argument("--out", default=None)
    parser.add_argument("--only", default="")
    args = parser.parse_args()
    libdir = os.path.abspath(args.lib)
    oracle.build()
    out = open(args.out, "w") if args.out else sys.stdout

    def say(text):
        out.write(text + "\n")
        out.flush()

    with tempfile.TemporaryDirectory() as directory:
        binary = T.build_driver(directory, libdir)
        fixtures = {}
        for ring in first_call_fixture.RINGS:
            fixtures[ring.name] = os.path.join(directory, ring.name + ".bin")
            first_call_fixture.write(fixtures[ring.name], oracle, ring, threads=min(16, len(os.sched_getaffinity(0))))
        say("library: %s" % os.path.join(libdir, "libhe_amd.so"))
        counts = {"ok": 0, "WRONG": 0}
        for cell in T.CELLS:
            name = T.cell_id(cell)
            if args.only not in name:
                continue
            try:
                result = T.run_cell(binary, fixtures[cell[1].name], cell, libdir)
            except subprocess.TimeoutExpired:
                say("%-60s HUNG (time limit); stopping" % name)
                return 1
            verdict = {0: "ok", 1: "WRONG"}.get(result.returncode, "status %d" % result.returncode)
            counts[verdict] = counts.get(verdict, 0) + 1
            say("%-60s %s" % (name, verdict))
            if result.returncode != 0:
                for line in (result.stdout + result.stderr).splitlines():
                    say("      " + line)
            if result.returncode < 0 or result.returncode in (3, 134, 139):
                say("a child died or a library call failed; stopping")
                return 1
        say("cells: " + ", ".join("%d %s" % (n, verdict) for verdict, n in sorted(counts.items())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
