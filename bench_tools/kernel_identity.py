"""Whether two builds of the library hold the same kernels (no GPU needed): the check of a change that only regroups sources.

  python bench_tools/kernel_identity.py BEFORE_BUILD_DIR AFTER_BUILD_DIR

Every object (*.o) of either directory is read, since a kernel may have moved to another object.  A kernel is keyed by its
demangled full name and compared by
  - its metadata notes (bench_tools/kernel_metadata.py): VGPRs, SGPRs, scratch, spilled VGPRs, LDS, max workgroup size;
  - its instruction stream (bench_tools/mad_counts.py disassemble), without what depends only on where the kernel lies in
    its code object: the address of each instruction, a branch target's symbol (kept as the offset from the kernel's start),
    the padding behind the last instruction.
A name that several objects define is compared as the sorted list of its definitions.  Prints the counts of identical,
changed, only-before and only-after kernels and every name that is not identical; exit status 0 only if all are identical.
"""
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bench_tools"))
import kernel_metadata  # noqa: E402
import mad_counts  # noqa: E402

PADDING = ("s_nop", "s_code_end", "...")  # ("...": the run of zeros llvm-objdump skips behind a section's last kernel)


def normalised(body):
    lines = []
    for line in body:
        line = re.sub(r"//\s*[0-9A-Fa-f]+:", "//", line)                 # the instruction's address
        line = re.sub(r"<[^<>\s]+?(\+0x[0-9a-f]+)?>\s*$", lambda m: "<%s>" % (m.group(1) or "+0x0"), line)  # branch target
        lines.append(re.sub(r"\s+", " ", line).strip())
    while lines and lines[-1].split(" ")[0] in PADDING:
        lines.pop()
    return lines


def kernels_of(build_dir):
    """{demangled full name: sorted [(metadata, instruction lines), ...]} over all objects of a build directory."""
    found = {}
    with tempfile.TemporaryDirectory() as workdir:
        for path in sorted(glob.glob(os.path.join(os.path.abspath(build_dir), "*.o"))):
            code = kernel_metadata.code_object(path, workdir)
            if code is None:  # host code only
                continue
            rows = list(kernel_metadata.kernels(code))
            names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True, text=True,
                                   check=True).stdout.split("\n")
            bodies = mad_counts.disassemble(path, workdir, full_names=True)
            for row, name in zip(rows, names):
                notes = tuple(sorted((key, value) for key, value in row.items() if key != "name"))
                found.setdefault(name, []).append((notes, tuple(normalised(bodies[name]))))
    return {name: sorted(definitions) for name, definitions in found.items()}


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    before, after = kernels_of(sys.argv[1]), kernels_of(sys.argv[2])
    only_before, only_after = sorted(set(before) - set(after)), sorted(set(after) - set(before))
    changed = []
    for name in sorted(set(before) & set(after)):
        if before[name] == after[name]:
            continue
        what = []
        if len(before[name]) != len(after[name]):
            what.append(f"{len(before[name])} -> {len(after[name])} definitions")
        if [d[0] for d in before[name]] != [d[0] for d in after[name]]:
            what.append("metadata %s -> %s" % ([dict(d[0]) for d in before[name]], [dict(d[0]) for d in after[name]]))
        if [d[1] for d in before[name]] != [d[1] for d in after[name]]:
            what.append("instructions %s -> %s" % ([len(d[1]) for d in before[name]], [len(d[1]) for d in after[name]]))
        changed.append((name, "; ".join(what)))
    identical = len(set(before) & set(after)) - len(changed)
    print(f"kernels: {len(before)} before, {len(after)} after")
    print(f"identical {identical}  changed {len(changed)}  only before {len(only_before)}  only after {len(only_after)}")
    for name, what in changed:
        print(f"changed: {name}\n    {what}")
    for name in only_before:
        print(f"only before: {name}")
    for name in only_after:
        print(f"only after: {name}")
    return 1 if changed or only_before or only_after else 0


if __name__ == "__main__":
    sys.exit(main())
