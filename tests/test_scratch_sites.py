"""tests/scratch_sites.py held to the source: the table lists exactly the places in csrc/ that take library-owned scratch, every
entry it names is in include/he_amd.h, every case it names exists, and what it leaves without a case keeps to the limits."""
import ast
import os
import re

import aliasing_cases as A
import footprint_cases as F
import scratch_sites as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "swift-homomorphic-encryption_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "he_amd.h")
# the scratch layer itself: the class definitions and the allocator
LAYER = ("api_internal.hpp", "scratch_cache.cpp", "zeroized_workspace.hpp", "scratch_ledger.hpp")
DECLARATION = re.compile(r"^\s+(?:heamd::)?(?:Scratch|ZeroizedWorkspace) (\w+\(.*\));\s*(?://.*)?$", re.S)
# a definition at column 0: `int name(`, `int heamd::name(`, `HEAMD_..._ENTRY(name, ...)` is not one (its body is a macro's)
FUNCTION = re.compile(r'^(?!\s|//|#|namespace|using|template|struct|class|static_assert|extern "C" \{|\}|[A-Z_]+\()[^;=]*?\b(\w+)\(')
MAX_OTHER_EXEMPT = 4


def sites_in_source():
    found = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".cpp", ".hip", ".hpp")) or name in LAYER:
            continue
        lines = open(os.path.join(CSRC, name)).read().split("\n")
        for index, line in enumerate(lines):
            statement = line
            if re.match(r"^\s+(?:heamd::)?(?:Scratch|ZeroizedWorkspace) \w+\(", line):
                end = index
                while ";" not in lines[end]:  # a declaration over several lines
                    end += 1
                statement = " ".join([line] + [other.strip() for other in lines[index + 1: end + 1]])
            match = DECLARATION.match(statement)
            direct = "scratch_allocate(" in line
            if not match and not direct:
                continue
            above = index
            while above >= 0 and not FUNCTION.match(lines[above]):
                above -= 1
            assert above >= 0, (name, index + 1)
            function = FUNCTION.match(lines[above]).group(1)
            names = " ".join(n for n in re.findall(r"(\w+)\(", match.group(1)) if n != "as_stream") if match else "scratch_allocate"
            found.append((name, function, names))
    return found


def test_the_table_lists_exactly_the_sites_of_the_source():
    found = sites_in_source()
    listed = [(s.file, s.function, s.names) for s in S.SITES]
    assert len(found) > 50  # the pattern still finds them
    assert len(set(found)) == len(found), "two sites of one function declare the same names: %s" % sorted(
        s for s in found if found.count(s) > 1)
    missing = sorted(set(found) - set(listed))
    stale = sorted(set(listed) - set(found))
    assert not missing and not stale, "not in tests/scratch_sites.py: %s; no longer in csrc/: %s" % (missing, stale)
    assert len(listed) == len(set(listed))


def test_every_entry_is_in_the_header():
    header = open(HEADER).read()
    for s in S.SITES:
        assert re.search(r"\b%s\(" % re.escape(s.entry), header), s


def test_every_case_exists():
    rows = {row.name for row in A.CASES}
    for s in S.SITES:
        if s.case is None:
            continue
        if s.case in S.DELEGATED:
            module, function, given = S.DELEGATED[s.case]
            tree = ast.parse(open(os.path.join(ROOT, "tests", module + ".py")).read())
            definitions = {node.name: node for node in tree.body if isinstance(node, ast.FunctionDef)}
            assert function in definitions, s
            parameters = [a.arg for a in definitions[function].args.args]
            assert set(given) <= set(parameters) and set(parameters) - set(given) <= set(S.FIXTURES), (s, parameters)
        else:
            assert s.case in F.WORKSPACE and s.case in rows, s
            assert s.case == s.entry or s.case + "_u32" == s.entry, s
    used = {s.case for s in S.SITES}
    assert set(S.DELEGATED) <= used, "cases no site names: %s" % sorted(set(S.DELEGATED) - used)
    # every workspace-taking row is a case of the poison test; each reaches a site of this table
    assert set(F.WORKSPACE) >= {s.case for s in S.SITES if s.case is not None and s.case not in S.DELEGATED}


def test_sites_without_a_case_keep_to_the_limits():
    other = []
    for s in S.SITES:
        assert (s.case is None) == (s.reached is not None), s
        if s.case is not None:
            continue
        if s.file == "device_group.cpp" or s.reached.endswith(S.SECOND_DEVICE):
            continue
        assert "`" in s.reached, "a site is left out only with the source condition that keeps a small shape away: %s" % (s,)
        other.append(s)
    assert len(other) <= MAX_OTHER_EXEMPT, other
