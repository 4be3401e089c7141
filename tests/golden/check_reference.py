"""Holds the Swift goldens of this directory against a checkout of the reference (swift-homomorphic-encryption).  The
tests read only the committed goldens; run this where a checkout exists, after either side moves:

    python tests/golden/check_reference.py PATH/TO/swift-homomorphic-encryption [--write]

  * noop_scheme_members.json: the static members NoOpScheme declares, and the accelerated requirements HeScheme declares;
  * reference_swift_api.json: the label lists the package's calls resolve to, as the checkout declares them;
  * reference_bfv_suite_calls.json: the HeAPITestHelpers the reference's runBfvTests calls;
  * swift_protocol_signatures.json: HeScheme's and PirUtilProtocol's requirements, aliases and defaults (--write
    rewrites it from the checkout).

Exit status 1 when a golden differs from the checkout.
"""
import glob
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import swift_types as st  # noqa: E402
import test_swift_reference_api as api  # noqa: E402
from swift_source import static_members  # noqa: E402


def _read(*paths):
    return "\n".join(open(p).read() for p in paths)


def noop_scheme_members(sources):
    """(was tests/test_swift_package.py::test_the_golden_member_list_is_the_reference_s)"""
    golden = json.load(open(os.path.join(HERE, "noop_scheme_members.json")))
    he = os.path.join(sources, "HomomorphicEncryption")
    noop = static_members(_read(os.path.join(he, "NoOpScheme.swift")), "NoOpScheme")
    protocol = static_members(_read(os.path.join(he, "HeScheme.swift")), "HeScheme", kind="protocol")
    problems = [] if sorted(noop) == golden["noop_scheme_static_members"] else ["NoOpScheme's static members differ"]
    problems += ["HeScheme lacks %s" % r for r in golden["accelerated_protocol_requirements"] if r not in protocol]
    return problems


def reference_swift_api(sources):
    """(was tests/test_swift_reference_api.py::test_committed_reference_declarations_match_the_checkout)"""
    golden_by_name, golden_bare = api._reference_from_golden()
    checkout_by_name, checkout_bare = api._collect(glob.glob(os.path.join(sources, "**", "*.swift"), recursive=True))
    problems = ["label lists of %s differ" % name for name, label_lists in golden_by_name.items()
                if sorted(label_lists) != sorted(list(l) for l in {tuple(x) for x in checkout_by_name.get(name, [])})]
    problems += ["%s is not declared" % name for name in sorted(golden_bare - checkout_bare)]
    unresolved, _ = api._resolve(checkout_by_name, checkout_bare)
    problems += ["unresolved against the checkout: %s(%s)" % (n, ":".join(l)) for _, n, l, _ in unresolved]
    return problems


def bfv_suite_calls(checkout):
    """(was the checkout branch of tests/test_swift_reference_api.py::test_reference_suites_cover_what_the_reference_runs_for_bfv)"""
    golden = json.load(open(os.path.join(HERE, "reference_bfv_suite_calls.json")))
    body = _read(os.path.join(checkout, "Tests", "HomomorphicEncryptionTests", "HeAPITests.swift"))
    body = body[body.index("private func runBfvTests"):body.index("func bfvUInt32")]
    if sorted(set(re.findall(r"HeAPITestHelpers\.(\w+)\(", body))) != sorted(golden["helpers"]):
        return ["the HeAPITestHelpers runBfvTests calls differ"]
    return []


def protocol_signatures(sources):
    """What tests/golden/swift_protocol_signatures.json holds, derived from the checkout."""
    he = _read(os.path.join(sources, "HomomorphicEncryption", "HeScheme.swift"))
    he_extensions = _read(os.path.join(sources, "HomomorphicEncryption", "HeScheme.swift"),
                          os.path.join(sources, "HomomorphicEncryption", "HeSchemeAsync.swift"))
    pir = _read(os.path.join(sources, "PrivateInformationRetrieval", "IndexPir", "PirUtil.swift"))
    derived = {
        "source": "HeScheme.swift:190-1090 + extensions (HeScheme.swift, HeSchemeAsync.swift); PirUtil.swift:22-147 + extension "
                  "(reference checkout of this build)",
        "HeScheme": {
            "requirements": st.static_function_signatures(he, "HeScheme", kinds=("protocol",)),
            "aliases": st.typealiases(he, "HeScheme", kinds=("protocol",)),
            "defaults": st.static_function_signatures(he_extensions, "HeScheme", kinds=("extension",)),
        },
        "PirUtilProtocol": {
            "requirements": st.static_function_signatures(pir, "PirUtilProtocol", kinds=("protocol",)),
            "aliases": st.typealiases(pir, "PirUtilProtocol", kinds=("protocol",)),
            "defaults": st.static_function_signatures(pir, "PirUtilProtocol", kinds=("extension",)),
        },
    }
    return json.loads(json.dumps(derived))  # tuples -> lists, as JSON round-trips them


def main():
    args = [a for a in sys.argv[1:] if a != "--write"]
    if len(args) != 1:
        raise SystemExit(__doc__)
    sources = os.path.join(args[0], "Sources")
    problems = noop_scheme_members(sources) + reference_swift_api(sources) + bfv_suite_calls(args[0])
    path = os.path.join(HERE, "swift_protocol_signatures.json")
    derived = protocol_signatures(sources)
    if json.load(open(path)) != derived:
        if "--write" in sys.argv:
            with open(path, "w") as f:
                json.dump(derived, f, indent=1, sort_keys=True)
                f.write("\n")
            print("rewrote", path)
        else:
            problems.append("swift_protocol_signatures.json differs from the checkout (--write rewrites it)")
    for problem in problems:
        print(problem)
    print("goldens match the checkout" if not problems else "%d difference(s)" % len(problems))
    return 1 if problems else 0


if __name__ == "__main__":
    sys.exit(main())
