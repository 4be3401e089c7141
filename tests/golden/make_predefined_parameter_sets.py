"""Writes tests/golden/predefined_parameter_sets.json: the values of every PredefinedRlweParameters case of the reference
(Sources/HomomorphicEncryption/EncryptionParameters.swift, the `static let NAME = ParameterSet(...)` literals) -- name, degree,
plaintext modulus, coefficient moduli, supportsScalar32, errorStdDev and where the literal stands.  Values only: every modulus
is evaluated from its expression and held to the number in the comment next to it.  Run in the build container (reads
/root/reference); tests/predefined_sets.py reads the JSON and never this script.

    python tests/golden/make_predefined_parameter_sets.py            # writes the file
    python tests/golden/make_predefined_parameter_sets.py --check    # exit status 1 if the file differs from the reference
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = "Sources/HomomorphicEncryption/EncryptionParameters.swift"
REFERENCE = os.path.join("/root/reference", SOURCE)
TARGET = os.path.join(HERE, "predefined_parameter_sets.json")

_TERM = re.compile(r"\(1 << (\d+)\)|([0-9_]+)|([+-])")


def value_of(expression):
    """`(1 << 14) + 33`, `(1 << 29) - 180_223`: powers of two, decimal literals, + and -"""
    total, sign, rest = 0, 1, expression.strip()
    while rest:
        match = _TERM.match(rest)
        if not match:
            raise ValueError("not a modulus expression: %r" % expression)
        shift, literal, operator = match.groups()
        if operator:
            sign = 1 if operator == "+" else -1
        else:
            total += sign * (1 << int(shift) if shift else int(literal.replace("_", "")))
        rest = rest[match.end():].lstrip()
    return total


def commented(line):
    """(value of the expression, the number in the trailing comment) of `EXPR, // 1234` """
    code, _, comment = line.partition("//")
    value = value_of(code.split(":", 1)[-1].strip().rstrip(","))
    stated = int(re.sub(r"[^0-9]", "", comment))
    if value != stated:
        raise ValueError("%r: the expression gives %d" % (line.strip(), value))
    return value


def parameter_sets(text):
    lines = text.splitlines()
    first = next(i for i, line in enumerate(lines) if re.match(r"public enum PredefinedRlweParameters\b", line))
    last = next(i for i, line in enumerate(lines) if i > first and "struct ParameterSet" in line)
    cases = [m.group(1) for line in lines[first:last] for m in [re.match(r"\s*case (\w+)\s*(//.*)?$", line)] if m]
    found = {}
    for number, line in enumerate(lines, 1):
        head = re.match(r"\s*static let (\w+) = ParameterSet\($", line)
        if not head:
            continue
        entry = {"name": head.group(1), "source": "%s:%d" % (SOURCE, number), "coefficientModuli": []}
        at, in_moduli = number, False
        while True:
            body = lines[at].strip()
            at += 1
            if in_moduli:
                if body.startswith("]"):
                    in_moduli = False
                else:
                    entry["coefficientModuli"].append(commented(body))
            elif body.startswith("polyDegree:"):
                entry["degree"] = int(body.split(":")[1].strip().rstrip(","))
            elif body.startswith("errorStdDev:"):
                entry["errorStdDev"] = body.split(".")[1].rstrip(",")
            elif body.startswith("plaintextModulus:"):
                entry["plaintextModulus"] = commented(body)
            elif body.startswith("coefficientModuli:"):
                in_moduli = True
            elif body.startswith("supportsScalar32:"):
                entry["supportsScalar32"] = {"true": True, "false": False}[body.split(":")[1].strip().rstrip(")")]
                break
        found[entry["name"]] = entry
    if sorted(found) != sorted(cases):
        raise ValueError("enum cases and ParameterSet literals differ: %s" % sorted(set(found) ^ set(cases)))
    order = ("name", "degree", "plaintextModulus", "coefficientModuli", "supportsScalar32", "errorStdDev", "source")
    return [{key: found[name][key] for key in order} for name in cases]


def render(sets):
    return json.dumps({"source": "PredefinedRlweParameters, " + SOURCE, "sets": sets}, indent=1) + "\n"


if __name__ == "__main__":
    text = render(parameter_sets(open(REFERENCE).read()))
    if sys.argv[1:] not in ([], ["--check"]):
        sys.exit(__doc__)
    if "--check" in sys.argv[1:]:
        if not os.path.exists(TARGET) or open(TARGET).read() != text:
            print("predefined_parameter_sets.json differs from", REFERENCE)
            sys.exit(1)
        print("predefined_parameter_sets.json matches the reference:", text.count('"name"'), "sets")
    else:
        open(TARGET, "w").write(text)
        print(text.count('"name"'), "parameter sets ->", TARGET)
